"""Instruction streams of two builds of a convolution unit, kernel by kernel -- no GPU needed.  Each argument pair is the gfx950
assembly of one unit before and after a change, made with the flags csrc/Makefile gives the object plus `--cuda-device-only -S`:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result --cuda-device-only -S tdr_conv_bx3.hip -o after_bx3.s
Streams are compared the way profiles/probe_infer_isa.py does it (comments stripped, labels normalised), together with VGPRs, spills and
scratch.  A kernel is keyed by its role and template arguments, not its name: the float4-staged 1x1 kernels conv1x1_hx2_kernel<WM, TM,
TN, EPI, GATE, SCH> and conv1x1_bx3s_kernel<WM, TM, TN, EPI, GATE> (SCH = 0) of the older build are conv1x1_staged_kernel<..., SCH>.
    python profiles/conv1x1_staged/compare_isa.py before_bx3.s after_bx3.s [before_p16.s after_p16.s]"""
import hashlib
import re
import sys

MANGLED = re.compile(r'_ZN12_GLOBAL__N_1(\d+)')


def key_of(sym):
    m = MANGLED.match(sym)
    if not m:
        return sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    t = re.match(r'I((?:L[ib]\d+E)+)E', rest)
    targs = [int(v) for v in re.findall(r'L[ib](\d+)E', t.group(1))] if t else []
    if name == 'conv1x1_bx3s_kernel':
        name, targs = 'conv1x1_staged_kernel', targs + [0]
    elif name == 'conv1x1_hx2_kernel':
        name = 'conv1x1_staged_kernel'
    return name + ('<' + ', '.join(map(str, targs)) + '>' if targs else '')


def kernels(path):
    text, res = open(path).read(), {}
    entry = set(re.findall(r'^\s*\.amdhsa_kernel (\S+)', text, re.M))
    for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end', text, re.M | re.S):
        sym = m.group(1)
        if sym not in entry:
            continue
        ins = [re.sub(r'\s*;.*$', '', ln).strip() for ln in m.group(2).splitlines()]
        ins = [re.sub(r'\.LBB\d+_', '.LBB_', ln) for ln in ins if ln and not ln.startswith('.')]
        key = key_of(sym)
        assert key not in res, key
        res[key] = (hashlib.sha256('\n'.join(ins).encode()).hexdigest()[:16], len(ins),
                    int(re.search(r'\.set ' + sym + r'\.num_vgpr, (\d+)', text).group(1)),
                    int(re.search(r'\.name:\s+' + sym + r'\n.*?\.vgpr_spill_count:\s+(\d+)', text, re.S).group(1)),
                    int(re.search(r'\.set ' + sym + r'\.private_seg_size, (\d+)', text).group(1)))
    assert len(res) == len(entry), path
    return res


for before, after in zip(sys.argv[1::2], sys.argv[2::2]):
    x, y = kernels(before), kernels(after)
    assert sorted(x) == sorted(y), ('kernel sets differ', sorted(set(x) ^ set(y)))
    for fam in sorted({k.split('<')[0] for k in x}):
        ks = [k for k in x if k.split('<')[0] == fam]
        diff = [k for k in ks if x[k] != y[k]]
        print(f'{fam}: {len(ks)} kernels, {len(diff)} differ')
        for k in diff:
            print(f'    {k}: (sha, instructions, vgprs, spills, scratch) {x[k]} -> {y[k]}')
