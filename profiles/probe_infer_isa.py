"""What the compiler makes of the forward-only NAFBlock chains (csrc/tdr_nafblock_infer.hip: tdr_nafblock.hip with KEEP = false), read from
the gfx950 assembly -- no GPU needed.
  * per kernel (naf_tail_fwd_kernel / naf_head_fwd_kernel, C x arithmetic), KEEP = true | false: instructions, global stores, VGPRs, spilled
    VGPRs, scratch bytes;
  * both sets of instantiations compiled in ONE translation unit: how many kernels of each set then differ (labels aside) from the
    separately compiled ones.
Writes profiles/infer/probe_infer_isa.json (or `--out PATH`).   python profiles/probe_infer_isa.py [--out PATH] [--hipcc PATH]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'textualdegremoval_amd', 'csrc')
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'infer', 'probe_infer_isa.json'))
ap.add_argument('--hipcc', default=os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))
a = ap.parse_args()
# the flags of csrc/Makefile for tdr_nafblock.o / tdr_nafblock_infer.o
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-fno-slp-vectorize', '-I' + CSRC,
         '--cuda-device-only', '-S']
ONE_TU = '''#include "tdr_nafblock.hip"
extern "C" int tdr_naf_tail_infer(const TdrNafTailDesc* d, void* s) { return naf_tail_fwd_launch<false>(d, s); }
extern "C" int tdr_naf_head_infer(const TdrNafHeadFwdDesc* d, void* s) { return naf_head_fwd_launch<false>(d, s); }
'''
KERNEL = re.compile(r'naf_(tail|head)_fwd_kernelILi(\d+)ELb([01])ELi(\d+)E')


def asm(src, tmp, name):
    out = os.path.join(tmp, name + '.s')
    subprocess.run([a.hipcc] + FLAGS + [src, '-o', out], check=True, cwd=CSRC)
    return open(out).read()


def kernels(text):
    """{(half, C, keep, sch): dict(instructions, global_stores, vgprs, scratch_bytes, vgpr_spills)}"""
    res = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end', text, re.M | re.S):
        sym, k = m.group(1), KERNEL.search(m.group(1))
        if not k:
            continue
        ins = [re.sub(r'\s*;.*$', '', ln).strip() for ln in m.group(2).splitlines()]
        ins = [re.sub(r'\.LBB\d+_', '.LBB_', ln) for ln in ins if ln and not ln.startswith('.')]      # (labels carry the function's index)

        def num(pattern):
            return int(re.search(pattern, text, re.S).group(1))
        res[(k.group(1), int(k.group(2)), bool(int(k.group(3))), int(k.group(4)))] = dict(
            sha=hashlib.sha256('\n'.join(ins).encode()).hexdigest()[:16], instructions=len(ins),
            global_stores=sum(ln.startswith('global_store') for ln in ins),
            vgprs=num(r'\.set ' + sym + r'\.num_vgpr, (\d+)'), scratch_bytes=num(r'\.set ' + sym + r'\.private_seg_size, (\d+)'),
            vgpr_spills=num(r'\.name:\s+' + sym + r'\n.*?\.vgpr_spill_count:\s+(\d+)'))
    return res


with tempfile.TemporaryDirectory() as tmp:
    ks = kernels(asm('tdr_nafblock.hip', tmp, 'train'))
    assert ks and all(k[2] for k in ks), 'tdr_nafblock.hip holds the KEEP = true kernels alone'
    ki = kernels(asm('tdr_nafblock_infer.hip', tmp, 'infer'))
    assert ki and not any(k[2] for k in ki), 'tdr_nafblock_infer.hip holds the KEEP = false kernels alone'
    ks.update(ki)
    with open(os.path.join(tmp, 'one_tu.hip'), 'w') as f:
        f.write(ONE_TU)
    one = kernels(asm(os.path.join(tmp, 'one_tu.hip'), tmp, 'one'))
differ = {keep: sum(one[k]['sha'] != ks[k]['sha'] for k in ks if k[2] == keep) for keep in (True, False)}
for d in list(ks.values()):
    del d['sha']
rows = []
for half, c, keep, sch in sorted(ks):
    if keep:
        rows.append(dict(kernel=f'naf_{half}_fwd_kernel', C=c, sch=sch, keep=ks[(half, c, True, sch)], forward_only=ks[(half, c, False, sch)]))
res = dict(probe='infer_isa', arch='gfx950', hipcc=subprocess.run([a.hipcc, '--version'], capture_output=True, text=True).stdout.splitlines()[0],
           kernels=rows, one_translation_unit=dict(training_kernels=len(rows), training_kernels_that_differ=differ[True],
                                                   forward_only_kernels=len(rows), forward_only_kernels_that_differ=differ[False]))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res['one_translation_unit']))
