"""What the compiler makes of the fused NAFBlock chains and the depthwise stencils, read from the gfx950 assembly -- no GPU needed.
Units: csrc/tdr_nafblock.hip (training), tdr_nafblock_infer.hip (forward-only), tdr_dyn_infer.hip (modulated forward-only + its stencil),
tdr_dwsg.hip and tdr_nafblock_local.hip (the TLSC tail), each compiled with the flags csrc/Makefile gives its object.
  * per unit and kernel: a hash of the instruction stream (labels normalised, comments stripped), instructions, global stores, VGPRs,
    spilled VGPRs, scratch bytes, static LDS bytes, kernarg bytes.  A kernel is keyed by what it is, not by its mangled name:
    chain kernels `tail|head|bwd C=.. KEEP|HEAD=.. sch=.. mod=..`, every other kernel `name<template arguments>`;
  * the training and the forward-only instantiations compiled in ONE translation unit: how many kernels of each set then differ from
    the separately compiled ones (the recorded reason the units are separate).
Writes profiles/nafchain/isa.json (or `--out PATH`).  `--against OTHER.json` compares the fresh result with a recorded one kernel by
kernel (hash, VGPRs, spills, scratch, LDS, kernarg bytes) and exits 1 when any differ; a unit the recorded file does not have is
not compared.
    python profiles/probe_infer_isa.py [--out PATH] [--against PATH] [--hipcc PATH]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'textualdegremoval_amd', 'csrc')
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nafchain', 'isa.json'))
ap.add_argument('--against', default=None)
ap.add_argument('--hipcc', default=os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'))
a = ap.parse_args()
UNITS = ['tdr_nafblock', 'tdr_nafblock_infer', 'tdr_dyn_infer', 'tdr_dwsg', 'tdr_nafblock_local']
# the flags of csrc/Makefile for these objects (all of them are on its no-SLP list)
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-fno-slp-vectorize', '-I' + CSRC,
         '--cuda-device-only', '-S']
ONE_TU = '#include "tdr_nafblock.hip"\n#include "tdr_nafblock_infer.hip"\n'      # (both include tdr_nafblock_chain.h, once)
MANGLED = re.compile(r'_ZN12_GLOBAL__N_1(\d+)')      # <length><name>[I<template arguments>E]
SHARED_SINCE = {'dyn_pool_finish_kernel': 'dw_pool_finish_kernel'}      # (the stencil helpers the modulated unit once held copies of)
COMPARED = ('sha', 'vgprs', 'vgpr_spills', 'scratch_bytes', 'lds_bytes', 'kernarg_bytes')


def asm(src, tmp, name):
    out = os.path.join(tmp, name + '.s')
    subprocess.run([a.hipcc] + FLAGS + [src, '-o', out], check=True, cwd=CSRC)
    return open(out).read()


def key_of(sym, unit):
    m = MANGLED.match(sym)
    if not m:
        return sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    t = re.match(r'I((?:L[ib]\d+E)+)E', rest)
    targs = [int(v) for v in re.findall(r'L[ib](\d+)E', t.group(1))] if t else []
    chain = re.fullmatch(r'naf_(tail|head)_(fwd|bwd)_kernel', name)
    if chain and chain.group(2) == 'fwd':
        # (before the modulation was a template argument, the modulated unit's kernels carried three arguments like the others')
        mod = targs[3] if len(targs) > 3 else int(unit == 'tdr_dyn_infer')
        return f'{chain.group(1)} C={targs[0]} KEEP={targs[1]} sch={targs[2]} mod={mod}'
    if chain:
        return f'bwd C={targs[0]} HEAD={targs[1]} sch={targs[2]}'
    name = SHARED_SINCE.get(name, name)
    return name + ('<' + ', '.join(map(str, targs)) + '>' if targs else '')


def kernels(text, unit):
    """{key: dict(sha, instructions, global_stores, vgprs, vgpr_spills, scratch_bytes, lds_bytes, kernarg_bytes)}"""
    res = {}
    entry = set(re.findall(r'^\s*\.amdhsa_kernel (\S+)', text, re.M))
    for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end', text, re.M | re.S):
        sym = m.group(1)
        if sym not in entry:
            continue
        ins = [re.sub(r'\s*;.*$', '', ln).strip() for ln in m.group(2).splitlines()]
        ins = [re.sub(r'\.LBB\d+_', '.LBB_', ln) for ln in ins if ln and not ln.startswith('.')]      # (labels carry the function's index)

        def num(pattern):
            return int(re.search(pattern, text, re.S).group(1))
        key = key_of(sym, unit)
        assert key not in res, key
        res[key] = dict(
            sha=hashlib.sha256('\n'.join(ins).encode()).hexdigest()[:16], instructions=len(ins),
            global_stores=sum(ln.startswith('global_store') for ln in ins),
            vgprs=num(r'\.set ' + sym + r'\.num_vgpr, (\d+)'), vgpr_spills=num(r'\.name:\s+' + sym + r'\n.*?\.vgpr_spill_count:\s+(\d+)'),
            scratch_bytes=num(r'\.set ' + sym + r'\.private_seg_size, (\d+)'),
            lds_bytes=num(r'\.amdhsa_kernel ' + sym + r'\n\s*\.amdhsa_group_segment_fixed_size (\d+)'),
            kernarg_bytes=int(re.findall(r'\.kernarg_segment_size:\s+(\d+)', text[:re.search(r'\.name:\s+' + sym + r'\n', text).start()])[-1]))
    assert len(res) == len(entry), (unit, sorted(entry))
    return res


def differing(x, y):
    return sorted(k for k in x if k not in y or any(x[k][f] != y[k][f] for f in COMPARED))


with tempfile.TemporaryDirectory() as tmp:
    units = {u: kernels(asm(u + '.hip', tmp, u), u) for u in UNITS}
    train = {k: v for k, v in units['tdr_nafblock'].items() if ' KEEP=' in k}
    infer = units['tdr_nafblock_infer']
    assert train and all(' KEEP=1 ' in k for k in train), 'tdr_nafblock.hip holds the KEEP = true forward kernels alone'
    assert infer and all(' KEEP=0 ' in k and k.endswith('mod=0') for k in infer), 'tdr_nafblock_infer.hip holds the plain KEEP = false kernels alone'
    assert all(k.endswith('mod=1') for k in units['tdr_dyn_infer'] if ' KEEP=' in k), 'tdr_dyn_infer.hip holds modulated chains alone'
    with open(os.path.join(tmp, 'one_tu.hip'), 'w') as f:
        f.write(ONE_TU)
    one = kernels(asm(os.path.join(tmp, 'one_tu.hip'), tmp, 'one'), 'one')
one_tu = dict(training_kernels=len(train), training_kernels_that_differ=len(differing(train, one)),
              forward_only_kernels=len(infer), forward_only_kernels_that_differ=len(differing(infer, one)))
res = dict(probe='nafchain_isa', arch='gfx950', hipcc=subprocess.run([a.hipcc, '--version'], capture_output=True, text=True).stdout.splitlines()[0],
           units={u: dict(sorted(ks.items())) for u, ks in units.items()}, one_translation_unit=one_tu)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(one_tu))
if a.against:
    other = json.load(open(a.against))['units']
    diff = {u: differing(units[u], other[u]) + [k for k in other[u] if k not in units[u]] for u in UNITS if u in other}
    print(json.dumps(dict(against=a.against, kernels_compared=sum(len(units[u]) for u in diff),
                          kernels_that_differ=sum(map(len, diff.values())), differ={u: d for u, d in diff.items() if d})))
    sys.exit(1 if any(diff.values()) else 0)
