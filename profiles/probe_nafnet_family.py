"""The three callers of the NAFNet U-Net walk (engine.net_*, engine.unet_*, dynfusion_engine.dyn_unet_*) on seeded weights: one forward
and one backward with a fixed cotangent per case, for comparing two trees (or two runs of one tree) bit for bit.

    python profiles/probe_nafnet_family.py run OUT.json [--tree DIR] [--math bx3,f32,hx2] [--only guided|plain]
        every case under every arithmetic mode -> OUT.json: per case the sha256 of the output, of the input / k_v / dK gradients and of
        every parameter gradient, and the order of the gradient keys; OUT.npz: the guided `masa_enc.*` gradients themselves (the only
        tensors behind float atomics unless TDR_DETERMINISTIC=1), for a spread when the hashes differ.
        --tree: import the package and the oracle from DIR (another checkout) instead of this one.
        TDR_FORCE_DP_SCHEDULE=1 / TDR_DETERMINISTIC=1 / TDR_LIB_PATH act through the package as usual.
    python profiles/probe_nafnet_family.py cmp A.json B.json
        -> one line per (case, math): identical, or the tensors that differ (with max |a - b| where both .npz hold them); exit 1 on a difference
    python profiles/probe_nafnet_family.py trace TRACE_DIR OUT.txt
        the kernel-trace CSV of `rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python ... run ... --math bx3`
        -> OUT.txt, one `kernel grid workgroup` line per dispatch in dispatch order (compare two of them with cmp)
"""
import csv
import glob
import hashlib
import json
import os
import re
import sys

MODES = ('bx3', 'f32', 'hx2')
W8 = dict(width=8, nf=8, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1, 1])
HEAD = dict(width=32, nf=32, enc_blk_nums=[1, 1, 1, 28], ext_n_blocks=[4, 4, 4, 4], reffusion_n_blocks=[2, 2, 2, 2, 2])   # bench.py's default
# (name, cfg overrides, (N, H, W), ref (H, W) or None)
GUIDED = [('guided_w8_2x64x64', W8, (2, 64, 64), None), ('guided_w8_1x120x100_pad', W8, (1, 120, 100), None),
          ('guided_w8_1x64x64_ref96', W8, (1, 64, 64), (96, 96)), ('guided_headline_4x512x512', HEAD, (4, 512, 512), None)]
PLAIN_CFG = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 2], dec_blk_nums=[1, 1, 1])
# TLSC boxes per level, written out: smaller than the 64 / 16 maps of levels 0 and 2, covering the 32 / 8 maps of levels 1 and 3
# (engine.tlsc_kernel_sizes scales every level alike, so no train size mixes the two paths in one pass)
LOCAL_KS = [(40, 40), (32, 32), (10, 10), (8, 8)]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:20]


def cotangent(torch, shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * (scale / (shape[1] * shape[2] * shape[3]))).cuda()


def plain_params(torch, O, dyn=False):
    """NAFNet's parameters are the guided network's without the reference branch; the DynamicFusion blocks sit under `.layers.`
    and carry three projections of the 10240 k_v features each"""
    full = O.synth_params(O.default_cfg(**dict(PLAIN_CFG, nf=8, ext_n_blocks=[1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1])), seed=7)
    P = {k: v for k, v in full.items() if not k.startswith('masa_')}
    if not dyn:
        return {k: v.cuda().contiguous() for k, v in P.items()}
    from textualdegremoval_amd import dynfusion_engine as D
    Q = {re.sub(r'^(encoders\.\d+|decoders\.\d+|middle_blks)\.(\d+)\.', r'\1.layers.\2.', k): v for k, v in P.items()}
    g = torch.Generator().manual_seed(11)
    for pre, c in D.block_prefixes(PLAIN_CFG):
        for name, n in zip(D.proj_names(pre), (2 * c, 4 * c, 4 * c)):
            Q[name] = (torch.rand(n, D.KV_DIM, generator=g) * 2 - 1) / 101.0
    return {k: v.cuda().contiguous() for k, v in Q.items()}


def run(out_json, modes, only):
    import numpy as np
    import torch
    from oracle import nafnet_ref_oracle as O
    from textualdegremoval_amd import dynfusion_engine as D, engine as E, kernels as K
    res, keep = {}, {}

    def record(case, mode, out, G, **extra):
        torch.cuda.synchronize()
        r = dict(out=sha(out), keys=list(G.keys()), grads={k: sha(v) for k, v in G.items()})
        r.update({k: sha(v) for k, v in extra.items() if v is not None})
        res[f'{case}/{mode}'] = r
        for k, v in G.items():
            if k.startswith('masa_enc.') and v.numel() <= 40000:
                keep[f'{case}/{mode}/{k}'] = v.detach().cpu().numpy()
        print(case, mode, 'done', flush=True)

    for mode in modes:
        K.set_math(mode)
        scale = 65536.0 if mode == 'hx2' else 1.0       # hx2: a loss-scaled backward (the fp16-pair data-gradient packs)
        prev = K.set_grad_scaled(mode == 'hx2')
        try:
            if only in (None, 'guided'):
                for case, kw, (N, H, W), ref_hw in GUIDED:
                    cfg = O.default_cfg(**kw)
                    P = {k: v.cuda().contiguous() for k, v in O.synth_params(cfg, seed=3).items()}
                    lq, _, ref = O.synth_pair(N, H, W, seed=1237, ref_hw=ref_hw)
                    out, saved = E.net_fwd(P, cfg, lq.cuda(), ref.cuda())
                    G = E.net_bwd(cotangent(torch, out.shape, 5, scale), P, cfg, saved)
                    record(case, mode, out, G)
                    del P, saved, G, out
            if only in (None, 'plain'):
                P = plain_params(torch, O)
                for case, shape in (('nafnet_2x64x64', (2, 3, 64, 64)), ('nafnet_1x60x90_pad', (1, 3, 60, 90))):
                    x = torch.rand(shape, generator=torch.Generator().manual_seed(21)).cuda()
                    out, saved = E.unet_fwd(P, PLAIN_CFG, x)
                    dinp, G = E.unet_bwd(cotangent(torch, out.shape, 6, scale), P, PLAIN_CFG, saved)
                    record(case, mode, out, G, dinp=dinp)
                x = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(22)).cuda()
                out, _ = E.unet_fwd(P, PLAIN_CFG, x, local=LOCAL_KS)
                record('nafnetlocal_1x64x64', mode, out, {})
                P = plain_params(torch, O, dyn=True)
                for case, shape, need_dkv in (('dynfusion_2x64x64_dkv', (2, 3, 64, 64), True), ('dynfusion_2x60x44_pad_nodkv', (2, 3, 60, 44), False)):
                    g = torch.Generator().manual_seed(23)
                    x, kv = torch.rand(shape, generator=g).cuda(), torch.randn(shape[0], 10, 1024, generator=g).cuda()
                    out, saved = D.dyn_unet_fwd(P, PLAIN_CFG, x, kv)
                    dinp, dkv, G, dK = D.dyn_unet_bwd(cotangent(torch, out.shape, 8, scale), P, PLAIN_CFG, saved, need_dkv=need_dkv)
                    assert (dkv is not None) == need_dkv
                    record(case, mode, out, G, dinp=dinp, dkv=dkv, dK=dK)
        finally:
            K.set_grad_scaled(prev)
    json.dump(dict(env={k: os.environ.get(k) for k in ('TDR_FORCE_DP_SCHEDULE', 'TDR_DETERMINISTIC')}, cases=res), open(out_json, 'w'), indent=1)
    np.savez_compressed(os.path.splitext(out_json)[0] + '.npz', **keep)


def cmp(a, b):
    if a.endswith('.txt'):
        la, lb = open(a).read().splitlines(), open(b).read().splitlines()
        first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None if len(la) == len(lb) else min(len(la), len(lb)))
        print(f'{a} vs {b}: {len(la)} / {len(lb)} dispatches,', 'identical sequence' if first is None else f'first difference at dispatch {first}')
        return first is None
    import numpy as np
    A, B = json.load(open(a))['cases'], json.load(open(b))['cases']
    na, nb = (np.load(os.path.splitext(f)[0] + '.npz') for f in (a, b))
    same = sorted(A) == sorted(B)
    for c in sorted(set(A) & set(B)):
        ra, rb = A[c], B[c]
        bad = [k for k in ra if k not in ('grads', 'keys') and ra[k] != rb.get(k)]
        if ra['keys'] != rb['keys']:
            bad.append('ORDER OF THE GRADIENT KEYS')
        for k in ra['grads']:
            if ra['grads'][k] != rb['grads'].get(k):
                key = f'{c}/{k}'
                d = f' (max |a-b| {np.abs(na[key] - nb[key]).max():.3g}, max |a| {np.abs(na[key]).max():.3g})' if key in na.files and key in nb.files else ''
                bad.append(k + d)
        print(f'{c}: {len(ra["grads"])} gradients,', 'bit-identical' if not bad else f'{len(bad)} DIFFER: ' + '; '.join(bad))
        same = same and not bad
    return same


def trace(trace_dir, out_txt):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    dims = [c for c in (rows[0] if rows else {}) if c.startswith(('Grid_Size', 'Workgroup_Size'))]
    with open(out_txt, 'w') as fh:
        for r in rows:
            fh.write(' '.join([re.sub(r'\(.*', '', r['Kernel_Name'])] + [r[c] for c in dims]) + '\n')
    print(out_txt, len(rows), 'dispatches; columns', dims)


if __name__ == '__main__':
    args = sys.argv[1:]
    opt = {}
    for flag in ('--tree', '--math', '--only'):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    if args[0] == 'run':
        sys.path.insert(0, os.path.abspath(opt.get('--tree', os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
        run(args[1], opt.get('--math', ','.join(MODES)).split(','), opt.get('--only'))
    elif args[0] == 'cmp':
        sys.exit(0 if cmp(args[1], args[2]) else 1)
    elif args[0] == 'trace':
        trace(args[1], args[2])
    else:
        sys.exit(__doc__)
