"""The Restormer-family networks (restormer_engine / promptir_engine / drsformer_engine net_fwd, net_bwd: they reach the deferred-leaf
scheduler through restormer_engine._pw_bwd) on seeded weights: one forward and one backward with a fixed cotangent per case, for comparing
two trees (or two runs of one tree) bit for bit.  The sibling of profiles/probe_nafnet_family.py: same result files, same `cmp` / `trace`.

    python profiles/probe_restormer_family.py run OUT.json [--tree DIR] [--math bx3,f32,hx2]
    python profiles/probe_nafnet_family.py cmp A.json B.json
    python profiles/probe_nafnet_family.py trace TRACE_DIR OUT.txt
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from probe_nafnet_family import MODES, cotangent, sha  # noqa: E402

SMALL = dict(num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1])
# (name, engine module, oracle module, cfg overrides, (N, H, W), guided)
CASES = [('restormer_guided_2x64x64', 'restormer_engine', 'restormer_ref_oracle', {}, (2, 64, 64), True),
         ('restormer_guided_1x120x100_pad', 'restormer_engine', 'restormer_ref_oracle', {}, (1, 120, 100), True),
         ('restormer_2x64x64', 'restormer_engine', 'restormer_ref_oracle', {}, (2, 64, 64), False),
         ('promptir_guided_2x64x64', 'promptir_engine', 'promptir_ref_oracle', SMALL, (2, 64, 64), True),
         ('promptir_2x64x64', 'promptir_engine', 'promptir_ref_oracle', SMALL, (2, 64, 64), False),
         ('drsformer200l_guided_2x64x64', 'drsformer_engine', 'drsformer_ref_oracle', {}, (2, 64, 64), True),
         # (the un-guided DRSformer class has the MEFC sub-networks: cfg['mefc'], full_synth_params)
         ('drsformer_2x64x64', 'drsformer_engine', 'drsformer_ref_oracle', dict(dim=16, nf=16, heads=[1, 2, 2, 4], mefc=True), (2, 64, 64), False)]


def run(out_json, modes):
    import importlib
    import numpy as np
    import torch
    from oracle import nafnet_ref_oracle as NO
    from textualdegremoval_amd import kernels as K
    res, keep = {}, {}
    for mode in modes:
        K.set_math(mode)
        scale = 65536.0 if mode == 'hx2' else 1.0       # hx2: a loss-scaled backward (the fp16-pair data-gradient packs)
        prev = K.set_grad_scaled(mode == 'hx2')
        try:
            for case, eng, orc, kw, (N, H, W), guided in CASES:
                M = importlib.import_module('textualdegremoval_amd.' + eng)
                O = importlib.import_module('oracle.' + orc)
                cfg = O.default_cfg(**kw)
                synth = O.full_synth_params if cfg.get('mefc') else O.synth_params
                P = {k: v.cuda().contiguous() for k, v in synth(cfg, seed=3).items()}
                lq, _, ref = NO.synth_pair(N, H, W, seed=1237)
                out, saved = M.net_fwd(P, cfg, lq.cuda(), ref.cuda() if guided else None)
                G = M.net_bwd(cotangent(torch, out.shape, 5, scale), P, cfg, saved)
                torch.cuda.synchronize()
                res[f'{case}/{mode}'] = dict(out=sha(out), keys=list(G.keys()), grads={k: sha(v) for k, v in G.items()})
                for k, v in G.items():
                    if k.startswith('masa_enc.') and v.numel() <= 40000:
                        keep[f'{case}/{mode}/{k}'] = v.detach().cpu().numpy()
                print(case, mode, 'done', len(G), 'gradients', flush=True)
                del P, saved, G, out
        finally:
            K.set_grad_scaled(prev)
    json.dump(dict(env={k: os.environ.get(k) for k in ('TDR_FORCE_DP_SCHEDULE', 'TDR_DETERMINISTIC')}, cases=res), open(out_json, 'w'), indent=1)
    np.savez_compressed(os.path.splitext(out_json)[0] + '.npz', **keep)


if __name__ == '__main__':
    args = sys.argv[1:]
    opt = {}
    for flag in ('--tree', '--math'):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    if not args or args[0] != 'run':
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(opt.get('--tree', os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
    run(args[1], opt.get('--math', ','.join(MODES)).split(','))
