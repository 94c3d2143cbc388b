"""calculate_niqe on a 1280 x 720 BGR uint8 image (7 x 13 blocks of 96 after the crop of niqe()): HIP-event times of the whole call
(host colour conversion, upload, the five launches of tdr_niqe_features, download, the float64 36 x 36 tail) and of the device part
alone (kernels.niqe_features on a resident Y plane).  Warm-up, then the median of 30 calls each.  The pristine parameters are the
synthetic ones of tests/golden/niqe.npz.  Writes one JSON object:   python profiles/probe_niqe.py [out.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd.metrics import calculate_niqe, to_y_channel  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'niqe', 'probe_niqe.json')
H, W, CALLS, WARMUP = 720, 1280, 30, 5
assert torch.cuda.is_available(), 'probe_niqe needs the GPU'


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


g = np.load(os.path.join(ROOT, 'tests', 'golden', 'niqe.npz'))
pris = {k: g[k] for k in ('mu_pris_param', 'cov_pris_param', 'gaussian_window')}
rng = np.random.default_rng(3)
yy, xx = np.mgrid[0:H, 0:W]
img = np.clip(120 + 60 * np.sin(yy / 17.0)[..., None] * np.cos(xx / 23.0)[..., None] + rng.normal(0, 20, (H, W, 3)), 0, 255).astype(np.uint8)
score = float(np.squeeze(calculate_niqe(img, 0, pris_params=pris)))
y = np.squeeze(to_y_channel(img.astype(np.float32)))[:H // 96 * 96, :W // 96 * 96]
yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
call = median_ms(lambda: calculate_niqe(img, 0, pris_params=pris))
dev = median_ms(lambda: K.niqe_features(yd, pris['gaussian_window'], 96))
res = dict(probe='niqe', image=[H, W], blocks=[H // 96, W // 96], calls=CALLS, warmup=WARMUP, score=score,
           calculate_niqe_ms=dict(median=round(call[0], 3), min=round(call[1], 3), max=round(call[2], 3)),
           niqe_features_ms=dict(median=round(dev[0], 3), min=round(dev[1], 3), max=round(dev[2], 3)),
           device=torch.cuda.get_device_name(0), torch=torch.__version__)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
