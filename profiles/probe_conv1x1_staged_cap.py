"""Launches of more than one round of workgroups, and the 256-pixel tiles (16-channel stages), on the float4-staged bx3 1x1 kernel against the
generic kernel (kernels.CONV1X1_STAGED on / off; c1_staged_ok<SCH_BX3> in csrc/tdr_conv_bx3.hip has no workgroup cap -- these lines are why).  A cap can
be tried in a TUNING build of the library:
    make -C textualdegremoval_amd/csrc variant VFILE=tdr_conv_bx3 VFLAGS=-DTDR_TUNING_KNOBS VOUT=../libtdr_hip_tune.so
    TDR_LIB_PATH=textualdegremoval_amd/libtdr_hip_tune.so TDR_C1_BLOCKS=512 python profiles/probe_conv1x1_staged_cap.py
usage: python profiles/probe_conv1x1_staged_cap.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from textualdegremoval_amd import kernels as K
K.set_math('bx3')
torch.manual_seed(0)


def t(N, Cin, Cout, H):
    xs = [torch.randn(N, Cin, H, H, device='cuda') for _ in range(2)]
    wp, mp, *_ = K.pack_weights(torch.randn(Cout, Cin, 1, 1, device='cuda') * 0.05, K.PACK_FWD)
    outs = [torch.empty(N, Cout, H, H, device='cuda') for _ in range(2)]
    line = f'1x1 {Cin}->{Cout} @{H} N{N}:'
    for on in (False, True):
        K.CONV1X1_STAGED = on
        staged = K.conv1x1_staged_takes(xs[0], wp, mp, Cout, 1, out=outs[0])
        f = lambda i: K.conv_forward(xs[i & 1], wp, mp, Cout, 1, out=outs[i & 1])
        for i in range(3): f(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                for i in range(20): f(i)
        g.replay(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5): g.replay()
        e1.record(); torch.cuda.synchronize()
        line += f'  {"staged " if staged else "generic"} {e0.elapsed_time(e1) / 100 * 1e3:6.1f} us'
    K.CONV1X1_STAGED = True
    print(line, flush=True)


for (Cin, Cout, H) in [(512, 1024, 64), (1024, 512, 64), (512, 512, 64), (256, 512, 128), (256, 256, 128), (128, 256, 256)]:
    t(4, Cin, Cout, H)
print('256-pixel tiles (16-channel stages: one barrier per 16 channels as in the generic kernel, only the load width differs):', flush=True)
for (N, Cin, Cout, H) in [(8, 64, 32, 256), (8, 256, 32, 128), (8, 256, 64, 128), (8, 512, 64, 128), (4, 64, 32, 512)]:
    t(N, Cin, Cout, H)                                      # 32 x 256: Cout <= 32 and >= 512 such blocks; 64 x 256: Cout <= 64 likewise
