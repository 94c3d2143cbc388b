"""Grouped 3x3 weight gradients on plane tensors (kernels.wgrad3x3_p16_group -> tdr_wgrad3x3_p16_group, csrc/tdr_wgrad_p16.hip): the
weight / bias gradients of the ResidualBlock convolutions of one MASA-encoder level in ONE launch (+ ONE fixed-order reduction, none with
one slice per problem).  Checked per problem against float64 in both plane formats, bit-for-bit across repeated calls and across
permutations of the table, through engine.encoder_bwd with grouping on against grouping off, and under hipGraph replay (the pinned
pointer tables).  Replaces autograd's weight gradients of the reference's ResidualBlocks
(models/archs/network_nafnet_guided_arch.py:44-59,110-143).

Every case asserts through the plan query which path it reaches.  The plan is nsplit = clamp(512 / (nprob * out_tiles), 1, units): with
8 problems of (3, 64, 64, 8, 32) that is 64 slices wanted for 3 units, one unit per workgroup -- so the cases in which one workgroup
walks several units (across strips and images, with partials and with the direct write) use more table rows, which alias a few operand
pairs: the aliases must also agree bit for bit (a problem's bits do not depend on its row)."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_p16 import _encoder_params, rnd

# (N, Cin, Cout, H, W), table rows, distinct operand pairs, what the plan must give
CASES = [
    ((2, 32, 32, 20, 40), 3, 3, 'split'),             # 32 x 32-tile configuration, second strip partial, several chunks
    ((3, 64, 64, 8, 32), 8, 8, 'split'),              # 64 x 64 tiles, an encoder level's 8 problems
    ((1, 256, 256, 8, 32), 8, 8, 'direct'),           # nsplit == 1: direct write, no reduction
    ((2, 48, 80, 19, 45), 2, 2, 'split'),             # Cin != Cout, channel counts that do not fill a tile, odd H and W
    ((3, 64, 64, 8, 32), 256, 4, 'split+walk'),       # 2 slices of 3 units: a workgroup's run of units crosses images
    ((3, 32, 32, 20, 40), 200, 4, 'split+walk'),      # the same on the 32 x 32-tile configuration: across strips and images
    ((2, 256, 256, 8, 32), 32, 4, 'direct+walk'),     # one slice walks both images and writes g / db itself
]
# triple planes hold every fp32 value: also gradients of 2^-30, the size an unscaled backward pass sees.  The fp16 pair's contract is
# operands inside the fp16 window (include/tdr.h: the loss-scaled backward), which 2^-30 is not
FMT_SCALES = [('bx3', 1.0), ('bx3', 2.0 ** -30), ('hx2', 1.0)]


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    prev = kernels.MATH
    kernels.set_math('bx3')
    yield kernels
    kernels.set_math(prev)


def _operands(shape, i):
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(1000 + 2 * i)
    return torch.randn(N, Cin, H, W, generator=g), torch.randn(N, Cout, H, W, generator=g)


def _ref64(x, d):
    """the float64 einsum of tests/test_hip_p24.py::test_wgrad3x3_triple_vs_fp64"""
    N, Cin, H, W = x.shape
    xp = F.pad(x.double(), (1, 1, 1, 1))
    dd = d.double()
    ref = torch.empty(d.shape[1], Cin, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            ref[:, :, ky, kx] = torch.einsum('nchw,nkhw->ck', dd, xp[:, :, ky:ky + H, kx:kx + W])
    return ref, dd.sum((0, 2, 3))


_refs = {}


def _case_refs(shape, distinct):
    """operands and float64 references of a case, computed once and shared by its tests (never modified)"""
    key = (shape, distinct)
    if key not in _refs:
        ops = [_operands(shape, i) for i in range(distinct)]
        _refs[key] = (ops, [_ref64(x, d) for x, d in ops])
    return _refs[key]


def _planes(K, shape, distinct, fmt, scale):
    ops, _ = _case_refs(shape, distinct)
    f = K.FMT_BX3 if fmt == 'bx3' else K.FMT_HX2
    return [(K.p16_from_f32(x.cuda(), fmt=f), K.p16_from_f32((d * scale).cuda(), fmt=f)) for x, d in ops]


def _assert_plan(K, reqs, expect):
    nsplit, units, upw = K.wgrad3x3_p16_group_plan(reqs[0][0], reqs[0][1], len(reqs))
    assert 1 <= nsplit <= units and upw == -(-units // nsplit)
    if 'direct' in expect:
        assert nsplit == 1, (nsplit, units)
    if 'split' in expect:
        assert nsplit > 1, (nsplit, units)
    if 'walk' in expect:
        assert upw > 1, (nsplit, units, upw)
    return nsplit, units, upw


@pytest.mark.parametrize('case', CASES[:4], ids=lambda c: 'x'.join(map(str, c[0])) + f'-{c[1]}')
def test_float64_reference_is_far_inside_the_bounds(case):
    """CPU: the float64 einsum against a second summation order (images and rows reversed, row by row) -- 1e-3 of the bound the kernel is
    held to, so that bound measures the kernel"""
    shape, _, distinct, _ = case
    ops, refs = _case_refs(shape, min(distinct, 2))
    for (x, d), (ref, rb) in zip(ops, refs):
        N, Cin, H, W = x.shape
        xp = F.pad(x.double(), (1, 1, 1, 1))
        dd = d.double()
        ref2 = torch.zeros_like(ref)
        rb2 = torch.zeros_like(rb)
        for n in reversed(range(N)):
            for y in reversed(range(H)):
                for ky in range(3):
                    for kx in range(3):
                        ref2[:, :, ky, kx] += dd[n, :, y, :] @ xp[n, :, y + ky, kx:kx + W].t()
                rb2 += dd[n, :, y, :].sum(1)
        assert (ref - ref2).abs().max().item() < 2e-9 * ref.abs().max().item()
        assert (rb - rb2).abs().max().item() < 2e-9 * rb.abs().max().item()


def test_plan_of_the_encoder_levels():
    """CPU (the plan is host arithmetic): the 8 problems of the five encoder levels of the headline step (N = 8, C = 32 .. 512 at 512^2 ..
    32^2) get 64 / 64 / 16 / 4 / 1 slices per problem -- 512 workgroups each -- where one problem alone is cut into 512 / 512 / 128 / 32 / 8;
    one slice needs no workspace; a single problem in a group keeps the single-problem plan"""
    import ctypes as C
    from textualdegremoval_amd import _lib
    lib = _lib.load()

    def plan(N, Cc, H, nprob):
        d = _lib.TdrWgradP16Desc()
        d.N, d.Cin, d.Cout, d.H, d.W, d.fmt = N, Cc, Cc, H, H, 1
        ns, un, upw = C.c_int(), C.c_int(), C.c_int()
        assert lib.tdr_wgrad3x3_p16_group_plan(C.byref(d), nprob, C.byref(ns), C.byref(un), C.byref(upw)) == 0
        per = lib.tdr_wgrad3x3_p16_group_ws_floats(C.byref(d), nprob)
        assert per == (0 if ns.value == 1 else ns.value * Cc * (Cc * 9 + 1))
        return ns.value, un.value, upw.value, per, lib.tdr_wgrad3x3_p16_ws_floats(C.byref(d))

    got = [plan(8, 32 << l, 512 >> l, 8) for l in range(5)]
    assert [g[0] for g in got] == [64, 64, 16, 4, 1]
    tiles = [1, 1, 4, 16, 64]
    assert all(8 * g[0] * t == 512 for g, t in zip(got, tiles))
    assert all(g[1] % g[0] == 0 and g[2] == g[1] // g[0] for g in got)              # whole images / strips per workgroup
    assert all(8 * g[3] <= g[4] for g in got)                                         # partials per problem: at most 1 / 8 of today's
    single = [plan(8, 32 << l, 512 >> l, 1) for l in range(5)]
    assert [g[0] for g in single] == [512, 512, 128, 32, 8] and all(g[3] == g[4] and g[2] == 1 for g in single)


@pytest.mark.gpu
@pytest.mark.parametrize('fmt,scale', FMT_SCALES)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[0])) + f'-{c[1]}')
def test_group_vs_fp64_and_deterministic(K, case, fmt, scale):
    """per problem against float64: 2e-6 of the reference's maximum (the bound of test_wgrad3x3_triple_vs_fp64 and of
    test_wgrad3x3_p16_vs_fp64).  Twice: the same bits; rows permuted: the same bits per problem; aliased rows: the same bits."""
    shape, nprob, distinct, expect = case
    N, Cin, Cout, H, W = shape
    planes = _planes(K, shape, distinct, fmt, scale)
    _, refs = _case_refs(shape, distinct)
    reqs = [planes[i % distinct] for i in range(nprob)]
    _assert_plan(K, reqs, expect)
    seq = ('test3x3', shape, nprob, fmt)
    out = K.wgrad3x3_p16_group(reqs, seq=seq)
    again = K.wgrad3x3_p16_group(reqs, seq=seq)
    perm = torch.randperm(nprob, generator=torch.Generator().manual_seed(3)).tolist()
    shuffled = K.wgrad3x3_p16_group([reqs[j] for j in perm], seq=seq)
    torch.cuda.synchronize()
    for i in range(nprob):
        assert torch.equal(out[i][0], again[i][0]) and torch.equal(out[i][1], again[i][1]), i
    for pos, j in enumerate(perm):
        assert torch.equal(out[j][0], shuffled[pos][0]) and torch.equal(out[j][1], shuffled[pos][1]), (pos, j)
    for i in range(distinct, nprob):
        assert torch.equal(out[i][0], out[i % distinct][0]) and torch.equal(out[i][1], out[i % distinct][1]), i
    for i in range(distinct):
        ref, rb = refs[i]
        g, db = out[i]
        assert g.shape == (1, Cout, Cin, 3, 3) and db.shape == (Cout,)
        eg = (g[0].double().cpu() - ref * scale).abs().max().item() / (ref.abs().max().item() * scale)
        eb = (db.double().cpu() - rb * scale).abs().max().item() / (rb.abs().max().item() * scale)
        print(f'wgrad3x3_p16_group {shape} x{nprob} {fmt} scale {scale}: problem {i} g {eg:.2e} db {eb:.2e}')
        assert eg < 2e-6, (i, eg)
        assert eb < 2e-6, (i, eb)


@pytest.mark.gpu
def test_group_without_bias_gradient(K):
    shape, nprob, distinct, expect = CASES[0]
    reqs = _planes(K, shape, distinct, 'bx3', 1.0)
    full = K.wgrad3x3_p16_group(reqs, seq=('test3x3', 'nodb', 1))
    nodb = K.wgrad3x3_p16_group(reqs, seq=('test3x3', 'nodb', 0), want_db=False)
    for (g, _), (g2, db2) in zip(full, nodb):
        assert db2 is None and torch.equal(g, g2)


def _encoder_step(K, E, P, x, dfe, cnt):
    feats, saved = E.encoder_fwd(x, P, 'masa_enc.', [cnt, cnt, cnt], levels=3)
    G = {}
    E.encoder_bwd([d.clone() for d in dfe], P, 'masa_enc.', [cnt, cnt, cnt], saved, G)
    return feats, G


@pytest.fixture
def encoder(K, monkeypatch):
    """the small encoder of test_encoder_on_triples_equals_the_fp32_tensor_path: nf 32, 2 blocks per level, 2 x 48 x 64, on planes at
    every level"""
    from textualdegremoval_amd import engine as E
    monkeypatch.setattr(E, 'P16_ON', True)
    monkeypatch.setattr(E, 'P16_MIN_C', 32)
    nf, cnt = 32, 2
    P = {k: v.cuda().contiguous() for k, v in _encoder_params(nf, cnt).items()}
    x = rnd(2, 3, 48, 64, seed=11)
    dfe = [rnd(2, nf * 2 ** l, 48 >> l, 64 >> l, seed=20 + l, scale=1e-7) for l in range(3)]
    return E, P, x, dfe, cnt


@pytest.mark.gpu
def test_encoder_level_grouped_equals_per_problem_launches(K, encoder, monkeypatch):
    E, P, x, dfe, cnt = encoder
    calls = []
    orig = K.wgrad3x3_p16_group
    monkeypatch.setattr(K, 'wgrad3x3_p16_group', lambda reqs, seq, want_db=True: (calls.append(len(reqs)), orig(reqs, seq, want_db))[1])
    res = {}
    for mode in (True, False):
        monkeypatch.setattr(E, 'GROUP_LEAVES', mode)
        _, G = _encoder_step(K, E, P, x, dfe, cnt)
        torch.cuda.synchronize()
        res[mode] = G
    assert calls == [2 * cnt] * 3                       # one grouped launch per level, none with GROUP_LEAVES off
    assert list(res[True].keys()) == list(res[False].keys())
    assert set(res[True].keys()) == set(P.keys())
    worst = 0.0
    for k, g in res[False].items():
        assert res[True][k].shape == g.shape, k
        worst = max(worst, (res[True][k] - g).abs().max().item() / g.abs().max().item())
    print('encoder grouped vs per-problem launches: worst', worst)
    assert worst < 2e-5, worst


@pytest.mark.gpu
def test_encoder_grouped_under_graph_replay(K, encoder):
    """the pinned pointer tables: a captured encoder step, replayed on new values in the captured buffers, equals eager steps bit for bit"""
    E, P, x, dfe, cnt = encoder
    assert E.GROUP_LEAVES
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _encoder_step(K, E, P, x, dfe, cnt)             # eager first: the call sites get their pinned tables
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph, refs = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph, capture_error_mode='thread_local'), K.workspace_capture(refs):
        feats_g, G_g = _encoder_step(K, E, P, x, dfe, cnt)
    for r in range(2):
        x.copy_(rnd(2, 3, 48, 64, seed=40 + r))
        for l, d in enumerate(dfe):
            d.copy_(rnd(*d.shape, seed=50 + 10 * r + l, scale=1e-7))
        graph.replay()
        torch.cuda.synchronize()
        got_f = [f.clone() for f in feats_g]
        got = {k: v.clone() for k, v in G_g.items()}
        feats, G = _encoder_step(K, E, P, x, dfe, cnt)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got_f, feats))
        assert list(got.keys()) == list(G.keys())
        for k in G:
            assert torch.equal(got[k], G[k]), (r, k)
