"""Every instantiation of the text-embedding projection kernels (csrc/tdr_dynfusion.hip: kvproj_fwd_kernel, kvproj_wgrad_kernel,
kvproj_dkv_part_kernel, built for NB = 1, 2, 4, 8, 16 and chosen by the batch size) against float64 matmuls on the CPU:
    out[:, col0:col0 + rows] = kv W^T,    dW = dk_seg^T kv,    dkv = sum_seg dk_seg W
through kernels.kvproj_fwd / kvproj_wgrad / kvproj_dkv with a segment table {W.data_ptr(), col0, rows, tile0} built here the way
dynfusion_engine.ProjTable builds it.  N = 1 -> NB 1; 2 -> 2; 3, 4 -> 4; 5, 8 -> 8; 9, 16 -> 16: every NB with N == NB and (from 4 on) N < NB.
Segments of 16, 12, 8, 20 and 4 rows: last tiles of 4 rows (nr < the tile height) and a segment smaller than one tile.  dk is a column
slice of a wider tensor, so its row stride is not its width.  The weight gradients are written into one buffer with sentinel rows
between the segments: a tile that writes past its segment's last row is seen.
Bars: weight gradient 1e-5 of the tensor's maximum (a sum of at most 16 terms; the bar of test_hip_dynfusion.py::test_golden).  Forward and
dkv: 8 x the deviation of a float32 CPU matmul of the same operands from the float64 one, relative to the tensor's maximum, never looser than
1e-4.  Measured errors and bars are printed and persisted as kvproj.json beside the other tests' margins
(test_hip_full_size._record_margin).  Every call is repeated and must return the same bits (fixed reduction order)."""
import pytest
import torch

from test_hip_full_size import _record_margin

pytestmark = pytest.mark.gpu
ROWS = [16, 12, 8, 20, 4]
SENTINEL = -12345.0
_margins = {}


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    return kernels


def record(name, line):
    print(line)
    _margins[name] = line
    _record_margin('kvproj', [_margins[k] for k in sorted(_margins)])


class Table:
    def __init__(self, K, rows, Kd, gen):
        self.R = K._lib.load().tdr_kvproj_tile_rows()
        self.rows, self.Kd = rows, Kd
        self.W = [torch.randn(r, Kd, generator=gen) / Kd ** 0.5 for r in rows]
        self.Wd = [w.cuda() for w in self.W]
        tab, self.col0 = [], []
        col = tile = 0
        for w, r in zip(self.Wd, rows):
            tab.append((w.data_ptr(), col, r, tile))
            self.col0.append(col)
            col += r
            tile += -(-r // self.R)
        self.ld, self.ntiles, self.nseg = col, tile, len(rows)
        self.tab = torch.tensor(tab, dtype=torch.int64).cuda()
        self.Wcat = torch.cat(self.W)                        # [ld, Kd]: the columns of the output in table order

    def grad_buffer(self):
        """one flat buffer: each segment's [rows, Kd] gradient followed by R sentinel rows -> (buffer, gtable, row offsets)"""
        offs, o = [], 0
        for r in self.rows:
            offs.append(o)
            o += r + self.R
        buf = torch.full((o, self.Kd), SENTINEL, dtype=torch.float32, device='cuda')
        gtab = torch.tensor([buf[o].data_ptr() for o in offs], dtype=torch.int64).cuda()
        return buf, gtab, offs


def strided_dk(N, ld, gen):
    """dk [N, ld] as a column slice of a wider [N, ld + 7] tensor: row stride ld + 7, first column 3"""
    wide = torch.randn(N, ld + 7, generator=gen)
    dk = wide.cuda()[:, 3:3 + ld]
    assert dk.stride(0) == ld + 7 and dk.stride(1) == 1
    return wide[:, 3:3 + ld], dk


def rel(a, ref):
    a, ref = a.detach().cpu().double(), ref.double()
    return ((a - ref).abs().max() / ref.abs().max()).item()


def matmul_bar(a, b, ref):
    """(deviation of the float32 CPU matmul a @ b from the float64 result relative to its maximum, bar = 8 x that, at most 1e-4)"""
    dev = rel(a @ b, ref)
    return dev, min(8 * dev, 1e-4)


def run_all(K, t, N, gen, tag):
    """forward, weight gradient and dkv of table t at batch size N against float64; each call twice, bit-identical"""
    Kd = t.Kd
    kv = torch.randn(N, Kd, generator=gen)
    kvd = kv.cuda()
    dk, dkd = strided_dk(N, t.ld, gen)

    out = K.kvproj_fwd(t.tab, t.nseg, t.ntiles, kvd, t.ld)
    assert out.shape == (N, t.ld)
    assert torch.equal(out, K.kvproj_fwd(t.tab, t.nseg, t.ntiles, kvd, t.ld))
    ref = kv.double() @ t.Wcat.double().t()
    dev_f, bar_f = matmul_bar(kv, t.Wcat.t(), ref)
    e_f = rel(out, ref)

    buf, gtab, offs = t.grad_buffer()
    K.kvproj_wgrad(t.tab, gtab, t.nseg, t.ntiles, kvd, dkd)
    buf2, gtab2, _ = t.grad_buffer()
    K.kvproj_wgrad(t.tab, gtab2, t.nseg, t.ntiles, kvd, dkd)
    assert torch.equal(buf, buf2)
    buf = buf.cpu()
    e_w = 0.0
    for o, r, c0 in zip(offs, t.rows, t.col0):
        assert (buf[o + r:o + r + t.R] == SENTINEL).all(), 'a tile wrote past the last row of its segment'
        e_w = max(e_w, rel(buf[o:o + r], dk[:, c0:c0 + r].double().t() @ kv.double()))

    dkv = K.kvproj_dkv(t.tab, t.nseg, t.ntiles, dkd, Kd)
    assert dkv.shape == (N, Kd)
    assert torch.equal(dkv, K.kvproj_dkv(t.tab, t.nseg, t.ntiles, dkd, Kd))
    ref = dk.double() @ t.Wcat.double()
    dev_d, bar_d = matmul_bar(dk.contiguous(), t.Wcat, ref)
    e_d = rel(dkv, ref)
    record(tag, f'{tag}: forward {e_f:.3e} (float32 matmul {dev_f:.3e}, bar {bar_f:.3e}); weight gradient {e_w:.3e} (bar 1e-05); '
                f'dkv {e_d:.3e} (float32 matmul {dev_d:.3e}, bar {bar_d:.3e})')
    assert e_f <= bar_f
    assert e_w <= 1e-5
    assert e_d <= bar_d


@pytest.mark.parametrize('N', [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize('Kd', [1024, 2048])
def test_every_batch_instantiation_vs_float64(K, Kd, N):
    gen = torch.Generator().manual_seed(1000 * N + Kd)
    t = Table(K, ROWS, Kd, gen)
    assert t.R == 8 and t.ntiles == 9 and t.ld == 60         # two last tiles of 4 rows (12, 20), one segment below a tile (4)
    run_all(K, t, N, gen, f'rows {ROWS} K {Kd} N {N}')


def test_more_tiles_than_dkv_row_groups(K):
    """50 segments of 40 rows: 250 tiles > the 192 row groups of kvproj_dkv's first stage -> 2 tiles per workgroup, 125 of 192 groups used"""
    lib = K._lib.load()
    gen = torch.Generator().manual_seed(50)
    t = Table(K, [40] * 50, 1024, gen)
    assert t.ntiles == 250 and lib.tdr_kvproj_dkv_parts(t.ntiles) == 192
    run_all(K, t, 5, gen, 'rows 50 x 40 K 1024 N 5')


def test_dkv_column_tail(K):
    """K = 1284: a multiple of 4 but not of 1024 -- the last column block of kvproj_dkv is partly outside the matrix"""
    gen = torch.Generator().manual_seed(1284)
    Kd, N = 1284, 3
    t = Table(K, ROWS, Kd, gen)
    dk, dkd = strided_dk(N, t.ld, gen)
    dkv = K.kvproj_dkv(t.tab, t.nseg, t.ntiles, dkd, Kd)
    assert dkv.shape == (N, Kd)
    assert torch.equal(dkv, K.kvproj_dkv(t.tab, t.nseg, t.ntiles, dkd, Kd))
    ref = dk.double() @ t.Wcat.double()
    dev, bar = matmul_bar(dk.contiguous(), t.Wcat, ref)
    e = rel(dkv, ref)
    record('dkv tail', f'rows {ROWS} K {Kd} N {N}: dkv {e:.3e} (float32 matmul {dev:.3e}, bar {bar:.3e})')
    assert e <= bar


def test_batch_above_16_is_refused(K):
    from textualdegremoval_amd._lib import TdrError
    gen = torch.Generator().manual_seed(17)
    t = Table(K, ROWS, 1024, gen)
    kvd = torch.randn(17, 1024, generator=gen).cuda()
    _, dkd = strided_dk(17, t.ld, gen)
    _, gtab, _ = t.grad_buffer()
    with pytest.raises(TdrError):
        K.kvproj_fwd(t.tab, t.nseg, t.ntiles, kvd, t.ld)
    with pytest.raises(TdrError):
        K.kvproj_wgrad(t.tab, gtab, t.nseg, t.ntiles, kvd, dkd)
    with pytest.raises(TdrError):
        K.kvproj_dkv(t.tab, t.nseg, t.ntiles, dkd, 1024)
