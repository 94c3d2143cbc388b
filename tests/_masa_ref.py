"""Float64 reference of the MASA match-and-transfer kernels (csrc/tdr_masa.hip), composed from the functions of
oracle/nafnet_ref_oracle.py (they run unchanged in float64 and under autograd), and the seeded input builders of
tests/test_hip_masa_kernels.py.  Torch on the CPU only; nothing here imports the GPU package.

Every reference function takes a dtype: called with float64 on the float32 inputs cast up it is the reference, called with
float32 it is the yardstick -- e32 = max |f32 run - f64 run| is what fp32 arithmetic in the reference's own summation order
leaves, and a kernel is held to bar(e32, ref64) = max(8 e32, 4 float32 ulp of max |ref64|) (another order over the same number
of terms: merged multiplicities, atomics in arrival order, per-chunk partials)."""
import torch
import torch.nn.functional as F

from oracle import nafnet_ref_oracle as O

ULP32 = 2.0 ** -23


def maxabs(a, b):
    return (a.detach().double() - b.detach().double()).abs().max().item()


def floor_bar(ref64):
    return 4 * ULP32 * ref64.detach().double().abs().max().item()


def bar(e32, ref64):
    return max(8 * e32, floor_bar(ref64))


# ---------------------------------------------------------------------------------------------------------- references
def transfer_ref(feat, y1, x1, index_all, soft_att, py, px, K, side, s, dout, dtype):
    """feat [N, C, Hdeep*s, Wdeep*s]; y1, x1 [N, py*px] (long); index_all (long), soft_att [N*py*px, K*K]; dout [N, C, py*K*s,
    px*K*s].  Returns out, dfeat, datt of gather_ref_block -> transfer -> the re-tiling of masa_match_and_transfer."""
    N, C = feat.shape[:2]
    B = N * py * px
    f = feat.to(dtype).clone().requires_grad_(True)
    a = soft_att.to(dtype).clone().requires_grad_(True)
    blk = O.gather_ref_block(f, y1, x1, side, s)
    t = O.transfer(blk, index_all.view(B, K, K), a.view(B, 1, K, K), s, side - 2)
    out = t.view(N, py, px, C, K * s, K * s).permute(0, 3, 1, 4, 2, 5).reshape(N, C, py * K * s, px * K * s)
    out.backward(dout.to(dtype))
    return out.detach(), f.grad, a.grad.view(B, K * K)


def fine_bwd_ref(lrb, refb, index_all, datt, dtype):
    """lrb [B, C, K+2, K+2], refb [B, C, D, D], index_all (long), datt [B, K*K].  The cosine similarity of O.fine_search taken at
    the GIVEN index (gather, not max: near-ties cannot matter).  Returns att [B, K*K], invq [B, K*K], invk [B, (D-2)^2] (the
    reciprocal norms with the 1e-12 clamp), dlrb, drefb."""
    B = lrb.shape[0]
    lr = lrb.to(dtype).clone().requires_grad_(True)
    rf = refb.to(dtype).clone().requires_grad_(True)
    q = F.unfold(lr, 3).transpose(1, 2)              # [B, K*K, C*9]
    k = F.unfold(rf, 3)                              # [B, C*9, (D-2)^2]
    corr = torch.bmm(O._l2n(q, 2), O._l2n(k, 1))
    att = corr.gather(2, index_all.view(B, -1, 1)).squeeze(2)
    att.backward(datt.to(dtype).view(B, -1))
    invq = 1.0 / q.detach().norm(dim=2).clamp_min(1e-12)
    invk = 1.0 / k.detach().norm(dim=1).clamp_min(1e-12)
    return att.detach(), invq, invk, lr.grad, rf.grad


def argmax_products(dots, invq, invk, dtype=torch.float64):
    """the values the arg-max kernels compare.  Fine layout: dots [B, P, R], invq [B, P], invk [B, R].  Coarse layout: dots [ND,
    N, P, R], invq [ND, N, P], invk [ND, N, R], summed over the ND dilations in order."""
    d, iq, ik = dots.to(dtype), invq.to(dtype), invk.to(dtype)
    if d.dim() == 3:
        return d * iq.unsqueeze(2) * ik.unsqueeze(1)
    v = 0
    for n in range(d.shape[0]):
        v = v + d[n] * iq[n].unsqueeze(2) * ik[n].unsqueeze(1)
    return v


def argmax_ref(dots, invq, invk):
    """index (first one on exact ties) and value in float64, both layouts of argmax_products"""
    v = argmax_products(dots, invq, invk)
    R = v.shape[-1]
    val = v.max(dim=-1).values
    cols = torch.arange(R).expand_as(v)
    idx = torch.where(v == val.unsqueeze(-1), cols, torch.full_like(cols, R)).min(dim=-1).values
    return idx, val


def coarse_products(lrb, ref, dilations, dtype=torch.float64):
    """the un-normalised correlations and reciprocal norms of O.coarse_search: dots [ND, N, P, R], invq [ND, N, P], invk [ND, N, R]"""
    N, Pn, C, Kh, Kw = lrb.shape
    Hr, Wr = ref.shape[-2:]
    lrb, ref = lrb.to(dtype), ref.to(dtype)
    cy, cx = Kh // 2, Kw // 2
    dots, invq, invk = [], [], []
    for d in dilations:
        q = lrb[:, :, :, [cy - d, cy, cy + d]][:, :, :, :, [cx - d, cx, cx + d]].reshape(N, Pn, C * 9)
        rp = F.pad(ref, (d, d, d, d))
        taps = [rp[:, :, ky * d: ky * d + Hr, kx * d: kx * d + Wr] for ky in range(3) for kx in range(3)]
        k = torch.stack(taps, dim=2).reshape(N, C * 9, Hr * Wr)
        dots.append(torch.bmm(q, k))
        invq.append(1.0 / q.norm(dim=2).clamp_min(1e-12))
        invk.append(1.0 / k.norm(dim=1).clamp_min(1e-12))
    return torch.stack(dots), torch.stack(invq), torch.stack(invk)


def gather_ref(feat, y1, x1, side, s, dblk, dtype):
    """O.gather_ref_block and its adjoint: returns blk [N*P, C, side*s, side*s] and dfeat"""
    f = feat.to(dtype).clone().requires_grad_(True)
    blk = O.gather_ref_block(f, y1, x1, side, s)
    blk.backward(dblk.to(dtype))
    return blk.detach(), f.grad


# ------------------------------------------------------------------------------------------------------ input builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


INDEX_PATTERNS = ('random', 'coherent', 'constant', 'corners')


def index_pattern(kind, B, K, R1, seed):
    """index_all [B, K*K] (long) into the R1 x R1 grid of ref patches.
    random:   uniform.
    coherent: idx(i, j) = (r0 + i) R1 + c0 + j -- every covering patch of a pixel names the same source, the multiplicity path
              carries the whole sum (needs K <= R1).
    constant: one index per block, the most collisions per address in the scatter.
    corners:  only 0, R1-1, R1 (R1-1), R1 R1 - 1."""
    g = _gen(seed)
    if kind == 'random':
        return torch.randint(0, R1 * R1, (B, K * K), generator=g)
    if kind == 'coherent':
        assert K <= R1, 'coherent matches need K <= R1: use constant'
        r0 = torch.randint(0, R1 - K + 1, (B, 1, 1), generator=g)
        c0 = torch.randint(0, R1 - K + 1, (B, 1, 1), generator=g)
        i = torch.arange(K).view(1, K, 1)
        j = torch.arange(K).view(1, 1, K)
        return ((r0 + i) * R1 + c0 + j).reshape(B, K * K)
    if kind == 'constant':
        return torch.randint(0, R1 * R1, (B, 1), generator=g).expand(B, K * K).contiguous()
    if kind == 'corners':
        c = torch.tensor([0, R1 - 1, R1 * (R1 - 1), R1 * R1 - 1])
        return c[torch.randint(0, 4, (B, K * K), generator=g)]
    raise ValueError(kind)


def boxes(N, P, Hdeep, Wdeep, side):
    """block starts y1, x1 [N, P] (long): centres on the four borders and in the interior put through O.box_start (the list is
    rotated per image); with P >= 2 the last block of every image repeats the box of its first block, so contributions collide
    across blocks."""
    dia = side - 2
    H, W = Hdeep, Wdeep
    centres = [(0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2), (0, 0), (H - 1, W - 1)]
    cy = torch.empty(N, P, dtype=torch.long)
    cx = torch.empty(N, P, dtype=torch.long)
    for n in range(N):
        for p in range(P):
            c = centres[(n * 3 + p) % len(centres)] if (p < P - 1 or P == 1) else centres[(n * 3) % len(centres)]
            cy[n, p], cx[n, p] = c
    return O.box_start(cy, H, dia), O.box_start(cx, W, dia)


# transfer geometries (N, C, py, px, K, side, Hdeep, Wdeep)
TRANSFER_GEOM = {
    'A': (2, 9, 2, 3, 8, 15, 12, 17),      # negative y1 (12 < 15), non-square ref, six blocks per image, C % 8 = 1
    'B': (1, 44, 1, 2, 8, 15, 20, 20),     # five channel chunks of the backward, the last one ragged (cpb = 9)
    'C': (2, 16, 1, 1, 12, 21, 24, 24),    # K = 12
    'D': (1, 8, 2, 2, 8, 9, 10, 10),       # R1 = 7 < K
}
# (geometry, s, index pattern): every (geometry, s) runs 'random' and one other pattern, A at s = 2 all four
TRANSFER_CASES = [
    ('A', 1, 'random'), ('A', 1, 'coherent'),
    ('A', 2, 'random'), ('A', 2, 'coherent'), ('A', 2, 'constant'), ('A', 2, 'corners'),
    ('A', 4, 'random'), ('A', 4, 'constant'),
    ('A', 8, 'random'), ('A', 8, 'corners'),
    ('A', 16, 'random'), ('A', 16, 'coherent'),
    ('B', 1, 'random'), ('B', 1, 'constant'),
    ('B', 2, 'random'), ('B', 2, 'coherent'),
    ('C', 1, 'random'), ('C', 1, 'corners'),
    ('C', 4, 'random'), ('C', 4, 'coherent'),
    ('D', 1, 'random'), ('D', 1, 'constant'),
    ('D', 2, 'random'), ('D', 2, 'corners'),
]


def case_seed(*key):
    """a fixed seed per case (no hash(): it is salted per process)"""
    h = 17
    for ch in repr(key):
        h = (h * 131 + ord(ch)) % 1000003
    return h


def transfer_inputs(geom, s, pattern):
    N, C, py, px, K, side, Hd, Wd = TRANSFER_GEOM[geom]
    P, B = py * px, N * py * px
    seed = case_seed(geom, s, pattern)
    g = _gen(seed)
    y1, x1 = boxes(N, P, Hd, Wd, side)
    return dict(N=N, C=C, py=py, px=px, K=K, side=side, s=s, Hdeep=Hd, Wdeep=Wd, y1=y1, x1=x1,
                feat=torch.randn(N, C, Hd * s, Wd * s, generator=g),
                dout=torch.randn(N, C, py * K * s, px * K * s, generator=g),
                soft_att=torch.rand(B, K * K, generator=g) * 0.8 + 0.2,
                index_all=index_pattern(pattern, B, K, side - 2, seed + 1),
                dfeat_pre=torch.randn(N, C, Hd * s, Wd * s, generator=g),
                datt_pre=torch.randn(B, K * K, generator=g))


def transfer_reference(inp):
    """float64 reference and float32 yardstick of one transfer case: out, and dfeat / datt AFTER the += into the pre-filled buffers"""
    args = [inp[k] for k in ('feat', 'y1', 'x1', 'index_all', 'soft_att', 'py', 'px', 'K', 'side', 's', 'dout')]
    r = {}
    for name, dt in (('64', torch.float64), ('32', torch.float32)):
        out, dfeat, datt = transfer_ref(*args, dt)
        r[name] = dict(out=out, dfeat=inp['dfeat_pre'].to(dt) + dfeat, datt=inp['datt_pre'].to(dt) + datt)
    ref = r['64']
    ref['e32'] = {k: maxabs(r['32'][k], ref[k]) for k in ('out', 'dfeat', 'datt')}
    return ref


FINE_BWD_CASES = [(6, 8, 8, 15), (3, 70, 8, 15), (2, 16, 12, 21), (4, 8, 8, 9)]       # (B, C, K, D)
FINE_BWD_PATTERNS = ('random', 'constant', 'corners')


def fine_bwd_inputs(B, C, K, D, pattern):
    seed = case_seed('fine', B, C, K, D, pattern)
    g = _gen(seed)
    return dict(lrb=torch.randn(B, C, K + 2, K + 2, generator=g), refb=torch.randn(B, C, D, D, generator=g),
                datt=torch.randn(B, K * K, generator=g), index_all=index_pattern(pattern, B, K, D - 2, seed + 1))


PLANT = 1.5           # a planted winner's product is PLANT x the largest magnitude of its row
PLANT_MARGIN = 1.4    # ... so it exceeds every other product's magnitude by at least this factor (float32 rounding of dots included)


def _plant_columns(R):
    return [0, R - 1, 64 + (R - 64) // 2 if R > 64 else R // 2]


def fine_argmax_inputs(B, P, R):
    """ordinary rows: standard-normal dots, reciprocal norms in [0.5, 1.5], a winner planted at the first column, the last column
    and a column >= 64 (R // 2 where R <= 64) in turn.  Returns dots [B, P, R], invq [B, P], invk [B, R], planted columns [B, P]."""
    g = _gen(case_seed('fargmax', B, P, R))
    dots = torch.randn(B, P, R, generator=g)
    invq = torch.rand(B, P, generator=g) + 0.5
    invk = torch.rand(B, R, generator=g) + 0.5
    cols = torch.tensor(_plant_columns(R))[torch.arange(B * P) % 3].view(B, P)
    v = argmax_products(dots, invq, invk)
    top = v.abs().max(dim=2).values
    want = PLANT * top / (invq.double() * invk.double().gather(1, cols))
    dots.scatter_(2, cols.unsqueeze(2), want.float().unsqueeze(2))
    return dots, invq, invk, cols


def _tie_columns(row, R):
    """columns that share the maximum: the same lane in different strides (c, c + 64, ...), lanes at several shuffle distances,
    and the last column"""
    sets = [[5, 69, 133, 261], [9, 10, 41], [R - 1, 3, 35], [70, 7, 71], [2, 258, 130]]
    cols = sorted({c for c in sets[row % len(sets)] if c < R})
    return cols if len(cols) >= 2 else [R // 2, R - 1]


def fine_argmax_tie_inputs(B, P, R):
    """exact rows: invq = invk = 1 and integer dots in [-3, 3], the maximum 5 repeated at _tie_columns"""
    g = _gen(case_seed('ftie', B, P, R))
    dots = torch.randint(-3, 4, (B, P, R), generator=g).float()
    first = torch.empty(B, P, dtype=torch.long)
    for r in range(B * P):
        cols = _tie_columns(r, R)
        dots.view(B * P, R)[r, cols] = 5.0
        first.view(-1)[r] = cols[0]
    return dots, torch.ones(B, P), torch.ones(B, R), first


COARSE_MAPS = [(12, 12), (20, 31), (9, 40)]
COARSE_ND, COARSE_N, COARSE_P = 3, 2, 5


def _coarse_positions(Hr, Wr):
    ym, xm = Hr // 2, Wr // 2
    pos = [(0, 0), (0, Wr - 1), (Hr - 1, 0), (Hr - 1, Wr - 1), (0, xm), (Hr - 1, xm), (ym, 0), (ym, Wr - 1), (ym, xm), (ym - 2, xm + 3)]
    return torch.tensor([y * Wr + x for y, x in pos])


def coarse_argmax_inputs(Hr, Wr):
    """dots [ND, N, P, R], invq [ND, N, P], invk [ND, N, R]; the ten rows have winners planted at the four corners, on each edge and at
    two interior positions (each dilation carries a third of the planted sum)"""
    ND, N, P, R = COARSE_ND, COARSE_N, COARSE_P, Hr * Wr
    g = _gen(case_seed('cargmax', Hr, Wr))
    dots = torch.randn(ND, N, P, R, generator=g)
    invq = torch.rand(ND, N, P, generator=g) + 0.5
    invk = torch.rand(ND, N, R, generator=g) + 0.5
    cols = _coarse_positions(Hr, Wr).view(N, P)
    top = argmax_products(dots, invq, invk).abs().max(dim=2).values
    for d in range(ND):
        want = PLANT * top / ND / (invq[d].double() * invk[d].double().gather(1, cols))
        dots[d].scatter_(2, cols.unsqueeze(2), want.float().unsqueeze(2))
    return dots, invq, invk, cols


def coarse_argmax_tie_inputs(Hr, Wr):
    """exact rows: all reciprocal norms 1, integer dots in [-3, 3] per dilation, the summed maximum 15 repeated at _tie_columns
    (c and c + 256 meet in one thread of the 256-wide block where R > 256)"""
    ND, N, P, R = COARSE_ND, COARSE_N, COARSE_P, Hr * Wr
    g = _gen(case_seed('ctie', Hr, Wr))
    dots = torch.randint(-3, 4, (ND, N, P, R), generator=g).float()
    first = torch.empty(N, P, dtype=torch.long)
    for r in range(N * P):
        cols = _tie_columns(r, R)
        dots.view(ND, N * P, R)[:, r, cols] = 5.0
        first.view(-1)[r] = cols[0]
    return dots, torch.ones(ND, N, P), torch.ones(ND, N, R), first
