"""The float64 reference that tests/test_hip_attention_cores.py holds the channel-attention kernels to (tests/_attn_core_ref.py), checked on
the CPU against the formulation the model code uses -- F.normalize -> q k^T * temperature -> topk / scatter mask -> softmax -> weighted sum,
written as in oracle/restormer_ref_oracle.mdta and oracle/drsformer_ref_oracle.tksa -- and the W / dtemp / dam mapping against that
formulation's autograd: d[q;k] = W [q;k].  Also the place where the near-tie cap of the chosen seeds is asserted without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import _attn_core_ref as AR


def model_attention(q, k, temp, am, kind):
    """q, k [N, heads, c, HW] -> the c x c attention matrix per head that multiplies v (TKSA: the four branches multiply the same v, so
    sum_m (a_m @ v) attn_m = (sum_m attn_m a_m) @ v)"""
    ch = q.shape[2]
    qn = F.normalize(q, dim=-1)
    kn = F.normalize(k, dim=-1)
    attn = (qn @ kn.transpose(-2, -1)) * temp
    if kind == 'mdta':
        return attn.softmax(dim=-1)
    out = 0
    for m, kk in enumerate((int(ch / 2), int(ch * 2 / 3), int(ch * 3 / 4), int(ch * 4 / 5))):
        idx = torch.topk(attn, k=kk, dim=-1, largest=True)[1]
        mask = torch.zeros_like(attn).scatter_(-1, idx, 1.0)
        a = torch.where(mask > 0, attn, torch.full_like(attn, float('-inf'))).softmax(dim=-1)
        out = out + a * am[m]
    return out


@pytest.mark.parametrize('kind', ['mdta', 'tksa'])
@pytest.mark.parametrize('C,heads', [(16, 2), (160, 2)])
def test_reference_is_the_model_formulation(C, heads, kind):
    """forward to 1e-12 absolute; d[q;k] = W [q;k], dtemp and dam against the model formulation's autograd to 1e-10 of each tensor's maximum.
    Everything in float64, G and ss formed in float64 from the same q, k (the helper is handed them as they are)."""
    HW, N = (96, 2) if C == 16 else (64, 2)
    inp = AR.make_inputs(C, heads, HW, N, seed=C + heads)
    c = inp['c']
    q = inp['q'].double().requires_grad_(True)
    k = inp['k'].double().requires_grad_(True)
    temp = inp['temp'].double().requires_grad_(True)
    am = inp['am'].double().requires_grad_(True)
    dAb = AR.blocks(inp['dA'].double(), heads)
    attn = model_attention(q, k, temp, am, kind)
    (attn * dAb).sum().backward()

    G64 = inp['G'].double()                  # keeps the random off-head blocks
    Gb = q.detach() @ k.detach().transpose(-2, -1)
    for h in range(heads):
        G64[:, h * c:(h + 1) * c, h * c:(h + 1) * c] = Gb[:, h]
    ss64 = torch.cat([(q.detach() ** 2).sum(-1).reshape(N, C), (k.detach() ** 2).sum(-1).reshape(N, C)], dim=1)
    ref = AR.reference(dict(inp, G=G64, ss=ss64), kind)
    assert not ref['bad'].any()              # no near tie at these seeds: both formulations select the same entries

    assert (AR.blocks(ref['A'][:, :C, :C], heads) - attn.detach()).abs().max().item() < 1e-12
    assert (ref['A'][:, ~AR.structure_A(C, heads)] == 0).all()
    qk = torch.cat([q.detach().reshape(N, C, HW), k.detach().reshape(N, C, HW)], dim=1)
    d = ref['W'][:, :2 * C, :2 * C] @ qk
    want = torch.cat([q.grad.reshape(N, C, HW), k.grad.reshape(N, C, HW)], dim=1)
    assert AR.rel_dev(d, want) < 1e-10
    assert (ref['W'][:, ~AR.structure_W(C, heads)] == 0).all()
    assert AR.rel_dev(ref['dtemp'], temp.grad) < 1e-10
    if kind == 'tksa':
        assert AR.rel_dev(ref['dam'], am.grad) < 1e-10


def test_topk_sizes_are_the_model_literals():
    for c in (6, 8, 12, 48, 80, 96, 176, 192):
        assert AR.tksa_ks(c) == [int(c / 2), int(c * 2 / 3), int(c * 3 / 4), int(c * 4 / 5)]
        assert all(1 <= k < c for k in AR.tksa_ks(c))


@pytest.mark.parametrize('shape', AR.SHAPES, ids=lambda s: 'C%d-h%d-HW%d-N%d' % s)
def test_near_tie_cap_of_the_chosen_seeds(shape):
    """at most 1 % of a case's rows sit within 2e-6 of a top-k cut in the float64 logits (the counts are those _attn_core_ref.SEEDS was chosen
    for), and the fp32 logits are within 1e-7 of the float64 ones: the 2e-6 gap is 20 x the error that could reorder two entries"""
    C, heads, HW, N = shape
    inp = AR.make_inputs(C, heads, HW, N, AR.SEEDS[shape])
    L = AR.logits(inp['G'].double(), inp['ss'].double(), inp['temp'].double(), heads)
    bad = AR.near_tie_rows(L, AR.tksa_ks(C // heads))
    assert bad.numel() == N * C
    assert int(bad.sum()) <= AR.TIE_CAP * bad.numel()
    assert int(bad.sum()) == AR.LEFT_OUT[shape]
    L32 = AR.logits(inp['G'], inp['ss'], inp['temp'], heads)
    assert (L32.double() - L).abs().max().item() < 1e-7


def test_near_tie_detection_and_lowest_index_rule():
    """a planted pair 1e-7 apart at the first cut is flagged, the same pair 1e-3 apart is not; equal entries are ranked lower index first"""
    c = 8
    ks = AR.tksa_ks(c)                      # 4, 5, 6, 6
    row = torch.tensor([0.8, 0.7, 0.6, 0.5, 0.5 - 1e-7, 0.3, 0.2, 0.1], dtype=torch.float64)
    assert AR.near_tie_rows(row.view(1, 1, 1, c), ks).item()
    row[4] = 0.5 - 1e-3
    assert not AR.near_tie_rows(row.view(1, 1, 1, c), ks).item()
    tie = torch.tensor([0.1, 0.5, 0.9, 0.5, 0.5, 0.2, 0.9, 0.0], dtype=torch.float64)
    assert AR.ranks(tie.view(1, 1, 1, c)).flatten().tolist() == [6, 2, 0, 3, 4, 5, 1, 7]


def test_float32_evaluation_leaves_the_inputs_alone():
    """the float32 evaluation (the yardstick of the backward bars) casts nothing, so it must not turn the shared inputs into autograd leaves:
    a second evaluation returns the same bits instead of accumulated gradients"""
    inp = AR.make_inputs(16, 2, 96, 2, seed=18)
    ref = AR.reference(inp, 'tksa')
    a = AR.reference(inp, 'tksa', torch.float32, masks=ref['masks'])
    b = AR.reference(inp, 'tksa', torch.float32, masks=ref['masks'])
    assert not any(inp[k].requires_grad for k in ('G', 'ss', 'temp', 'am'))
    assert all(torch.equal(a[k], b[k]) for k in ('A', 'W', 'dtemp', 'dam'))
    bars = AR.backward_bars(inp, 'tksa', ref)
    assert all(0 < dev < 2e-6 and bar == min(8 * dev, 1e-4) for dev, bar in bars.values())


def test_dead_channel_reference_is_finite():
    """a zero q row and a zero k row: uniform softmax row, zero diagonal gradient, nothing NaN (the clamp is a torch.where on ss)"""
    C, heads, HW, N = 80, 1, 64, 2
    inp = AR.make_inputs(C, heads, HW, N, seed=81, dead=(0, 70, 3))
    ref = AR.reference(inp, 'mdta')
    assert all(torch.isfinite(ref[n]).all() for n in ('A', 'W', 'dtemp'))
    assert (ref['A'][:, 70, :C] - 1.0 / C).abs().max().item() < 1e-15
    assert (ref['W'][:, 70, 70] == 0).all() and (ref['W'][:, C + 3, C + 3] == 0).all()
    # the float32 evaluation that sets the backward bars stays finite and close where both norms are clamped (W there is ~1e24 times the rest)
    r32 = AR.reference(inp, 'mdta', torch.float32)
    assert all(torch.isfinite(r32[n]).all() for n in ('A', 'W', 'dtemp'))
    assert abs(r32['W'][0, 70, C + 3].item() / ref['W'][0, 70, C + 3].item() - 1) < 1e-5 and AR.rel_dev(r32['dtemp'], ref['dtemp']) < 1e-5
