"""The grouped router on the GPU.  moe_topk_grouped returns, on request, the scores it selected on; the numpy definition of tests/test_moe_route_grouped_cpu.py
(grouped_topk_ref: float32 s + bias, float32 top-2 sums, stable sorts) applied to THOSE scores must give the kernel's ids exactly, on every row, ties included.
The scores themselves are checked against float64 within derived bounds, the weights bit for bit (plain) or within a derived bound (renormalised).  Then: no effect
from asking for the scores or from the rows' alignment, masked groups, non-finite rows, agreement with moe_topk_softmax where both are defined, moe_route_grouped
(sort results, graph replay) and a whole layer."""
import numpy as np
import pytest
import torch

from test_moe_route_grouped_cpu import grouped_topk_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
SHAPES = [(8, 1), (8, 2), (8, 4), (16, 16), (60, 4), (160, 8), (256, 8), (384, 1), (1024, 64), (1024, 8)]   # (E, n_group)
TOKENS = [1, 3, 5, 67]
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _f64(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().float().numpy().astype(np.float64)   # bf16 -> float32 -> float64: both exact


def _np(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.numpy()


def _topk_groups(G):
    return sorted({1, (G + 1) // 2, G})


def _topks(E, G, tg):
    top = min(32, tg * (E // G))
    return sorted({k for k in (1, 2, 8, top) if k <= top})


def _logits(T, E, dtype, seed):
    """randn * 3, every second row on a grid of quarters (exact ties); when there is room, a row of all-equal logits, a row of +0.0 / -0.0 mixed and a row with
    -inf entries"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T, E, generator=gen) * 3.0
    x[1::2] = torch.round(x[1::2] * 4.0) / 4.0
    if T >= 3:
        x[0] = 1.25
        x[1] = torch.where(torch.rand(E, generator=gen) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        x[2, torch.randperm(E, generator=gen)[: max(E // 3, 1)]] = float("-inf")
    return x.to(dtype)


def _bias(E, seed):
    """a coarse grid (multiples of 1/8 in [-3/8, 3/8]): exact ties in c and in the group scores occur on the all-equal and the quarter-grid rows"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(-3, 4, (E,), generator=gen).float() / 8.0)


# ------------------------------------------------------------------------------------------------
# 1. 3. 4a.  selection is exact on the returned scores; weights; no effect from asking for the scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("scoring", ["sigmoid", "softmax"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E,G", SHAPES)
def test_selection_is_exact_on_the_returned_scores_and_weights_follow(q, E, G, dtype, scoring, with_bias):
    """ids: equal to grouped_topk_ref on the returned scores, every row, no tolerance.  weights, plain: float32(s[ids]) * float32(scale) bit for bit.  Renormalised:
    within (topk + 4) * 2^-24 relative of the float64 quotient of the returned scores times the scale -- at most topk - 1 roundings in the fp32 sum of topk positive
    terms in any order, one in the divide, one in the multiply, two units spare --, and the row sum within 64 * 2^-24 of the scale (relative).  Without
    return_scores: the same bits."""
    scale = 2.5
    bias = _bias(E, E + G) if with_bias else None
    bias_np = None if bias is None else bias.numpy()
    bias_dev = None if bias is None else bias.to(DEV)
    worst = 0.0
    for T in TOKENS:
        x = _logits(T, E, dtype, seed=E * 100 + G * 7 + T).to(DEV)
        for tg in _topk_groups(G):
            for topk in _topks(E, G, tg):
                for renorm in (False, True):
                    kw = dict(n_group=G, topk_group=tg, bias=bias_dev, scoring=scoring, renormalize=renorm, routed_scaling_factor=scale)
                    w, ids, s = q.moe_topk_grouped(x, topk, return_scores=True, **kw)
                    assert w.shape == ids.shape == (T, topk) and s.shape == (T, E) and w.dtype == s.dtype == torch.float32 and ids.dtype == torch.int32
                    w2, ids2 = q.moe_topk_grouped(x, topk, **kw)
                    assert torch.equal(ids, ids2) and torch.equal(w.view(torch.int32), w2.view(torch.int32)), (T, tg, topk, renorm)
                    s_np, ids_np, w_np = s.cpu().numpy(), ids.cpu().numpy(), w.cpu().numpy()
                    assert not np.isnan(s_np).any()
                    want_ids, want_w = grouped_topk_ref(s_np, topk, n_group=G, topk_group=tg, bias=bias_np, renormalize=renorm, routed_scaling_factor=scale)
                    assert np.array_equal(ids_np, want_ids), (T, tg, topk, int((ids_np != want_ids).any(axis=1).sum()), np.argwhere(ids_np != want_ids)[:4].tolist())
                    if not renorm:
                        assert np.array_equal(w_np.view(np.int32), want_w.view(np.int32)), (T, tg, topk)
                    else:
                        ok = np.take_along_axis(s_np, want_ids, axis=1).astype(np.float64).sum(axis=1) > 0     # a row whose selected scores sum to 0: unspecified
                        err = np.abs(w_np[ok] - want_w[ok]) / np.where(want_w[ok] > 0, want_w[ok], 1.0)
                        worst = max(worst, float(err.max() / U) if err.size else 0.0)
                        assert (np.abs(w_np[ok] - want_w[ok]) <= (topk + 4) * U * want_w[ok]).all(), (T, tg, topk, err.max() / U)
                        assert (np.abs(w_np[ok].astype(np.float64).sum(axis=1) - scale) <= 64 * U * scale).all(), (T, tg, topk)
    print(f"E={E} G={G} {dtype} {scoring} bias={with_bias}: renormalised weights, max relative error {worst:.2f} x 2^-24")
    w, ids, s = q.moe_topk_grouped(torch.empty(0, E, dtype=dtype, device=DEV), 1, n_group=G, topk_group=1, return_scores=True)
    assert w.shape == ids.shape == (0, 1) and s.shape == (0, E)


# ------------------------------------------------------------------------------------------------
# 2. the scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,G", SHAPES)
def test_sigmoid_scores_are_within_the_derived_bound_and_do_not_depend_on_the_dtype(q, E, G):
    """|s - s64| <= 8 * 2^-24 * s64 for |x| <= 32, s64 the float64 sigmoid: s = 1 / (1 + exp(-x)) with an exp of at most 2 ulp (4 * 2^-24 relative, which the
    sum 1 + e passes on at most in full), one rounding of 1 + e (2^-24) and one of the divide (2^-24): 6 * 2^-24, rounded up to a power of two.  A bf16 tensor and
    its float32 copy give the same bits."""
    gen = torch.Generator(device="cpu").manual_seed(E + G)
    x = torch.randn(67, E, generator=gen) * 3.0
    x[0] = torch.linspace(-32.0, 32.0, E)
    x[1] = 32.0
    x[2] = -32.0
    x = x.clamp(-32.0, 32.0).to(torch.bfloat16)
    s16 = q.moe_topk_grouped(x.to(DEV), 1, n_group=G, topk_group=G, return_scores=True)[2]
    s32 = q.moe_topk_grouped(x.float().to(DEV), 1, n_group=G, topk_group=G, return_scores=True)[2]
    assert torch.equal(s16.view(torch.int32), s32.view(torch.int32))
    xf = (torch.randn(67, E, generator=gen) * 6.0).clamp(-32.0, 32.0)
    sf = q.moe_topk_grouped(xf.to(DEV), 1, n_group=G, topk_group=G, return_scores=True)[2]
    worst = 0.0
    for xs, ss in ((x, s16), (xf, sf)):
        s64 = 1.0 / (1.0 + np.exp(-_f64(xs)))
        err = np.abs(ss.cpu().numpy().astype(np.float64) - s64) / s64
        worst = max(worst, float(err.max() / U))
        assert (err <= 8 * U).all(), (E, G, err.max() / U)
    print(f"E={E} G={G}: sigmoid scores, max relative error {worst:.2f} x 2^-24 (bound 8)")
    edge = torch.tensor([[float("-inf"), float("inf"), 0.0, -0.0] * (E // 4)] if E % 4 == 0 else [[float("-inf")] * (E - 1) + [float("inf")]])
    se = q.moe_topk_grouped(edge.to(DEV), 1, n_group=G, topk_group=G, return_scores=True)[2].cpu().numpy()
    assert set(np.unique(se[edge.numpy() == float("-inf")])) == {0.0} and set(np.unique(se[edge.numpy() == float("inf")])) == {1.0}
    assert (se[edge.numpy() == 0.0] == 0.5).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E,G", SHAPES)
def test_softmax_scores_are_within_moe_topk_softmax_bound(q, E, G, dtype):
    """|p - p64| <= (E + 64) * 2^-24 * p64, moe_topk_softmax's bound (tests/test_gpu_moe_route.py): the scores are that op's p_j"""
    gen = torch.Generator(device="cpu").manual_seed(E + 17)
    x = torch.randn(67, E, generator=gen) * 3.0
    x[0] = -0.75
    x = x.to(dtype)
    x64 = _f64(x)
    assert np.abs(x64 - x64.max(axis=1, keepdims=True)).max() <= 32.0
    e = np.exp(x64 - x64.max(axis=1, keepdims=True))
    p64 = e / e.sum(axis=1, keepdims=True)
    s = q.moe_topk_grouped(x.to(DEV), 1, n_group=G, topk_group=G, scoring="softmax", return_scores=True)[2].cpu().numpy().astype(np.float64)
    err = np.abs(s - p64) / p64
    print(f"E={E} G={G} {dtype}: softmax scores, max relative error {err.max() / U:.2f} x 2^-24 (bound {E + 64})")
    assert (err <= (E + 64) * U).all(), (E, G, err.max() / U)


# ------------------------------------------------------------------------------------------------
# 4b. no effect from placement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", ["sigmoid", "softmax"])
def test_rows_that_do_not_start_on_16_bytes_give_the_same_bits(q, scoring):
    gen = torch.Generator(device="cpu").manual_seed(5)
    bias = _bias(64, 3).to(DEV)
    for dtype in DTYPES:
        buf = (torch.randn(1 + 33 * 64, generator=gen) * 3.0).to(dtype).to(DEV)
        view = buf[1:].view(33, 64)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        for G, tg in ((1, 1), (8, 3)):
            kw = dict(n_group=G, topk_group=tg, bias=bias, scoring=scoring, routed_scaling_factor=2.5)
            for rs in (False, True):
                a = q.moe_topk_grouped(view.clone(), 8, return_scores=rs, **kw)
                v = q.moe_topk_grouped(view, 8, return_scores=rs, **kw)
                assert all(torch.equal(i.view(torch.int32), j.view(torch.int32)) for i, j in zip(a, v)), (dtype, G, rs)
            assert np.array_equal(a[1].cpu().numpy(), grouped_topk_ref(a[2].cpu().numpy(), 8, n_group=G, topk_group=tg, bias=bias.cpu().numpy())[0])


# ------------------------------------------------------------------------------------------------
# 5. masked groups
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,G", [(8, 4), (60, 4), (160, 8), (256, 8), (1024, 64)])
def test_experts_of_masked_groups_are_never_taken(q, E, G):
    """(a) a strongly negative bias on every expert of the first half of the groups, zero elsewhere, and one more group kept than have no bias: a negative group
    survives, its experts (c < 0) are taken once the others run out, and no id leaves the surviving groups.  (b) the -inf mask against the zero fill: the chosen
    groups win on the sum of two strongly positive experts while all their other experts are strongly negative; the masked groups' c are all positive and still
    never taken.  Both are checked against the definition on the returned scores as well."""
    S = E // G
    gen = torch.Generator(device="cpu").manual_seed(E)
    x = (torch.randn(19, E, generator=gen) * 3.0).to(torch.bfloat16).to(DEV)
    group_of = np.arange(E) // S
    # (a)
    bias = np.where(group_of < G // 2, -4.0, 0.0).astype(np.float32)
    tg = G - G // 2 + 1
    topk = min(32, tg * S)
    w, ids, s = q.moe_topk_grouped(x, topk, n_group=G, topk_group=tg, bias=torch.from_numpy(bias).to(DEV), return_scores=True)
    ids_np = ids.cpu().numpy()
    want = grouped_topk_ref(s.cpu().numpy(), topk, n_group=G, topk_group=tg, bias=bias)[0]
    assert np.array_equal(ids_np, want)
    for row in ids_np:
        groups = set(group_of[row].tolist())
        assert len(groups) <= tg and len([g for g in groups if g < G // 2]) <= 1, row
    # (b)
    if S >= 3:
        chosen = np.arange(G) % 2 == 1                                               # every second group
        bias = np.where(chosen[group_of], -4.0, 0.0).astype(np.float32)
        bias[(np.arange(E) % S < 2) & chosen[group_of]] = 4.0
        tg = int(chosen.sum())
        topk = min(32, tg * S)
        assert topk > 2 * tg or topk == 32
        w, ids, s = q.moe_topk_grouped(x, topk, n_group=G, topk_group=tg, bias=torch.from_numpy(bias).to(DEV), renormalize=False, return_scores=True)
        ids_np, s_np = ids.cpu().numpy(), s.cpu().numpy()
        assert chosen[group_of[ids_np]].all()                                          # although every c outside is positive and most c inside are negative
        if topk > 2 * tg:
            assert (np.take_along_axis(s_np + bias, ids_np.astype(np.int64), axis=1)[:, 2 * tg:] < 0).all()
        assert np.array_equal(ids_np, grouped_topk_ref(s_np, topk, n_group=G, topk_group=tg, bias=bias)[0])
        assert np.array_equal(w.cpu().numpy(), np.take_along_axis(s_np, ids_np.astype(np.int64), axis=1))   # the bias never reaches a weight


def test_a_bias_of_minus_infinity_is_taken_last_or_not_at_all(q):
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(9, 16, generator=gen) * 3.0).to(DEV)
    bias = np.zeros(16, dtype=np.float32)
    bias[::4] = -np.inf                                                              # experts 0, 4, 8, 12
    b = torch.from_numpy(bias).to(DEV)
    for scoring in ("sigmoid", "softmax"):
        w, ids, s = q.moe_topk_grouped(x, 16, bias=b, scoring=scoring, return_scores=True)
        ids_np = ids.cpu().numpy()
        assert np.array_equal(ids_np[:, 12:], np.tile(np.arange(0, 16, 4), (9, 1))) and np.array_equal(ids_np, grouped_topk_ref(s.cpu().numpy(), 16, bias=bias)[0])
        ids12 = q.moe_topk_grouped(x, 12, bias=b, scoring=scoring)[1].cpu().numpy()
        assert (ids12 % 4 != 0).all() and np.array_equal(ids12, ids_np[:, :12])
        # in groups of four with the first expert of each masked: the two surviving groups are taken whole, their masked experts in the last two places
        ids_g = q.moe_topk_grouped(x, 8, n_group=4, topk_group=2, bias=b, scoring=scoring)[1].cpu().numpy()
        assert (ids_g[:, :6] % 4 != 0).all() and (ids_g[:, 6:] % 4 == 0).all() and all(len(set(r.tolist())) == 8 for r in ids_g)
        assert np.array_equal(ids_g, grouped_topk_ref(s.cpu().numpy(), 8, n_group=4, topk_group=2, bias=bias)[0])


# ------------------------------------------------------------------------------------------------
# 6. a non-finite row does not leak
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", ["sigmoid", "softmax"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E,G,tg,topk", [(8, 2, 1, 2), (160, 8, 3, 6), (1024, 64, 2, 32), (384, 1, 1, 8)])
def test_a_non_finite_row_does_not_leak(q, E, G, tg, topk, dtype, scoring):
    gen = torch.Generator(device="cpu").manual_seed(E)
    x = (torch.randn(9, E, generator=gen) * 3.0).to(dtype)
    bias = _bias(E, 1).to(DEV)
    bad = x.clone()
    bad[2, E // 3] = float("nan")
    bad[2, 0] = float("nan")
    bad[6, E - 1] = float("inf")
    bad[7] = float("nan")
    kw = dict(n_group=G, topk_group=tg, bias=bias, scoring=scoring, routed_scaling_factor=2.5)
    w0, i0, s0 = q.moe_topk_grouped(x.to(DEV), topk, return_scores=True, **kw)
    w1, i1, s1 = q.moe_topk_grouped(bad.to(DEV), topk, return_scores=True, **kw)
    good = [0, 1, 3, 4, 5, 8]
    assert torch.equal(i0[good], i1[good]) and torch.equal(w0[good].view(torch.int32), w1[good].view(torch.int32))
    assert torch.equal(s0[good].view(torch.int32), s1[good].view(torch.int32))
    for r in (2, 6, 7):
        row = i1[r].cpu().numpy()
        assert len(set(row.tolist())) == topk and row.min() >= 0 and row.max() < E, (r, row)


# ------------------------------------------------------------------------------------------------
# 7. agreement with moe_topk_softmax where both are defined
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E", [8, 60, 384, 1024])
def test_softmax_without_bias_in_one_group_agrees_with_moe_topk_softmax(q, E, dtype):
    """rows on a grid of quarters with |x - m| <= 16: exp merges no two different logits there (neighbours differ by a factor e^(1/4)), so selecting on the
    probabilities and selecting on the logits give the same ids, ties to the lower index in both.  The weights of both lie within (E + 64) * 2^-24 of one float64
    softmax."""
    gen = torch.Generator(device="cpu").manual_seed(E)
    x = (torch.round(torch.randn(67, E, generator=gen) * 12.0) / 4.0).clamp(-8.0, 8.0).to(dtype)
    x64 = _f64(x)
    e = np.exp(x64 - x64.max(axis=1, keepdims=True))
    p64 = e / e.sum(axis=1, keepdims=True)
    for topk in sorted({1, 2, 8, min(E, 32)}):
        for renorm in (False, True):
            w_s, i_s = q.moe_topk_softmax(x.to(DEV), topk, renormalize=renorm)
            w_g, i_g = q.moe_topk_grouped(x.to(DEV), topk, scoring="softmax", renormalize=renorm)
            assert torch.equal(i_s, i_g), (E, topk)
            w64 = np.take_along_axis(p64, i_s.cpu().numpy().astype(np.int64), axis=1)
            w64 = w64 / w64.sum(axis=1, keepdims=True) if renorm else w64
            for w in (w_s, w_g):
                assert (np.abs(w.cpu().numpy() - w64) <= (E + 64) * U * w64).all(), (E, topk, renorm)


# ------------------------------------------------------------------------------------------------
# 8. moe_route_grouped
# ------------------------------------------------------------------------------------------------
def _sort_ref(flat, E, topk):
    kept = (flat >= 0) & (flat < E)
    key = np.where(kept, flat, E)
    order = np.argsort(key, kind="stable")
    pos = np.empty(flat.size, dtype=np.int64)
    pos[order] = np.arange(flat.size)
    return (order // topk).astype(np.int32), np.cumsum(np.bincount(flat[kept], minlength=E)).astype(np.int32), np.where(kept, pos, -1).astype(np.int32)


def test_route_grouped_is_topk_grouped_then_the_fused_sort(q):
    E, G, tg, topk, T = 256, 8, 4, 8, 67
    x = _logits(T, E, torch.bfloat16, 11).to(DEV)
    bias = _bias(E, 2).to(DEV)
    kw = dict(n_group=G, topk_group=tg, bias=bias, routed_scaling_factor=2.5)
    w, ids = q.moe_topk_grouped(x, topk, **kw)
    r = q.moe_route_grouped(x, topk, **kw)
    assert len(r) == 5 and torch.equal(r[0].view(torch.int32), w.view(torch.int32)) and torch.equal(r[1], ids)
    for got, lib, want in zip(r[2:], q.moe_sort_fused(ids, E), _sort_ref(ids.cpu().numpy().astype(np.int64).reshape(-1), E, topk)):
        assert torch.equal(got, lib) and np.array_equal(got.cpu().numpy().reshape(-1), want)
    L = 64                                                                             # expert parallelism: this rank holds experts 64 .. 127
    emap = np.full(E, -1, dtype=np.int32)
    emap[64:128] = np.arange(L)
    em = torch.from_numpy(emap).to(DEV)
    r = q.moe_route_grouped(x, topk, L, expert_map=em, **kw)
    assert torch.equal(r[1], ids) and r[3].shape == (L,)
    mapped = emap[ids.cpu().numpy().reshape(-1)].astype(np.int64)
    for got, lib, want in zip(r[2:], q.moe_sort_fused(ids, L, expert_map=em), _sort_ref(mapped, L, topk)):
        assert torch.equal(got, lib) and np.array_equal(got.cpu().numpy().reshape(-1), want)


def test_route_grouped_replays_in_a_graph(q):
    E, G, tg, topk, T = 160, 8, 3, 6, 33
    gen = torch.Generator(device="cpu").manual_seed(31)
    logits = [(torch.randn(T, E, generator=gen) * 3.0).to(torch.bfloat16).to(DEV) for _ in range(2)]

    def step(lg):
        return q.moe_route_grouped(lg, topk, n_group=G, topk_group=tg, scoring="softmax", routed_scaling_factor=16.0)

    eager = [step(lg) for lg in logits]
    torch.cuda.synchronize()
    buf = logits[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        step(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a host synchronisation inside the ops would make the capture fail)
        cap = step(buf)
    for j in (1, 0, 1):
        buf.copy_(logits[j])
        for t in cap:
            t.view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        for i, (c, e) in enumerate(zip(cap, eager[j])):
            assert torch.equal(c.view(torch.int32), e.view(torch.int32)), (j, i)


# ------------------------------------------------------------------------------------------------
# 9. a whole layer with this router in front
# ------------------------------------------------------------------------------------------------
def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(DEV)


def test_moe_layer_behind_the_grouped_router_is_byte_equal_to_the_chain_fed_by_the_definition(q):
    """E = 8 in 4 groups, top-2 groups, top-2, bias, plain weights times 2.5 (exact in numpy): the layer behind moe_route_grouped equals the same chain fed with ids
    and weights computed by grouped_topk_ref from the returned scores"""
    T, E, G, tg, topk, H, I, R = 35, 8, 4, 2, 2, 256, 128, 32
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(8)
    tok = torch.randn(T, H, generator=gen).to(torch.bfloat16).to(DEV)
    w13 = torch.randn(E, 2 * I, H, generator=gen).to(torch.bfloat16).to(DEV)
    w2 = torch.randn(E, H, I, generator=gen).to(torch.bfloat16).to(DEV)
    alpha = torch.ones(1, device=DEV)
    logits = torch.randn(T, E, generator=gen).to(DEV)
    bias = _bias(E, 4)

    def quant_w(w):   # (E, N, K) -> codes (E, N, K/2), row-major scales (E * N * K / 32)
        c, s = q.fusedQuantizeMx(w.view(-1, w.size(-1)), h, method="abs_max")
        return c.view(w.size(0), w.size(1), -1), s.view(torch.uint8).reshape(-1)[: w.numel() // 32].clone().view(torch.float8_e8m0fnu)

    w13q, w13s = quant_w(w13)
    w2q, w2s = quant_w(w2)

    def layer(src_row, offs, pos, weights):
        aq, asf = q.fusedGatherQuantizeMx(tok, h, src_row, method="abs_max")
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
        return q.moe_combine(q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs), pos, weights)

    kw = dict(n_group=G, topk_group=tg, bias=bias.to(DEV), renormalize=False, routed_scaling_factor=2.5)
    weights, ids, src_row, offs, pos = q.moe_route_grouped(logits, topk, **kw)
    out = layer(src_row, offs, pos, weights)
    s = q.moe_topk_grouped(logits, topk, return_scores=True, **kw)[2].cpu().numpy()
    ref_ids, ref_w = grouped_topk_ref(s, topk, n_group=G, topk_group=tg, bias=bias.numpy(), renormalize=False, routed_scaling_factor=2.5)
    assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(weights.cpu().numpy(), ref_w)
    ref = layer(*q.moe_sort(torch.from_numpy(ref_ids).to(DEV), E), torch.from_numpy(ref_w).to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    assert np.array_equal(_np(out), _np(ref)), int((_np(out) != _np(ref)).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0
