"""MoE routing on the GPU: moe_topk_softmax's ids against a numpy stable argsort of the logits (exact, ties included) and its weights against a float64 softmax
within a derived bound, non-finite rows, moe_sort_fused against moe_sort and a numpy stable sort on all three results (both launch shapes, dropped ids, expert_map),
graph capture of moe_route, and a whole layer from the router's logits.  The checkers are numpy code in this file.  The CPU half is tests/test_moe_route_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
EXPERTS = [1, 2, 8, 60, 64, 65, 128, 129, 256, 1024]
TOKENS = [1, 3, 64, 257]
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _topks(E):
    return sorted({k for k in (1, 2, 8, min(E, 32)) if k <= min(E, 32)})


def _f64(logits: torch.Tensor) -> np.ndarray:
    return logits.detach().cpu().float().numpy().astype(np.float64)   # bf16 -> float32 -> float64: both exact


def _np(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint16).numpy() if t.dtype == torch.bfloat16 else t.numpy()


def _logits(T, E, dtype, topk, seed):
    """randn * 3, every second row on a grid of quarters (exact ties in float32 too; bf16 randn at E = 1024 has plenty on its own); when there is room, a row of
    all-equal logits, a row of +0.0 / -0.0 mixed and a row with -inf entries, fewer than E - topk of them"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T, E, generator=gen) * 3.0
    x[1::2] = torch.round(x[1::2] * 4.0) / 4.0
    if T >= 3:
        x[0] = 1.25
        x[1] = torch.where(torch.rand(E, generator=gen) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        ninf = min(max(E - topk - 1, 0), max(E // 3, 1))
        if ninf > 0:
            x[2, torch.randperm(E, generator=gen)[:ninf]] = float("-inf")
    return x.to(dtype)


# ------------------------------------------------------------------------------------------------
# 1. ids are exact: the first topk of (logit descending, expert index ascending)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E", EXPERTS)
def test_ids_equal_a_stable_argsort_of_the_logits(q, E, dtype):
    for topk in _topks(E):
        for T in TOKENS:
            x = _logits(T, E, dtype, topk, seed=E * 1000 + topk * 10 + T)
            w, ids = q.moe_topk_softmax(x.to(DEV), topk)
            assert w.shape == ids.shape == (T, topk) and w.dtype == torch.float32 and ids.dtype == torch.int32
            want = np.argsort(-_f64(x), axis=1, kind="stable")[:, :topk]
            got = ids.cpu().numpy()
            assert np.array_equal(got, want), (E, topk, T, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    w, ids = q.moe_topk_softmax(torch.empty(0, E, dtype=dtype, device=DEV), 1)
    assert w.shape == ids.shape == (0, 1)


def test_ids_are_exact_on_rows_that_do_not_start_on_16_bytes(q):
    """a contiguous view whose rows start off the 16-byte grid takes the one-column-per-load path: same ids, same weights as the aligned copy"""
    gen = torch.Generator(device="cpu").manual_seed(5)
    for dtype in DTYPES:
        buf = (torch.randn(1 + 33 * 64, generator=gen) * 3.0).to(dtype).to(DEV)
        view = buf[1:].view(33, 64)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        w_a, i_a = q.moe_topk_softmax(view.clone(), 8)
        w_v, i_v = q.moe_topk_softmax(view, 8)
        assert np.array_equal(i_a.cpu().numpy(), np.argsort(-_f64(view), axis=1, kind="stable")[:, :8])
        assert torch.equal(i_a, i_v) and torch.equal(w_a, w_v)


# ------------------------------------------------------------------------------------------------
# 2. weights against a float64 softmax of the same logits, at the ids the kernel returned
# ------------------------------------------------------------------------------------------------
def _softmax64(x64):
    e = np.exp(x64 - x64.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("renorm", [True, False], ids=["renorm", "plain"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E", EXPERTS)
def test_weights_are_the_softmax_within_the_derived_bound(q, E, dtype, renorm):
    """|w - w64| <= (E + 64) * 2^-24 * w64: (E - 1) * 2^-24 bounds an fp32 sum of E positive terms in any order; the other 64 units cover the rounding of the
    exponent's argument for |x - m| <= 32 (2^-19), a 2-ulp exp, the divides and the renormalising sum of at most 32 terms."""
    T = 67
    gen = torch.Generator(device="cpu").manual_seed(E + 17)
    x = torch.randn(T, E, generator=gen) * 3.0
    x[0] = -0.75                                   # all equal: every weight is 1 / E, or 1 / topk renormalised
    x[1] = 2.0 - 1.0                               # two levels: one logit at c, the rest at c - 1
    x[1, E // 2] = 2.0
    x = x.to(dtype)
    x64 = _f64(x)
    assert np.abs(x64 - x64.max(axis=1, keepdims=True)).max() <= 32.0
    p64 = _softmax64(x64)
    for topk in _topks(E):
        w, ids = q.moe_topk_softmax(x.to(DEV), topk, renormalize=renorm)
        ids_np, w_np = ids.cpu().numpy(), w.cpu().numpy().astype(np.float64)
        assert np.array_equal(ids_np, np.argsort(-x64, axis=1, kind="stable")[:, :topk])
        w64 = np.take_along_axis(p64, ids_np.astype(np.int64), axis=1)
        if renorm:
            w64 = w64 / w64.sum(axis=1, keepdims=True)
            assert np.abs(w_np.sum(axis=1) - 1.0).max() <= 64 * 2.0 ** -24, (E, topk, np.abs(w_np.sum(axis=1) - 1.0).max())
        err = np.abs(w_np - w64) / w64
        print(f"E={E} topk={topk} {dtype} renorm={renorm}: max relative error {err.max() / 2.0 ** -24:.2f} x 2^-24 (bound {E + 64})")
        assert (np.abs(w_np - w64) <= (E + 64) * 2.0 ** -24 * w64).all(), (E, topk, err.max() / 2.0 ** -24)
        want0 = 1.0 / topk if renorm else 1.0 / E
        assert np.abs(w_np[0] - want0).max() <= (E + 64) * 2.0 ** -24 * want0
        lo = 1.0 / (np.e + E - 1)                  # the two-level row: e / (e + E - 1) once, 1 / (e + E - 1) for the rest, lowest indices first
        want1 = np.array([np.e * lo] + [lo] * (topk - 1))
        want1 = want1 / want1.sum() if renorm else want1
        assert ids_np[1, 0] == E // 2 and np.array_equal(ids_np[1, 1:], [j for j in range(E) if j != E // 2][: topk - 1])
        assert (np.abs(w_np[1] - want1) <= (E + 64) * 2.0 ** -24 * want1).all()


def test_masked_experts_get_probability_zero(q):
    x = torch.randn(5, 16, generator=torch.Generator().manual_seed(3)) * 3.0
    x[:, ::2] = float("-inf")                      # 8 of 16 masked: topk = 12 has to take 4 of them, last, in index order, with weight 0
    w, ids = q.moe_topk_softmax(x.to(DEV), 12, renormalize=False)
    ids_np, w_np = ids.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(ids_np, np.argsort(-_f64(x), axis=1, kind="stable")[:, :12])
    assert np.array_equal(ids_np[:, 8:], np.tile(np.arange(0, 8, 2), (5, 1))) and (w_np[:, 8:] == 0).all() and (w_np[:, :8] > 0).all()
    assert np.abs(w_np.sum(axis=1) - 1.0).max() <= 64 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------
# 3. a non-finite row does not leak
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("E,topk", [(8, 2), (129, 8), (1024, 32)])
def test_a_non_finite_row_does_not_leak(q, E, topk, dtype):
    gen = torch.Generator(device="cpu").manual_seed(E)
    x = (torch.randn(9, E, generator=gen) * 3.0).to(dtype)
    bad = x.clone()
    bad[2, E // 3] = float("nan")
    bad[2, 0] = float("nan")
    bad[6, E - 1] = float("inf")
    bad[7] = float("-inf")                          # nothing but -inf: unspecified weights too
    w0, i0 = q.moe_topk_softmax(x.to(DEV), topk)
    w1, i1 = q.moe_topk_softmax(bad.to(DEV), topk)
    good = [0, 1, 3, 4, 5, 8]
    assert torch.equal(i0[good], i1[good]) and torch.equal(w0[good], w1[good])
    for r in (2, 6, 7):
        row = i1[r].cpu().numpy()
        assert len(set(row.tolist())) == topk and row.min() >= 0 and row.max() < E, (r, row)


# ------------------------------------------------------------------------------------------------
# 4. moe_sort_fused equals moe_sort and a numpy stable sort, exactly, on all three results
# ------------------------------------------------------------------------------------------------
def _one_launch_bound(q, E):
    """the largest n with no workspace: workspace_bytes is 0 up to it and monotone beyond (tests/test_moe_route_cpu.py)"""
    ws = q._lib.load().qutlass_amd_moe_sort_workspace_bytes
    lo, hi = 1, 1 << 30
    assert ws(lo, E) == 0 and ws(hi, E) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ws(mid, E) == 0 else (lo, mid)
    return lo


def _shape_for(n):
    topk = next(k for k in (8, 5, 3, 2, 1) if n % k == 0)
    return n // topk, topk


def _routing(n, E, pattern, rng):
    if pattern == "uniform":
        ids = rng.integers(0, E, n)
    elif pattern == "one":
        ids = np.full(n, E - 1)
    else:   # skewed: half of the slots in expert 0, the rest on a few experts
        ids = np.where(rng.random(n) < 0.5, 0, rng.integers(0, max(E // 4, 1), n))
    ids = ids.astype(np.int64)
    if n >= 8:   # dropped ids
        where = rng.permutation(n)[: max(4, n // 16)]
        ids[where] = np.array([-1, E, I32_MIN, I32_MAX])[np.arange(where.size) % 4]
    return ids


def _sort_ref(flat, E, topk):
    kept = (flat >= 0) & (flat < E)
    key = np.where(kept, flat, E)
    order = np.argsort(key, kind="stable")
    pos = np.empty(flat.size, dtype=np.int64)
    pos[order] = np.arange(flat.size)
    return (order // topk).astype(np.int32), np.cumsum(np.bincount(flat[kept], minlength=E)).astype(np.int32), np.where(kept, pos, -1).astype(np.int32)


def _check_fused_sort(q, flat, E, T, topk, dtype, ctx, expert_map=None, mapped=None):
    ids = torch.from_numpy(flat.reshape(T, topk)).to(dtype).to(DEV)
    got = q.moe_sort_fused(ids, E, expert_map=expert_map)
    eq_ids = ids if mapped is None else torch.from_numpy(mapped.reshape(T, topk)).to(dtype).to(DEV)
    lib = q.moe_sort(eq_ids, E)
    want = _sort_ref(flat if mapped is None else mapped, E, topk)
    for name, g, l, w in zip(("src_row", "offs", "pos"), got, lib, want):
        assert g.dtype == torch.int32 and g.shape == l.shape, (ctx, name)
        g_np = g.cpu().numpy()
        assert np.array_equal(g_np.reshape(-1), w), (ctx, name, "numpy", int((g_np.reshape(-1) != w).sum()))
        assert torch.equal(g, l), (ctx, name, "moe_sort")
    return got


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("E", [1, 8, 60, 128, 1024])
def test_sort_fused_equals_moe_sort_and_numpy(q, E, dtype):
    bound = _one_launch_bound(q, E)
    assert bound >= 4096
    rng = np.random.default_rng(E)
    sizes = [1, 63, 64, 65, 1000, bound, bound + 1, 40000]
    for n in sizes:
        T, topk = _shape_for(n)
        for pattern in ("uniform", "one", "skewed"):
            flat = _routing(n, E, pattern, rng)
            got = _check_fused_sort(q, flat, E, T, topk, dtype, (n, E, pattern))
            if n == sizes[-1]:   # the largest case twice: identical bytes
                again = q.moe_sort_fused(torch.from_numpy(flat.reshape(T, topk)).to(dtype).to(DEV), E)
                assert all(torch.equal(a, b) for a, b in zip(got, again)), (n, E, pattern)
    s, o, p = q.moe_sort_fused(torch.empty(0, 2, dtype=dtype, device=DEV), E)
    assert s.shape == (0,) and p.shape == (0, 2) and o.shape == (E,) and int(o.abs().sum()) == 0


def test_sort_fused_beyond_one_workgroup_per_256_blocks(q):
    """more than 256 * 4096 slots: the workgroups' ranges grow instead of their number; one case, int32, E = 128"""
    n, E = 256 * 4096 + 520, 128
    flat = _routing(n, E, "skewed", np.random.default_rng(9))
    _check_fused_sort(q, flat, E, *_shape_for(n), torch.int32, n)


# ------------------------------------------------------------------------------------------------
# 5. expert_map: two ranks of 8 local experts out of G = 16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [48, 20000])
def test_expert_map_gives_each_rank_its_own_sort(q, n):
    G, L = 16, 8
    rng = np.random.default_rng(n)
    flat = rng.integers(0, G, n).astype(np.int64)
    flat[rng.permutation(n)[:6]] = [-1, G, G + 5, I32_MAX, I32_MIN, -7]          # ids outside [0, G): dropped without reading the map
    T, topk = _shape_for(n)
    for rank in range(2):
        emap = np.full(G, -1, dtype=np.int32)
        emap[rank * L:(rank + 1) * L] = np.arange(L)
        if rank == 1:
            emap[3] = L                                                             # a map entry outside [0, L) other than -1 drops too
        mapped = np.where((flat >= 0) & (flat < G), emap[np.clip(flat, 0, G - 1)], -1).astype(np.int64)
        for dtype in (torch.int32, torch.int64):
            s, o, p = _check_fused_sort(q, flat, L, T, topk, dtype, (n, rank), expert_map=torch.from_numpy(emap).to(DEV), mapped=mapped)
        kept = (mapped >= 0) & (mapped < L)
        assert int(o[-1]) == int(kept.sum()) and (p.cpu().numpy().reshape(-1)[~kept] == -1).all()


# ------------------------------------------------------------------------------------------------
# 6. graph capture: moe_route followed by fusedGatherQuantizeMx, replayed on new logits
# ------------------------------------------------------------------------------------------------
def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("form", ["one_launch", "three_launches"])   # of the sort; the second allocates its scratch inside the capture
def test_graph_capture_replays_the_eager_results(q, form):
    E, topk, K = 64, 8, 256
    T = 33 if form == "one_launch" else _one_launch_bound(q, E) // topk + 5
    gen = torch.Generator(device="cpu").manual_seed(31)
    logits = [(torch.randn(T, E, generator=gen) * 3.0).to(torch.bfloat16).to(DEV) for _ in range(2)]
    x = (torch.randn(T, K, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    h = _hadamard(32)

    def step(lg):
        r = q.moe_route(lg, topk)
        return r + q.fusedGatherQuantizeMx(x, h, r[2], method="abs_max")

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
    n = T * topk * K // 32
    for j in (1, 0, 1):
        buf.copy_(logits[j])
        for t in cap:
            t.view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        for i, (c, e) in enumerate(zip(cap, eager[j])):
            if i == 6:   # flat e8m0 scales: the first n bytes
                assert torch.equal(c.view(torch.uint8).reshape(-1)[:n], e.view(torch.uint8).reshape(-1)[:n]), (j, i)
            else:
                assert torch.equal(c, e), (j, i)


# ------------------------------------------------------------------------------------------------
# 7. a whole layer from the router's logits
# ------------------------------------------------------------------------------------------------
def test_moe_layer_from_logits_is_byte_equal_to_the_torch_routing(q):
    T, E, topk, H, I, R = 35, 4, 2, 256, 128, 32
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(8)
    tok = torch.randn(T, H, generator=gen).to(torch.bfloat16).to(DEV)
    w13 = torch.randn(E, 2 * I, H, generator=gen).to(torch.bfloat16).to(DEV)
    w2 = torch.randn(E, H, I, generator=gen).to(torch.bfloat16).to(DEV)
    alpha = torch.ones(1, device=DEV)
    logits = torch.randn(T, E, generator=gen)
    assert all(len(set(r.tolist())) == E for r in logits)                                  # no ties: torch.topk has no choice to make
    logits = logits.to(DEV)

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

    weights, ids, src_row, offs, pos = q.moe_route(logits, topk)
    out = layer(src_row, offs, pos, weights)
    t_ids = torch.topk(torch.softmax(logits, dim=-1), topk, dim=-1).indices
    assert torch.equal(t_ids.to(torch.int32), ids)
    ref = layer(*q.moe_sort(t_ids, E), weights)
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    assert np.array_equal(_np(out), _np(ref)), int((_np(out) != _np(ref)).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0
