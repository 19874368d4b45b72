"""Per-expert global scales in the NVFP4 MoE quantizers on the GPU: fusedGatherQuantizeNvGrouped and fusedSiluMulQuantizeNvGrouped against the per-expert
composition of the single-scale ops (byte for byte: codes and the first M * K / 16 scale bytes), a second round of the capped grid, method quest, malformed offs,
graph capture with the routing changed between replays, and a whole NVFP4 MoE layer with per-expert activation and weight scales against the same layer computed
expert by expert with the single-scale ops and the dense GEMM.  Every case uses scales that are pairwise different and no powers of two, and first checks that the
single-scale op with global_scales[0] does NOT give the composed bytes in any non-empty group g > 0 -- a kernel that ignored offs would otherwise pass.  The CPU half
is tests/test_moe_grouped_scales_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)

DEV = "cuda:0"
ROTS = (16, 32, 64, 128)


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _np(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.uint16).numpy()
    if t.element_size() == 1:
        return t.view(torch.uint8).numpy()
    return t.numpy()


def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(DEV)


def _scales(E):
    """E global scales, pairwise different, none a power of two, every one at least 1.9 x the first (so that no group g > 0 can come out as under scale 0)"""
    g = np.arange(1, E)
    s = np.concatenate([[0.37], 0.37 * 1.9 ** (1 + (g - 1) % 5) + 0.0137 * g]).astype(np.float32)
    assert len(np.unique(s)) == E and ((s.view(np.uint32) & 0x7fffff) != 0).all() and (s[1:] >= 1.9 * s[0]).all()
    return torch.from_numpy(s).to(DEV)


def _offs_patterns(M):
    """(name, E, counts): the groups' row counts; sum(counts) < M leaves tail rows past offs[E - 1], which belong to expert E - 1"""
    def counts(E, owners, total):   # total rows dealt to the owners in turn
        c = np.zeros(E, dtype=np.int64)
        for i in range(total):
            c[owners[i % len(owners)]] += 1
        return c

    e3 = np.diff([0, min(31, M), min(32, M), min(33, M)])   # boundaries at rows 31 / 32 / 33; for M > 33 the rest is a tail
    e5 = np.array([M - 1 - (M - 1) // 3, 0, 1, 0, (M - 1) // 3])   # two empty groups (more for M = 1) and a one-row group
    return [("E1", 1, np.array([M])), ("E3", 3, e3), ("E5", 5, e5), ("E65", 65, counts(65, list(range(64, -1, -1)) if M < 65 else list(range(65)), M)),
            ("E1024", 1024, counts(1024, [517, 3, 1023], M)), ("E5tail", 5, counts(5, [0, 2, 3], M - min(7, M - 1)))]


def _codes_sf(pair, rows, k):
    """codes (rows, K / 2) and the flat scale bytes as (rows, K / 16)"""
    return _np(pair[0]).reshape(rows, k // 2), _np(pair[1]).reshape(-1)[: rows * k // 16].reshape(rows, k // 16)


def _check_against_composition(single, grouped, gs, counts, M, k, ctx):
    """single(lo, hi, scale (1,)) -> the single-scale op on rows [lo, hi) of the operand; grouped: the op under test on all M rows.  Asserts the precondition (scale 0
    alone does not give the composed bytes) and then equality with the composition, group by group and for the tail under the last expert's scale."""
    E = len(counts)
    ends = np.cumsum(counts)
    bounds = [(g, int(ends[g] - counts[g]), int(ends[g])) for g in range(E) if counts[g]]
    if ends[-1] < M:
        bounds.append((E - 1, int(ends[-1]), M))
    want_c, want_s = np.zeros((M, k // 2), np.uint8), np.zeros((M, k // 16), np.uint8)
    for g, lo, hi in bounds:
        want_c[lo:hi], want_s[lo:hi] = _codes_sf(single(lo, hi, gs[g:g + 1]), hi - lo, k)
    base_c, base_s = _codes_sf(single(0, M, gs[0:1]), M, k)
    for g, lo, hi in bounds:
        if g > 0:
            assert (base_c[lo:hi] != want_c[lo:hi]).any() or (base_s[lo:hi] != want_s[lo:hi]).any(), (ctx, "scale 0 gives group", g, "its composed bytes")
    got_c, got_s = _codes_sf(grouped, M, k)
    assert np.array_equal(got_c, want_c), (ctx, "codes", np.nonzero((got_c != want_c).any(1))[0][:8])
    assert np.array_equal(got_s, want_s), (ctx, "scales", np.nonzero((got_s != want_s).any(1))[0][:8])


def _gather_case(q, rot, T, M, k, counts, gen, ctx):
    h = _hadamard(rot)
    x = (torch.randn(T, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(0, T, (M,), generator=gen, dtype=torch.int32).to(DEV)
    gs = _scales(len(counts))
    offs = torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)
    grouped = q.fusedGatherQuantizeNvGrouped(x, h, gs, src, offs)
    assert grouped[0].shape == (M, k // 2) and grouped[1].dtype == torch.float8_e4m3fn
    _check_against_composition(lambda lo, hi, s: q.fusedQuantizeNv(x.index_select(0, src[lo:hi]), h, s, method="abs_max"), grouped, gs, counts, M, k, ctx)


def _gated_case(q, rot, M, k, counts, gen, ctx):
    h = _hadamard(rot)
    x = (torch.randn(M, 2 * k, generator=gen) * 2.0).to(torch.bfloat16).to(DEV)
    gs = _scales(len(counts))
    offs = torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)
    grouped = q.fusedSiluMulQuantizeNvGrouped(x, h, gs, offs)
    assert grouped[0].shape == (M, k // 2) and grouped[1].dtype == torch.float8_e4m3fn
    _check_against_composition(lambda lo, hi, s: q.fusedSiluMulQuantizeNv(x[lo:hi], h, s, method="abs_max"), grouped, gs, counts, M, k, ctx)


# ------------------------------------------------------------------------------------------------
# 1. / 2. byte for byte against the per-expert composition of the single-scale ops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTS)
def test_gather_equals_the_per_expert_composition(q, rot):
    gen = torch.Generator(device="cpu").manual_seed(100 + rot)
    for kk in (1, 3, 5):   # 32 logical rows per tile, rows that straddle tiles, both
        for M in (1, 33, 140):
            for name, E, counts in _offs_patterns(M):
                _gather_case(q, rot, 33, M, kk * max(rot, 32), counts, gen, (rot, kk, M, name))
    torch.cuda.synchronize()


@pytest.mark.parametrize("rot", ROTS)
def test_gated_equals_the_per_expert_composition(q, rot):
    gen = torch.Generator(device="cpu").manual_seed(200 + rot)
    for kk in (1, 3, 5):
        for M in (1, 33, 140):
            for name, E, counts in _offs_patterns(M):
                _gated_case(q, rot, M, kk * max(rot, 32), counts, gen, (rot, kk, M, name))
    torch.cuda.synchronize()


def test_the_offs_patterns_are_what_they_claim():
    for M in (1, 33, 140):
        pats = {name: (E, c) for name, E, c in _offs_patterns(M)}
        assert all(len(c) == E and (c >= 0).all() and c.sum() <= M for E, c in pats.values())
        assert all(c.sum() == M for n, (E, c) in pats.items() if n not in ("E3", "E5tail"))
        assert (pats["E5"][1] == 0).sum() >= 2 and pats["E5"][1][2] == 1 and (pats["E1024"][1] == 0).sum() >= 1021
    p = dict((n, c) for n, _, c in _offs_patterns(140))
    assert list(np.cumsum(p["E3"])) == [31, 32, 33] and p["E5tail"].sum() == 133 and (p["E65"] > 0).all()


# ------------------------------------------------------------------------------------------------
# 3. a second round of the capped grid: the one-tile-ahead scale lookup crosses rounds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [32, 128])
@pytest.mark.parametrize("kind", ["gather", "gated"])
def test_second_grid_round(q, rot, kind):
    """9.4 M outputs: more than one pass of the capped grid (8.4 M elements), so every wave walks on to a second, partial round of tiles"""
    gen = torch.Generator(device="cpu").manual_seed(rot)
    M, k = 2051, 4608
    counts = np.array([300, 0, 511, 1, 700, 38, 501])   # E = 7
    assert counts.sum() == M
    if kind == "gather":
        _gather_case(q, rot, 64, M, k, counts, gen, (rot, kind))
    else:
        _gated_case(q, rot, M, k, counts, gen, (rot, kind))


# ------------------------------------------------------------------------------------------------
# 4. quest reads no global scale: the grouped entry gives the single-scale op's bytes, whatever the scales
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTS)
def test_quest_equals_the_single_scale_op(q, rot):
    gen = torch.Generator(device="cpu").manual_seed(300 + rot)
    T, M, k, E = 33, 70, 3 * max(rot, 32), 5
    h = _hadamard(rot)
    gs = _scales(E)
    offs = torch.tensor([20, 20, 21, 50, 70], dtype=torch.int32, device=DEV)
    x = (torch.randn(T, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(0, T, (M,), generator=gen, dtype=torch.int32).to(DEV)
    xg = (torch.randn(M, 2 * k, generator=gen) * 2.0).to(torch.bfloat16).to(DEV)
    for got, want in ((q.fusedGatherQuantizeNvGrouped(x, h, gs, src, offs, method="quest"), q.fusedGatherQuantizeNv(x, h, gs[3:4], src, method="quest")),
                      (q.fusedSiluMulQuantizeNvGrouped(xg, h, gs, offs, method="quest"), q.fusedSiluMulQuantizeNv(xg, h, gs[1:2], method="quest"))):
        (gc, gsf), (wc, wsf) = _codes_sf(got, M, k), _codes_sf(want, M, k)
        assert np.array_equal(gc, wc) and np.array_equal(gsf, wsf), rot


# ------------------------------------------------------------------------------------------------
# 5. malformed offs: the call returns and every row carries the bytes of ONE of the experts' scales (all loads are bounded by construction: this looks for wrong
#    bytes, it cannot provoke a fault)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("seq", [[-5, 2 ** 31 - 1, 3], [49, 0, 0], [7, 3, 20]])
def test_malformed_offs_give_some_experts_bytes(q, rot, seq):
    gen = torch.Generator(device="cpu").manual_seed(400 + rot)
    T, M, k, E = 33, 40, 3 * max(rot, 32), 3
    assert seq[0] in (-5, M + 9, 7)
    h = _hadamard(rot)
    gs = _scales(E)
    offs = torch.tensor(seq, dtype=torch.int32, device=DEV)
    x = (torch.randn(T, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(0, T, (M,), generator=gen, dtype=torch.int32).to(DEV)
    xg = (torch.randn(M, 2 * k, generator=gen) * 2.0).to(torch.bfloat16).to(DEV)
    runs = ((q.fusedGatherQuantizeNvGrouped(x, h, gs, src, offs), [q.fusedGatherQuantizeNv(x, h, gs[g:g + 1], src) for g in range(E)]),
            (q.fusedSiluMulQuantizeNvGrouped(xg, h, gs, offs), [q.fusedSiluMulQuantizeNv(xg, h, gs[g:g + 1]) for g in range(E)]))
    torch.cuda.synchronize()   # the call returned
    for got, singles in runs:
        gc, gsf = _codes_sf(got, M, k)
        match = np.zeros(M, dtype=bool)
        for one in singles:
            oc, osf = _codes_sf(one, M, k)
            match |= (gc == oc).all(1) & (gsf == osf).all(1)
        assert match.all(), (rot, seq, np.nonzero(~match)[0])


# ------------------------------------------------------------------------------------------------
# 6. graph capture: route -> grouped-scale gather-quantize -> grouped GEMM, replayed with different routing
# ------------------------------------------------------------------------------------------------
def _quant_weights(q, w, h, w_gs):
    """(E, N, K) bf16 -> codes (E, N, K / 2), row-major e4m3 scales (E * N * K / 16), expert g under its own global scale w_gs[g]"""
    E, N, K = w.shape
    cs = [q.fusedQuantizeNv(w[g], h, w_gs[g:g + 1], method="abs_max") for g in range(E)]
    codes = torch.stack([c for c, _ in cs])
    sf = torch.cat([s.view(torch.uint8).reshape(-1)[: N * K // 16] for _, s in cs]).view(torch.float8_e4m3fn)
    return codes, sf


def test_graph_capture_replays_with_different_routing(q):
    T, E, topk, H, N, R = 33, 8, 2, 256, 128, 32
    gen = torch.Generator(device="cpu").manual_seed(61)
    h = _hadamard(R)
    tok = torch.randn(T, H, generator=gen).to(torch.bfloat16).to(DEV)
    a_gs = _scales(E)
    w_gs = torch.flip(_scales(E), [0]).contiguous()
    wq, ws = _quant_weights(q, torch.randn(E, N, H, generator=gen).to(torch.bfloat16).to(DEV), h, w_gs)
    alpha = (1.0 / (a_gs * w_gs)).contiguous()
    logits = [torch.randn(T, E, generator=gen).to(DEV) for _ in range(3)]
    logits[2][:, 5] = -30.0   # an expert that gets no row

    def run(lg):
        _, _, src_row, offs, _ = q.moe_route(lg, topk)
        aq, asf = q.fusedGatherQuantizeNvGrouped(tok, h, a_gs, src_row, offs)
        return aq, asf, q.grouped_matmul_nvf4_bf16_tn(aq, wq, asf, ws, alpha, offs), offs

    eager = []
    for lg in logits:
        aq, asf, out, offs = run(lg)
        eager.append((_np(aq), _np(asf).reshape(-1)[: T * topk * H // 16].copy(), _np(out), _np(offs)))
    assert not np.array_equal(eager[0][3], eager[1][3]) and eager[2][3][5] == eager[2][3][4]
    static = logits[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run(static)
    for lg, want in zip(logits, eager):
        static.copy_(lg)
        cap[0].zero_()
        cap[2].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(cap[3]), want[3])
        assert np.array_equal(_np(cap[0]), want[0]) and np.array_equal(_np(cap[1]).reshape(-1)[: want[1].size], want[1])
        assert np.array_equal(_np(cap[2]), want[2])


# ------------------------------------------------------------------------------------------------
# 7. a whole NVFP4 MoE layer with per-expert a13_gs, a2_gs and weight scales, against the same layer expert by expert with the single-scale ops and the dense GEMM
# ------------------------------------------------------------------------------------------------
def test_moe_layer_end_to_end_is_bit_equal_to_the_per_expert_layer(q):
    from qutlass_amd.utils import to_blocked

    T, E, topk, H, I, R = 33, 8, 2, 256, 256, 32
    gen = torch.Generator(device="cpu").manual_seed(71)
    h = _hadamard(R)
    tok = torch.randn(T, H, generator=gen).to(torch.bfloat16).to(DEV)
    s = _scales(3 * E)
    a13_gs, a2_gs, w13_gs = s[:E].contiguous(), s[E:2 * E].contiguous(), s[2 * E:].contiguous()
    w2_gs = torch.flip(a13_gs, [0]).contiguous()
    w13q, w13s = _quant_weights(q, (torch.randn(E, 2 * I, H, generator=gen) * 0.2).to(torch.bfloat16).to(DEV), h, w13_gs)
    w2q, w2s = _quant_weights(q, (torch.randn(E, H, I, generator=gen) * 0.2).to(torch.bfloat16).to(DEV), h, w2_gs)
    alpha13, alpha2 = (1.0 / (a13_gs * w13_gs)).contiguous(), (1.0 / (a2_gs * w2_gs)).contiguous()
    logits = torch.randn(T, E, generator=gen).to(DEV)
    logits[:, 6] = -30.0   # expert 6 stays empty

    weights, ids, src_row, offs, pos = q.moe_route(logits, topk)
    aq, asf = q.fusedGatherQuantizeNvGrouped(tok, h, a13_gs, src_row, offs)
    gate_up = q.grouped_matmul_nvf4_bf16_tn(aq, w13q, asf, w13s, alpha13, offs)
    bq, bsf = q.fusedSiluMulQuantizeNvGrouped(gate_up, h, a2_gs, offs)
    out = q.moe_combine(q.grouped_matmul_nvf4_bf16_tn(bq, w2q, bsf, w2s, alpha2, offs), pos, weights)

    ends = [0] + offs.cpu().tolist()
    assert ends[-1] == T * topk and ends[7] == ends[6] and sum(b > a for a, b in zip(ends, ends[1:])) >= 5
    y_ref = torch.zeros(T * topk, H, dtype=torch.bfloat16, device=DEV)
    for g in range(E):
        lo, hi = ends[g], ends[g + 1]
        if hi == lo:
            continue
        n = hi - lo
        cq, csf = q.fusedQuantizeNv(tok.index_select(0, src_row[lo:hi]), h, a13_gs[g:g + 1], method="abs_max")
        gu = q.matmul_nvf4_bf16_tn(cq, w13q[g], to_blocked(csf.view(torch.uint8).reshape(-1)[: n * H // 16].view(torch.float8_e4m3fn).view(n, H // 16)),
                                   to_blocked(w13s[g * 2 * I * H // 16:(g + 1) * 2 * I * H // 16].view(2 * I, H // 16)), alpha13[g:g + 1])
        dq, dsf = q.fusedSiluMulQuantizeNv(gu, h, a2_gs[g:g + 1], method="abs_max")
        y_ref[lo:hi] = q.matmul_nvf4_bf16_tn(dq, w2q[g], to_blocked(dsf.view(torch.uint8).reshape(-1)[: n * I // 16].view(torch.float8_e4m3fn).view(n, I // 16)),
                                             to_blocked(w2s[g * H * I // 16:(g + 1) * H * I // 16].view(H, I // 16)), alpha2[g:g + 1])
    want = q.moe_combine(y_ref, pos, weights)
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    assert np.array_equal(_np(out), _np(want)), int((_np(out) != _np(want)).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0


@pytest.mark.parametrize("rot", ROTS)
def test_exact_arithmetic_case_is_bit_equal_to_the_oracle_per_group(q, rot):
    """integer-valued x in -2 .. 2 times 100 and a Hadamard rotation: every product and sum of the rotation is exact, the tolerance is zero"""
    T, M, k = 37, 53, 3 * max(rot, 32)
    gen = torch.Generator(device="cpu").manual_seed(5 + rot)
    x = (torch.randint(-2, 3, (T, k), generator=gen).float() * 100.0).to(torch.bfloat16)
    src = torch.randint(0, T, (M,), generator=gen, dtype=torch.int32)
    h = _hadamard(rot)
    counts = np.array([20, 0, 1, 25, 7])
    gs = _scales(5)
    offs = torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)
    codes, sf = _codes_sf(q.fusedGatherQuantizeNvGrouped(x.to(DEV), h, gs, src.to(DEV), offs), M, k)
    xg_bits = _np(x)[src.numpy()]
    ends = np.cumsum(counts)
    for g in range(5):
        lo, hi = int(ends[g] - counts[g]), int(ends[g])
        if hi == lo:
            continue
        rq, rs = oracle.fused_quantize_nv(xg_bits[lo:hi], _np(h), float(gs[g]), oracle.ABS_MAX, acc_model=1)
        assert np.array_equal(sf[lo:hi].reshape(-1), rs.reshape(-1)[: (hi - lo) * k // 16]), (rot, g)
        assert oracle.codes_equal_mod_zero_sign(codes[lo:hi].reshape(-1), rq.reshape(-1)).all(), (rot, g)
