"""MoE dispatch and combine on the GPU: the gathering quantizers fusedGatherQuantize{Mx,Nv} against the library's own two steps (index_select + fusedQuantize*, bit
for bit) and against the pinned CPU oracle, out-of-range indices, the padding contract, moe_combine against its definition evaluated in numpy.float32, unreferenced
rows, graph capture, and a whole layer from (T, H) tokens plus router output to (T, H) results.  The CPU half is tests/test_moe_dispatch_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)

DEV = "cuda:0"
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


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


CASES = [("mx", r) for r in (32, 64, 128)] + [("nv", r) for r in (16, 32, 64, 128)]
GS = {"mx": 32, "nv": 16}


def _fused(q, fmt, x, h, src, method, gs):
    return q.fusedGatherQuantizeMx(x, h, src, method=method) if fmt == "mx" else q.fusedGatherQuantizeNv(x, h, gs, src, method=method)


def _plain(q, fmt, x, h, method, gs):
    return q.fusedQuantizeMx(x, h, method=method) if fmt == "mx" else q.fusedQuantizeNv(x, h, gs, method=method)


def _assert_same_bytes(fmt, fused, comp, numel, ctx):
    (fc, fs), (cc, cs) = fused, comp
    assert fc.shape == cc.shape and fc.dtype == cc.dtype and fs.shape == cs.shape and fs.dtype == cs.dtype, ctx
    assert np.array_equal(_np(fc), _np(cc)), (ctx, "codes", int((_np(fc) != _np(cc)).sum()))
    n = numel // GS[fmt]   # flat: the first numel / gs bytes are the scales, the rest of the buffer belongs to the caller
    a, b = _np(fs).reshape(-1)[:n], _np(cs).reshape(-1)[:n]
    assert np.array_equal(a, b), (ctx, "scales", int((a != b).sum()))


# ------------------------------------------------------------------------------------------------
# 1. fused equals composition, byte for byte
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rot", CASES)
@pytest.mark.parametrize("method", ["quest", "abs_max"])
def test_fused_equals_composition(q, fmt, rot, method):
    h = _hadamard(rot)
    gs = torch.tensor([3.0], device=DEV)
    rp = max(rot, 32)
    gen = torch.Generator(device="cpu").manual_seed(rot * 7 + (method == "quest"))
    for t in (1, 33, 70):
        for kk in (1, 3, 5):
            k = kk * rp
            x = (torch.randn(t, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
            for m in (1, 31, 33, 140):   # a ragged last tile, M > T with repeats, M < T
                src = torch.randint(0, t, (m,), generator=gen, dtype=torch.int32).to(DEV)
                fused = _fused(q, fmt, x, h, src, method, gs)
                comp = _plain(q, fmt, x.index_select(0, src), h, method, gs)
                _assert_same_bytes(fmt, fused, comp, m * k, (fmt, rot, method, t, k, m))
            ident = torch.arange(t, dtype=torch.int32, device=DEV)
            _assert_same_bytes(fmt, _fused(q, fmt, x, h, ident, method, gs), _plain(q, fmt, x, h, method, gs), t * k, (fmt, rot, method, t, k, "identity"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. a second round of the capped grid: the index prefetch crosses rounds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [32, 128])
def test_fused_equals_composition_second_grid_round(q, rot):
    """9.4 M outputs: more than one pass of the capped grid (8.4 M elements), so every wave walks on to a second, partial round of tiles"""
    h = _hadamard(rot)
    gen = torch.Generator(device="cpu").manual_seed(rot)
    t, k, m = 64, 4608, 2051
    x = (torch.randn(t, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(0, t, (m,), generator=gen, dtype=torch.int32).to(DEV)
    fused = _fused(q, "mx", x, h, src, "abs_max", None)
    comp = _plain(q, "mx", x.index_select(0, src), h, "abs_max", None)
    _assert_same_bytes("mx", fused, comp, m * k, rot)


# ------------------------------------------------------------------------------------------------
# 3. out-of-range indices give the bytes of an all-zero row (the loads are descriptor-bounded: a wrong range check gives wrong bytes, not a fault)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rot", CASES)
def test_out_of_range_indices_give_zero_rows(q, fmt, rot):
    h = _hadamard(rot)
    gs = torch.tensor([3.0], device=DEV)
    t, k, m = 33, 3 * max(rot, 32), 70
    gen = torch.Generator(device="cpu").manual_seed(31 + rot)
    x = (torch.randn(t, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(0, t, (m,), generator=gen, dtype=torch.int32)
    bad_at = torch.tensor([0, 5, 31, 32, 33, 47, 64, 69])
    src[bad_at] = torch.tensor([-1, t, I32_MIN, I32_MAX, -1, t + 1, I32_MAX - 1, -2], dtype=torch.int32)
    x_pad = torch.cat([x, torch.zeros(1, k, dtype=torch.bfloat16, device=DEV)])            # row t: all zero
    remapped = torch.where((src >= 0) & (src < t), src, torch.tensor(t, dtype=torch.int32)).to(DEV)
    clean = torch.where((src >= 0) & (src < t), src, torch.tensor(0, dtype=torch.int32)).to(DEV)
    good = np.ones(m, dtype=bool)
    good[bad_at.numpy()] = False
    for method in ("quest", "abs_max"):
        fused = _fused(q, fmt, x, h, src.to(DEV), method, gs)
        torch.cuda.synchronize()
        want = _plain(q, fmt, x_pad.index_select(0, remapped), h, method, gs)
        _assert_same_bytes(fmt, fused, want, m * k, (fmt, rot, method))                    # the bad rows: a zero row's bytes; the others as composed
        other = _fused(q, fmt, x, h, clean, method, gs)                                    # every other row is unchanged by its neighbours' bad indices
        assert np.array_equal(_np(fused[0])[good], _np(other[0])[good])
        n, spr = m * k // GS[fmt], k // GS[fmt]
        assert np.array_equal(_np(fused[1]).reshape(-1)[:n].reshape(m, spr)[good], _np(other[1]).reshape(-1)[:n].reshape(m, spr)[good])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 4. exact arithmetic against the pinned oracle: integer-valued x in -2 .. 2 times 100, Hadamard rotation -- every product and sum is exact, the tolerance is zero
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rot", CASES)
def test_exact_arithmetic_case_is_bit_equal_to_the_oracle(q, fmt, rot):
    t, m, k = 37, 53, 3 * max(rot, 32)
    gen = torch.Generator(device="cpu").manual_seed(5 + rot)
    x = (torch.randint(-2, 3, (t, k), generator=gen).float() * 100.0).to(torch.bfloat16)   # exact in bf16
    src = torch.randint(0, t, (m,), generator=gen, dtype=torch.int32)
    xg_bits = _np(x)[src.numpy()]
    h = _hadamard(rot)
    for method, om in (("quest", oracle.QUEST), ("abs_max", oracle.ABS_MAX)):
        if fmt == "mx":
            codes, sf = q.fusedGatherQuantizeMx(x.to(DEV), h, src.to(DEV), method=method)
            rq, rs, _ = oracle.fused_quantize_mx(xg_bits, _np(h), om, acc_model=1)
        else:
            codes, sf = q.fusedGatherQuantizeNv(x.to(DEV), h, torch.tensor([2.0], device=DEV), src.to(DEV), method=method)
            rq, rs = oracle.fused_quantize_nv(xg_bits, _np(h), 2.0, om, acc_model=1)
        assert np.array_equal(_np(sf).reshape(-1)[: rs.size], rs), (fmt, rot, method)
        assert oracle.codes_equal_mod_zero_sign(_np(codes).reshape(-1), rq).all(), (fmt, rot, method)


# ------------------------------------------------------------------------------------------------
# 5. padding contract: bytes past M * K / gs keep the caller's value
# ------------------------------------------------------------------------------------------------
def test_padding_contract(q):
    t, k, m = 5, 96, 3
    gen = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(t, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.tensor([4, 0, 4], dtype=torch.int32, device=DEV)
    h = _hadamard(32)
    gs = torch.tensor([3.0], device=DEV)
    amd = torch.ops.qutlass_amd
    for nv, gsz, dt in ((False, 32, torch.float8_e8m0fnu), (True, 16, torch.float8_e4m3fn)):
        codes = torch.empty(m, k // 2, dtype=torch.uint8, device=DEV)
        sf = torch.full((128, 8 if nv else 4), 0x5A, dtype=torch.uint8, device=DEV).view(dt)
        if nv:
            amd.fusedGatherQuantizeNv_(x, h, src, codes, sf, gs, 1)
        else:
            amd.fusedGatherQuantizeMx_(x, h, src, codes, sf, 1)
        torch.cuda.synchronize()
        flat = _np(sf).reshape(-1)
        n = m * k // gsz
        assert (flat[n:] == 0x5A).all(), (nv, int((flat[n:] != 0x5A).sum()))
        xg = x.index_select(0, src)
        want = q.fusedQuantizeNv(xg, h, gs, method="abs_max") if nv else q.fusedQuantizeMx(xg, h, method="abs_max")
        assert np.array_equal(flat[:n], _np(want[1]).reshape(-1)[:n]) and np.array_equal(_np(codes), _np(want[0]))


# ------------------------------------------------------------------------------------------------
# 6. moe_combine is bit-equal to its definition in numpy.float32: an explicit loop over k, a separate multiply and add, then bf16 RNE
# ------------------------------------------------------------------------------------------------
def _bf16_rne(a: np.ndarray) -> np.ndarray:
    """finite fp32 -> bf16 bits, round to nearest even"""
    u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _combine_ref(y_bits: np.ndarray, pos: np.ndarray, w: np.ndarray) -> np.ndarray:
    yf = (y_bits.astype(np.uint32) << 16).view(np.float32)
    m = yf.shape[0]
    acc = np.zeros((pos.shape[0], yf.shape[1]), dtype=np.float32)                          # +0.0f
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(pos.shape[1]):                                                      # in this order
            p = pos[:, k].astype(np.int64)
            ok = (p >= 0) & (p < m)
            prod = np.multiply(w[:, k:k + 1].astype(np.float32), yf[np.where(ok, p, 0)], dtype=np.float32)   # fmul_rn
            acc = np.where(ok[:, None], np.add(acc, prod, dtype=np.float32), acc)                             # fadd_rn; a skipped slot leaves acc alone
    return _bf16_rne(acc)


def _combine_case(t, hd, topk, seed, spare=5):
    """y ~ N(0, 1) in bf16 and |w| in {0} U [2^-6, 2): every product and sum is 0 or far inside fp32's normal range.  pos: a random injection into [1, M) -- row 0 is
    never named -- with about a quarter of the slots -1"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    m = t * topk + spare
    y = torch.randn(m, hd, generator=gen).to(torch.bfloat16)
    w = (torch.rand(t, topk, generator=gen) * 1.9 + 0.02) * torch.where(torch.rand(t, topk, generator=gen) < 0.3, -1.0, 1.0)
    special = torch.tensor([0.0, 1.0, -1.0, -0.0, 0.5])
    pick = torch.rand(t, topk, generator=gen) < 0.3
    w = torch.where(pick, special[torch.randint(0, 5, (t, topk), generator=gen)], w).float()
    pos = (torch.randperm(m - 1, generator=gen)[: t * topk] + 1).view(t, topk).to(torch.int32)
    pos = torch.where(torch.rand(t, topk, generator=gen) < 0.25, torch.tensor(-1, dtype=torch.int32), pos)
    return y, pos, w


@pytest.mark.parametrize("t", [1, 33])
@pytest.mark.parametrize("hd", [8, 104, 4096])
@pytest.mark.parametrize("topk", [1, 2, 8])
def test_moe_combine_is_bit_equal_to_the_definition(q, t, hd, topk):
    y, pos, w = _combine_case(t, hd, topk, seed=t * 1009 + hd * 13 + topk)
    out = q.moe_combine(y.to(DEV), pos.to(DEV), w.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (t, hd) and out.dtype == torch.bfloat16
    want = _combine_ref(_np(y), pos.numpy(), w.numpy())
    assert np.array_equal(_np(out), want), (int((_np(out) != want).sum()), want.size)


# ------------------------------------------------------------------------------------------------
# 7. unreferenced rows do not leak
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [104, 1024])
def test_unreferenced_rows_do_not_leak(q, hd):
    t, topk = 33, 4
    y, pos, w = _combine_case(t, hd, topk, seed=77 + hd, spare=9)
    m = y.size(0)
    pos[3] = -1                                                                            # a token whose slots are all dropped
    pos[7] = torch.tensor([m, I32_MAX, I32_MIN, -2], dtype=torch.int32)                    # every kind of out-of-range slot
    used = np.zeros(m, dtype=bool)
    p = pos.numpy().reshape(-1)
    used[p[(p >= 0) & (p < m)]] = True
    assert not used[0] and (~used).sum() >= 9
    bits = _np(y).copy()
    pat = np.array([0x7fc0, 0xffc0, 0x7f80, 0xff80, 0x7fff], dtype=np.uint16)              # NaNs of both signs, +-inf
    gen = torch.Generator(device="cpu").manual_seed(hd)
    bits[~used] = pat[torch.randint(0, 5, (int((~used).sum()), hd), generator=gen).numpy()]
    y_bad = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    zeroed = bits.copy()
    zeroed[~used] = 0
    y_zero = torch.from_numpy(zeroed.view(np.int16)).view(torch.bfloat16)
    out = q.moe_combine(y_bad.to(DEV), pos.to(DEV), w.to(DEV))
    out_zero = q.moe_combine(y_zero.to(DEV), pos.to(DEV), w.to(DEV))
    torch.cuda.synchronize()
    assert np.isfinite(out.float().cpu().numpy()).all()
    assert np.array_equal(_np(out), _np(out_zero))
    assert np.array_equal(_np(out), _combine_ref(zeroed, pos.numpy(), w.numpy()))
    assert (_np(out)[3] == 0).all() and (_np(out)[7] == 0).all()                           # +0, not -0


# ------------------------------------------------------------------------------------------------
# 8. graph capture: gather-quantize followed by moe_combine in one linear graph on a single stream
# ------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bytes(q):
    t, k, m = 33, 384, 70
    gen = torch.Generator(device="cpu").manual_seed(21)
    x = (torch.randn(t, k, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    src = torch.randint(-1, t, (m,), generator=gen, dtype=torch.int32).to(DEV)
    h = _hadamard(32)
    y, pos, w = (a.to(DEV) for a in _combine_case(t, 256, 2, seed=22))
    eager_q = q.fusedGatherQuantizeMx(x, h, src, method="abs_max")
    eager_c = q.moe_combine(y, pos, w)
    torch.cuda.synchronize()
    n = m * k // 32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        q.fusedGatherQuantizeMx(x, h, src, method="abs_max")
        q.moe_combine(y, pos, w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_q = q.fusedGatherQuantizeMx(x, h, src, method="abs_max")
        cap_c = q.moe_combine(y, pos, w)
    for _ in range(2):
        cap_q[0].zero_()
        cap_q[1].view(torch.uint8).zero_()
        cap_c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(cap_q[0]), _np(eager_q[0]))
        assert np.array_equal(_np(cap_q[1]).reshape(-1)[:n], _np(eager_q[1]).reshape(-1)[:n])
        assert np.array_equal(_np(cap_c), _np(eager_c))


# ------------------------------------------------------------------------------------------------
# 9. a whole mixture-of-experts layer: (T, H) tokens + router output -> (T, H) results
# ------------------------------------------------------------------------------------------------
def test_moe_layer_end_to_end_is_bit_equal_to_the_composition(q):
    T, E, topk, H, I, R = 35, 4, 2, 256, 128, 32
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(8)
    tok = torch.randn(T, H, generator=gen).to(torch.bfloat16).to(DEV)
    w13 = torch.randn(E, 2 * I, H, generator=gen).to(torch.bfloat16).to(DEV)
    w2 = torch.randn(E, H, I, generator=gen).to(torch.bfloat16).to(DEV)
    alpha = torch.ones(1, device=DEV)
    ids = torch.tensor([0, 1, 3])[torch.randint(0, 3, (T, topk), generator=gen)]           # expert 2 stays empty
    ids[4, 1], ids[11, 0], ids[20, 1], ids[34, 0] = -1, E, -1, E + 3                       # a few dropped ids
    topk_w = torch.softmax(torch.randn(T, topk, generator=gen), dim=-1).float()

    def quant_w(w):   # (E, N, K) -> codes (E, N, K/2), row-major scales (E * N * K / 32)
        c, s = q.fusedQuantizeMx(w.view(-1, w.size(-1)), h, method="abs_max")
        return c.view(w.size(0), w.size(1), -1), s.view(torch.uint8).reshape(-1)[: w.numel() // 32].clone().view(torch.float8_e8m0fnu)

    w13q, w13s = quant_w(w13)
    w2q, w2s = quant_w(w2)
    src_row, offs, pos = q.moe_sort(ids.to(DEV), E)
    assert int(offs[-1]) == T * topk - 4 and int(offs[2]) == int(offs[1])

    def experts(aq, asf):
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)          # (T * topk, 2 I) bf16
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
        return q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs)               # (T * topk, H) bf16; the dropped rows are never written

    out = q.moe_combine(experts(*q.fusedGatherQuantizeMx(tok, h, src_row, method="abs_max")), pos, topk_w.to(DEV))
    y_ref = experts(*q.fusedQuantizeMx(tok.index_select(0, src_row.long()), h, method="abs_max"))
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    kept = int(offs[-1])
    y_bits = _np(y_ref).copy()
    y_bits[kept:] = 0x7fc0                                                                 # whatever the unwritten rows hold must not matter
    want = _combine_ref(y_bits, _np(pos), topk_w.numpy())
    assert np.array_equal(_np(out), want), int((_np(out) != want).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0
