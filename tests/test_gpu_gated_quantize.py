"""Gated-MLP ops on the GPU: silu_and_mul against an fp64 reference, the fused quantizers fusedSiluMulQuantize{Mx,Nv}[Blocked] against the library's own two launches
(bit for bit: both call one device function for the activation) and against the pinned CPU oracle, the padding contracts of the plain quantizers, non-finite tail rows,
graph capture, and a two-GEMM mixture-of-experts MLP end to end.  The CPU half (argument checks, fake kernels) is tests/test_gated_quantize_cpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)

DEV = "cuda:0"


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


# ---- the fp64 reference of the activation (numpy; bf16 as uint16 bit patterns) -------------------------------------------------
def _bf16_to_f64(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _f64_to_bf16(v: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even from fp64 straight to bf16 (no double rounding through fp32): the 8-bit significand at v's own exponent."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape, dtype=np.uint16)
    sign = (np.signbit(v).astype(np.uint16) << 15)
    a = np.abs(v)
    fin = np.isfinite(a) & (a > 0)
    m, e = np.frexp(np.where(fin, a, 1.0))          # a = m * 2^e, m in [0.5, 1)
    e = np.maximum(e, -125)                         # below 2^-126: the subnormal quantum 2^-133
    quant = np.ldexp(1.0, e - 8)                    # 8 significand bits: ulp = 2^(e - 8)
    r = np.rint(np.where(fin, a, 0.0) / quant) * quant   # np.rint: ties to even; the division is by a power of two (exact)
    r32 = r.astype(np.float32)                      # exactly representable (or overflows to inf, as bf16 does: 2^128)
    bits = (r32.view(np.uint32) >> 16).astype(np.uint16)
    out = np.where(fin, bits, out)
    out = np.where(np.isinf(a), np.uint16(0x7f80), out)
    out = np.where(np.isnan(v), np.uint16(0x7fc0), out)
    return (out | sign).astype(np.uint16)


def _ref_act(x_bits: np.ndarray) -> np.ndarray:
    """act = bf16(bf16(g / (1 + exp(-g))) * u) in fp64, x = (.., 2 I) bf16 bits -> (.., I) bf16 bits."""
    inter = x_bits.shape[-1] // 2
    g, u = _bf16_to_f64(x_bits[..., :inter]), _bf16_to_f64(x_bits[..., inter:])
    with np.errstate(over="ignore"):
        s = _f64_to_bf16(g / (1.0 + np.exp(-g)))
    return _f64_to_bf16(_bf16_to_f64(s) * u)


def test_fp64_reference_rounding_helper():
    """(the checker's own bf16 rounding: every bf16 value round-trips, and the midpoints between neighbours go to the even one)"""
    bits = np.arange(0, 0x7f80, dtype=np.uint16)
    assert np.array_equal(_f64_to_bf16(_bf16_to_f64(bits)), bits)
    mid = (_bf16_to_f64(bits[:-1]) + _bf16_to_f64(bits[1:])) / 2
    assert np.array_equal(_f64_to_bf16(mid), np.where(bits[:-1] & 1, bits[1:], bits[:-1]))
    assert _f64_to_bf16(np.array([-0.0]))[0] == 0x8000


def _ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in bf16 steps between two finite bf16 bit patterns (sign-magnitude -> a monotone integer line; +0 and -0 coincide)"""
    def line(v):
        v = v.astype(np.int32)
        return np.where(v & 0x8000, -(v & 0x7fff), v)
    return np.abs(line(a) - line(b))


SPECIAL_G = [0.0, 0.5, -0.5, 1.0, -1.0, 8.0, -8.0, 30.0, -30.0, 100.0, -100.0]


def _act_input(rows, inter, seed):
    """g ~ N(0, 3^2), u ~ N(0, 2^2); the exact values of SPECIAL_G overwrite the head of every row's gate half, starting at a different one per row"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    g = torch.randn(rows, inter, generator=gen) * 3.0
    u = torch.randn(rows, inter, generator=gen) * 2.0
    n = min(inter, len(SPECIAL_G))
    sp = torch.tensor(SPECIAL_G)
    for r in range(rows):
        g[r, :n] = sp[(torch.arange(n) + 8 * r) % len(SPECIAL_G)]
    return torch.cat([g, u], dim=1).to(torch.bfloat16).to(DEV)


def _check_act(got: np.ndarray, want: np.ndarray, what: str):
    d = _ulp_distance(got, want)
    exact = float((d == 0).mean())
    print(f"{what}: bit-equal {exact:.5f}, max distance {int(d.max())} bf16 ulp")
    assert int(d.max()) <= 1, int(d.max())          # within one bf16 ulp, zeros of either sign alike
    assert exact >= 0.99, exact                     # single rounding / truncation would miss far more


# ------------------------------------------------------------------------------------------------
# 1. the activation against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("inter", [8, 104, 4096])
def test_silu_and_mul_vs_fp64(q, rows, inter):
    x = _act_input(rows, inter, seed=rows * 10007 + inter)
    got = q.silu_and_mul(x)
    torch.cuda.synchronize()
    assert got.shape == (rows, inter) and got.dtype == torch.bfloat16
    _check_act(_np(got), _ref_act(_np(x)), f"silu_and_mul rows={rows} I={inter}")


def test_silu_and_mul_exact_gate_values(q):
    """every value of the exact block against every up value of a small set; a large negative gate gives a zero (exp overflows to inf)"""
    ups = [1.0, -1.0, 0.75, -3.0, 2.5, 1e-3, 117.0, -0.0]
    g = torch.tensor(SPECIAL_G + [-88.0, -89.0, 88.0, 20.0, -20.0]).repeat_interleave(len(ups))       # 16 gates x 8 ups
    u = torch.tensor(ups).repeat(16)
    x = torch.cat([g.view(1, -1), u.view(1, -1)], dim=1).to(torch.bfloat16).to(DEV)
    got = _np(q.silu_and_mul(x))
    torch.cuda.synchronize()
    _check_act(got, _ref_act(_np(x)), "silu_and_mul exact gates")
    i100 = SPECIAL_G.index(-100.0) * len(ups)
    assert ((got[0, i100:i100 + len(ups)] & 0x7fff) == 0).all()
    p100 = SPECIAL_G.index(100.0) * len(ups)
    assert np.array_equal(got[0, p100:p100 + len(ups)], _np((torch.tensor(ups).to(torch.bfloat16).float() * 100.0).to(torch.bfloat16)))   # silu(100) == 100 in bf16


# ------------------------------------------------------------------------------------------------
# 2. fusion is bit-exact
# ------------------------------------------------------------------------------------------------
def _both(q, fmt, blocked, x, h, method, gs):
    """(fused, composed) outputs of one format / layout"""
    if fmt == "mx":
        fused = (q.fusedSiluMulQuantizeMxBlocked if blocked else q.fusedSiluMulQuantizeMx)(x, h, method=method)
        comp = (q.fusedQuantizeMxBlocked if blocked else q.fusedQuantizeMx)(q.silu_and_mul(x), h, method=method)
    else:
        fused = (q.fusedSiluMulQuantizeNvBlocked if blocked else q.fusedSiluMulQuantizeNv)(x, h, gs, method=method)
        comp = (q.fusedQuantizeNvBlocked if blocked else q.fusedQuantizeNv)(q.silu_and_mul(x), h, gs, method=method)
    return fused, comp


def _assert_same_bytes(fmt, blocked, fused, comp, numel, ctx):
    (fc, fs), (cc, cs) = fused, comp
    assert fc.shape == cc.shape and fs.shape == cs.shape and fs.dtype == cs.dtype, ctx
    assert np.array_equal(_np(fc), _np(cc)), (ctx, "codes", int((_np(fc) != _np(cc)).sum()))
    a, b = _np(fs).reshape(-1), _np(cs).reshape(-1)
    if not blocked:   # flat: the first numel / gs bytes are the scales, the rest of the buffer belongs to the caller
        n = numel // (32 if fmt == "mx" else 16)
        a, b = a[:n], b[:n]
    assert np.array_equal(a, b), (ctx, "scales", int((a != b).sum()))


CASES = [("mx", r) for r in (32, 64, 128)] + [("nv", r) for r in (16, 32, 64, 128)]


@pytest.mark.parametrize("fmt,rot", CASES)
@pytest.mark.parametrize("method", ["quest", "abs_max"])
def test_fused_equals_composition(q, fmt, rot, method):
    h = _hadamard(rot)
    gs = torch.tensor([3.0], device=DEV)
    rp = max(rot, 32)
    gen = torch.Generator(device="cpu").manual_seed(rot * 7 + (method == "quest"))
    shapes = [(rows, 2 * k * rp) for rows in (1, 31, 33, 70) for k in (1, 3, 5)] + [(2, 35, 2 * 3 * rp)]
    for shape in shapes:
        x = (torch.randn(*shape, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
        for blocked in (False, True):
            fused, comp = _both(q, fmt, blocked, x, h, method, gs)
            _assert_same_bytes(fmt, blocked, fused, comp, x.numel() // 2, (fmt, rot, method, shape, blocked))
    torch.cuda.synchronize()


@pytest.mark.parametrize("rot", [32, 128])
def test_fused_equals_composition_second_grid_round(q, rot):
    """9.4 M outputs: more than one pass of the capped grid (8.4 M elements), so the grid-stride loop runs a second, partial round"""
    h = _hadamard(rot)
    gen = torch.Generator(device="cpu").manual_seed(rot)
    x = (torch.randn(2051, 2 * 4608, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    for blocked in (False, True):
        fused, comp = _both(q, "mx", blocked, x, h, "abs_max", None)
        _assert_same_bytes("mx", blocked, fused, comp, x.numel() // 2, (rot, blocked))


# ------------------------------------------------------------------------------------------------
# 3. against the CPU oracle (act from the fp64 reference)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rot", [("mx", 32), ("nv", 16)])
@pytest.mark.parametrize("method", ["quest", "abs_max"])
def test_fused_vs_oracle(q, fmt, rot, method):
    """Bounds of the plain quantizers' oracle tests (MX: every scale byte equal, codes differ in <= 1e-4 of the elements, __graft_entry__.smoke / tests/test_gpu_parity.py;
    NV: <= 2e-4 of the scale bytes from the reciprocal / MFMA summation order, codes <= 1e-4 of the elements where the scale agrees), over the rotation groups whose
    activation is bit-equal to the fp64 reference; the others (a mis-rounded bf16, test 1: under 1 % of the values) are counted and bounded instead."""
    rows, inter = 70, 384
    x = _act_input(rows, inter, seed=99 + rot)
    h = _hadamard(rot)
    om = oracle.QUEST if method == "quest" else oracle.ABS_MAX
    act_ref = _ref_act(_np(x))
    act_got = _np(q.silu_and_mul(x))
    clean_run = (act_ref == act_got).reshape(-1, rot).all(axis=1)          # rotation runs the device fed exactly the reference's values
    print(f"{fmt} R={rot} {method}: {int((~clean_run).sum())} of {clean_run.size} rotation runs hold a mis-rounded activation")
    assert (~clean_run).mean() <= rot * 2.0 ** -9                              # R values per run, two roundings per value, each mis-rounded with probability of order 2^-10
    if fmt == "mx":
        codes, sf = q.fusedSiluMulQuantizeMx(x, h, method=method)
        rq, rs, _ = oracle.fused_quantize_mx(act_ref, _np(h), om, acc_model=1)
        gsz = 32
    else:
        codes, sf = q.fusedSiluMulQuantizeNv(x, h, torch.tensor([3.0], device=DEV), method=method)
        rq, rs = oracle.fused_quantize_nv(act_ref, _np(h), 3.0, om, acc_model=1)
        gsz = 16
    torch.cuda.synchronize()
    got_s = _np(sf).reshape(-1)[: rs.size]
    clean_grp = np.repeat(clean_run, rot // gsz) if rot >= gsz else clean_run.reshape(-1, gsz // rot).all(axis=1)
    clean_el = np.repeat(clean_grp, gsz)
    sbad = int(((got_s != rs) & clean_grp).sum())
    eq = oracle.codes_equal_mod_zero_sign(_np(codes).reshape(-1), rq)
    if fmt == "mx":
        cbad = int((~eq & clean_el).sum())
        print(f"  scale bytes differing: {sbad}; codes differing: {cbad} of {eq.size}")
        assert sbad == 0, sbad
    else:
        same = np.repeat(got_s == rs, gsz)
        cbad = int((~eq & clean_el & same).sum())
        print(f"  scale bytes differing: {sbad} of {rs.size}; codes differing under equal scales: {cbad} of {eq.size}")
        assert sbad <= 2e-4 * rs.size, sbad
    assert cbad <= 1e-4 * eq.size, cbad


# ------------------------------------------------------------------------------------------------
# 4. exact arithmetic: gate = +100 (silu(100) == 100 in bf16), small integer up, Hadamard rotation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rot", CASES)
def test_exact_arithmetic_case_is_bit_equal_to_the_oracle(q, fmt, rot):
    rows, inter = 37, 3 * max(rot, 32)
    gen = torch.Generator(device="cpu").manual_seed(5 + rot)
    u = torch.randint(-2, 3, (rows, inter), generator=gen).float()
    x = torch.cat([torch.full((rows, inter), 100.0), u], dim=1).to(torch.bfloat16).to(DEV)
    act = (u * 100.0).to(torch.bfloat16)                       # 100 * {-2 .. 2}: exact in bf16
    assert np.array_equal(_np(q.silu_and_mul(x)), _np(act)) and np.array_equal(_ref_act(_np(x)), _np(act))
    h = _hadamard(rot)
    for method, om in (("quest", oracle.QUEST), ("abs_max", oracle.ABS_MAX)):
        if fmt == "mx":
            codes, sf = q.fusedSiluMulQuantizeMx(x, h, method=method)
            rq, rs, _ = oracle.fused_quantize_mx(_np(act), _np(h), om, acc_model=1)
        else:
            codes, sf = q.fusedSiluMulQuantizeNv(x, h, torch.tensor([2.0], device=DEV), method=method)
            rq, rs = oracle.fused_quantize_nv(_np(act), _np(h), 2.0, om, acc_model=1)
        assert np.array_equal(_np(sf).reshape(-1)[: rs.size], rs), (fmt, rot, method)
        assert oracle.codes_equal_mod_zero_sign(_np(codes).reshape(-1), rq).all(), (fmt, rot, method)


# ------------------------------------------------------------------------------------------------
# 5. padding contracts
# ------------------------------------------------------------------------------------------------
def test_padding_contracts(q):
    rows, inter = 3, 96
    x = _act_input(rows, inter, seed=3)
    h = _hadamard(32)
    gs = torch.tensor([3.0], device=DEV)
    amd = torch.ops.qutlass_amd
    # flat: bytes past numel / gs keep the caller's 0x5A
    for nv, gsz, dt in ((False, 32, torch.float8_e8m0fnu), (True, 16, torch.float8_e4m3fn)):
        codes = torch.empty(rows, inter // 2, dtype=torch.uint8, device=DEV)
        sf = torch.full((128, 4 if not nv else 8), 0x5A, dtype=torch.uint8, device=DEV).view(dt)
        if nv:
            amd.fusedSiluMulQuantizeNv_(x, h, codes, sf, gs, 1, False)
        else:
            amd.fusedSiluMulQuantizeMx_(x, h, codes, sf, 1, False)
        torch.cuda.synchronize()
        flat = _np(sf).reshape(-1)
        n = rows * inter // gsz
        assert (flat[n:] == 0x5A).all(), (nv, int((flat[n:] != 0x5A).sum()))
        want = (q.fusedQuantizeNv(q.silu_and_mul(x), h, gs, method="abs_max") if nv else q.fusedQuantizeMx(q.silu_and_mul(x), h, method="abs_max"))[1]
        assert np.array_equal(flat[:n], _np(want).reshape(-1)[:n])
    # blocked: the padding of the (128, 4) / (128, 8) layout is zero-filled over whatever the buffer held
    for nv, cols, dt in ((False, 3, torch.float8_e8m0fnu), (True, 6, torch.float8_e4m3fn)):
        pc = (cols + 3) // 4 * 4
        codes = torch.empty(rows, inter // 2, dtype=torch.uint8, device=DEV)
        sf = torch.full((128 * pc,), 0x5A, dtype=torch.uint8, device=DEV).view(dt)
        if nv:
            amd.fusedSiluMulQuantizeNv_(x, h, codes, sf, gs, 1, True)
        else:
            amd.fusedSiluMulQuantizeMx_(x, h, codes, sf, 1, True)
        torch.cuda.synchronize()
        flat_scales = (q.fusedSiluMulQuantizeNv(x, h, gs) if nv else q.fusedSiluMulQuantizeMx(x, h, method="abs_max"))[1]
        mat = np.zeros((rows, cols), dtype=np.uint8)
        mat[:] = _np(flat_scales).reshape(-1)[: rows * cols].reshape(rows, cols)
        assert np.array_equal(_np(sf).reshape(-1), oracle.to_blocked(mat).reshape(-1)), nv


# ------------------------------------------------------------------------------------------------
# 6. non-finite tail rows (the unwritten tail of a grouped GEMM's output) stay in their own rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,rot", [("mx", 32), ("mx", 128), ("nv", 16), ("nv", 64)])
def test_non_finite_tail_rows_do_not_leak(q, fmt, rot):
    rows, bad, inter = 37, 5, 3 * max(rot, 32)
    gen = torch.Generator(device="cpu").manual_seed(11 + rot)
    bits = _np((torch.randn(rows, 2 * inter, generator=gen) * 4.0).to(torch.bfloat16)).copy()
    pat = np.array([0x7fc0, 0xffc0, 0x7f80, 0xff80, 0x7fff], dtype=np.uint16)                  # NaNs of both signs, +-inf
    bits[rows - bad:] = pat[torch.randint(0, 5, (bad, 2 * inter), generator=gen).numpy()]
    x = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(DEV)
    h = _hadamard(rot)
    gs = torch.tensor([3.0], device=DEV)
    good = rows - bad
    for blocked in (False, True):
        for method in ("quest", "abs_max"):
            if fmt == "mx":
                f = q.fusedSiluMulQuantizeMxBlocked if blocked else q.fusedSiluMulQuantizeMx
                full, head = f(x, h, method=method), f(x[:good].contiguous(), h, method=method)
            else:
                f = q.fusedSiluMulQuantizeNvBlocked if blocked else q.fusedSiluMulQuantizeNv
                full, head = f(x, h, gs, method=method), f(x[:good].contiguous(), h, gs, method=method)
            torch.cuda.synchronize()   # (raises if the launch faulted)
            assert np.array_equal(_np(full[0])[:good], _np(head[0])), (fmt, rot, blocked, method)
            gsz = 32 if fmt == "mx" else 16
            cols = inter // gsz
            if blocked:   # scale (r, c) of the blocked layout, rows < good
                pc = (cols + 3) // 4 * 4
                r, c = np.meshgrid(np.arange(good), np.arange(cols), indexing="ij")
                off = ((r >> 7) * (pc // 4) + (c >> 2)) * 512 + (r & 31) * 16 + ((r & 127) >> 5) * 4 + (c & 3)
                assert np.array_equal(_np(full[1]).reshape(-1)[off], _np(head[1]).reshape(-1)[off]), (fmt, rot, blocked, method)
            else:
                n = good * cols
                assert np.array_equal(_np(full[1]).reshape(-1)[:n], _np(head[1]).reshape(-1)[:n]), (fmt, rot, blocked, method)


# ------------------------------------------------------------------------------------------------
# 7. graph capture
# ------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bytes(q):
    x = _act_input(70, 384, seed=21)
    h = _hadamard(32)
    eager = q.fusedSiluMulQuantizeMx(x, h, method="abs_max")
    torch.cuda.synchronize()
    n = 70 * 384 // 32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q.fusedSiluMulQuantizeMx(x, h, method="abs_max")   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = q.fusedSiluMulQuantizeMx(x, h, method="abs_max")
    for _ in range(2):
        cap[0].zero_()
        cap[1].view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(cap[0]), _np(eager[0]))
        assert np.array_equal(_np(cap[1]).reshape(-1)[:n], _np(eager[1]).reshape(-1)[:n])


# ------------------------------------------------------------------------------------------------
# 8. a mixture-of-experts MLP end to end: grouped GEMM -> activation + quantizer -> grouped GEMM
# ------------------------------------------------------------------------------------------------
def test_moe_mlp_end_to_end_is_bit_equal_to_the_composition(q):
    E, H, I, R = 3, 256, 128, 32
    groups = (0, 37, 33)
    M = sum(groups)
    offs = torch.tensor(np.cumsum(groups), dtype=torch.int32, device=DEV)
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(8)
    tok = torch.randn(M, H, generator=gen).to(torch.bfloat16).to(DEV)
    w13 = torch.randn(E, 2 * I, H, generator=gen).to(torch.bfloat16).to(DEV)
    w2 = torch.randn(E, H, I, generator=gen).to(torch.bfloat16).to(DEV)
    alpha = torch.ones(1, device=DEV)

    def quant_w(w):   # (E, N, K) -> codes (E, N, K/2), row-major scales (E * N * K / 32)
        c, s = q.fusedQuantizeMx(w.view(-1, w.size(-1)), h, method="abs_max")
        return c.view(w.size(0), w.size(1), -1), s.view(torch.uint8).reshape(-1)[: w.numel() // 32].clone().view(torch.float8_e8m0fnu)

    w13q, w13s = quant_w(w13)
    w2q, w2s = quant_w(w2)
    tq, ts = q.fusedQuantizeMx(tok, h, method="abs_max")
    gate_up = q.grouped_matmul_mxf4_bf16_tn(tq, w13q, ts, w13s, alpha, offs)           # (M, 2 I) bf16
    assert gate_up.shape == (M, 2 * I)
    a_f, s_f = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
    y_f = q.grouped_matmul_mxf4_bf16_tn(a_f, w2q, s_f, w2s, alpha, offs)
    a_c, s_c = q.fusedQuantizeMx(q.silu_and_mul(gate_up), h, method="abs_max")
    y_c = q.grouped_matmul_mxf4_bf16_tn(a_c, w2q, s_c, w2s, alpha, offs)
    torch.cuda.synchronize()
    assert y_f.shape == (M, H)
    assert np.array_equal(_np(y_f), _np(y_c))
    assert np.isfinite(_np(y_f.float())).all() and float(y_f.float().abs().max()) > 0
