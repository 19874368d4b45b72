"""gpt-oss ops on the GPU: swiglu_oai_and_mul against the numpy model (tests/_swiglu_oai_model.py; tests/test_swiglu_oai_cpu.py shows that the model is a valid
judge) bit for bit over every gate the contract specifies, its accuracy against torch's bf16 composition, the per-expert bias against torch's own bf16 add,
malformed offs, fusedSwigluOaiQuantizeMx against the two-call composition byte for byte, graph capture, and a gpt-oss-shaped layer end to end."""
import numpy as np
import pytest
import torch

import _swiglu_oai_model as model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UPS = [1.0, -1.0, 0.75, -3.0, 2.5, 1e-3, 117.0, -0.0]   # 117 exercises the clamp


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


def _bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16)).view(torch.bfloat16).to(DEV)


def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return (h * n ** -0.5).to(torch.bfloat16).to(DEV)


def _offs_patterns(M):
    """(name, E, counts): the groups' row counts (tests/test_gpu_moe_grouped_scales.py's patterns): boundaries at rows 31 / 32 / 33, empty groups, E = 65 and 1024,
    and a tail past offs[E - 1], which belongs to expert E - 1"""
    def counts(E, owners, total):
        c = np.zeros(E, dtype=np.int64)
        for i in range(total):
            c[owners[i % len(owners)]] += 1
        return c

    e3 = np.diff([0, min(31, M), min(32, M), min(33, M)])
    e5 = np.array([M - 1 - (M - 1) // 3, 0, 1, 0, (M - 1) // 3])
    return [("E1", 1, np.array([M])), ("E3", 3, e3), ("E5", 5, e5), ("E65", 65, counts(65, list(range(64, -1, -1)) if M < 65 else list(range(65)), M)),
            ("E1024", 1024, counts(1024, [517, 3, 1023], M)), ("E5tail", 5, counts(5, [0, 2, 3], M - min(7, M - 1)))]


def _offs(counts):
    return torch.tensor(np.cumsum(counts), dtype=torch.int32, device=DEV)


def _experts(offs, M):
    """g(r) for rows 0 .. M - 1, by torch"""
    return torch.searchsorted(offs.to(torch.int64), torch.arange(M, device=DEV), right=True).clamp(max=offs.numel() - 1)


def _bias(E, width, gen, scale=1.0):
    """pairwise different rows (checked): a wrong expert changes bytes"""
    b = (torch.randn(E, width, generator=gen) * scale).to(torch.bfloat16)
    assert len({r.numpy().tobytes() for r in b.view(torch.int16)}) == E
    return b.to(DEV)


# ------------------------------------------------------------------------------------------------
# 1. every gate of the contract, bit for bit against the model
# ------------------------------------------------------------------------------------------------
def _gates_times_ups(gates: np.ndarray, ups_bits: np.ndarray, inter=1024) -> np.ndarray:
    """(n, 2 I) bits: every gate against every up, zero padded to whole rows"""
    g = np.repeat(gates, len(ups_bits))
    u = np.tile(ups_bits, len(gates))
    rows = -(-g.size // inter)
    x = np.zeros((rows, 2 * inter), dtype=np.uint16)
    x[:, :inter].reshape(-1)[: g.size] = g
    x[:, inter:].reshape(-1)[: u.size] = u
    return x


@pytest.mark.parametrize("alpha", [1.702, 1.0])
def test_every_specified_gate_is_bit_equal_to_the_model(q, alpha):
    gates = model.finite_gates()
    assert gates.size == 63490
    ups = _np(torch.tensor(UPS).to(torch.bfloat16))
    x = _gates_times_ups(gates, ups)
    got = _np(q.swiglu_oai_and_mul(_bf16(x), alpha=alpha, limit=7.0))
    want = model.swiglu_oai(x, alpha, 7.0)
    bad = np.nonzero(got != want)
    print(f"alpha {alpha}: {bad[0].size} of {got.size} differ")
    assert bad[0].size == 0, [(hex(x[r, c]), hex(x[r, 1024 + c]), hex(got[r, c]), hex(want[r, c])) for r, c in zip(bad[0][:8], bad[1][:8])]


@pytest.mark.parametrize("alpha", [1.702, 1.0])
def test_tiny_gates_are_within_one_bf16_step(q, alpha):
    """0 < |g| < 2^-120: the true s lies next to a tie between bf16 subnormals; with up = 0 the result is s itself"""
    gates = model.tiny_gates()
    assert gates.size == 65536 - 63490 - 256
    x = _gates_times_ups(gates, np.zeros(1, dtype=np.uint16))
    got = _np(q.swiglu_oai_and_mul(_bf16(x), alpha=alpha, limit=7.0))
    want = model.swiglu_oai(x, alpha, 7.0)
    d = np.abs(model.bf16_line(got) - model.bf16_line(want))
    print(f"alpha {alpha}: tiny gates, max distance {int(d.max())} bf16 steps, {int((d != 0).sum())} differ")
    assert int(d.max()) <= 1


@pytest.mark.parametrize("alpha", [1.702, 1.0])
def test_spot_values(q, alpha):
    ups = torch.tensor(UPS).to(torch.bfloat16)
    g = torch.tensor([100.0, -128.0, 0.0, 7.0]).repeat_interleave(len(UPS)).to(torch.bfloat16)
    x = torch.cat([g.view(1, -1), ups.repeat(4).view(1, -1)], dim=1).to(DEV)
    got = _np(q.swiglu_oai_and_mul(x, alpha=alpha))
    want = model.swiglu_oai(_np(x), alpha, 7.0)
    assert np.array_equal(got, want)
    n = len(UPS)
    up1 = (ups.float().clamp(-7, 7) + 1.0)
    assert np.array_equal(got[0, :n], _np((7.0 * up1).to(torch.bfloat16)))          # g = 100: gc = 7, s = 7 in bf16
    assert ((got[0, n:2 * n] & 0x7fff) == 0).all() and np.array_equal(got[0, n:2 * n], want[0, n:2 * n])   # a large negative gate: a zero, of the model's sign
    assert ((got[0, 2 * n:3 * n] & 0x7fff) == 0).all()
    zero = torch.zeros(3, 64, dtype=torch.bfloat16, device=DEV)
    assert (_np(q.swiglu_oai_and_mul(zero, alpha=alpha)) == 0).all()                                      # all-zero input: +0
    b0 = torch.zeros(1, 64, dtype=torch.bfloat16, device=DEV)
    assert (_np(q.swiglu_oai_and_mul(zero, alpha=alpha, bias=b0)) == 0).all()                             # and with a zero bias


# ------------------------------------------------------------------------------------------------
# 2. random inputs: the model bit for bit, and closer to the exact function than torch's bf16 composition
# ------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("inter", [8, 104, 4096])
def test_random_inputs_vs_model_and_vs_torch_composition(q, rows, inter):
    alpha, lim = 1.702, 7.0
    x = _act_input(rows, inter, seed=rows * 10007 + inter)
    got = q.swiglu_oai_and_mul(x, alpha=alpha, limit=lim)
    assert got.shape == (rows, inter) and got.dtype == torch.bfloat16
    xb = _np(x)
    assert np.array_equal(_np(got), model.swiglu_oai(xb, alpha, lim))
    g, u = x[:, :inter], x[:, inter:]
    gc = g.clamp(max=lim)
    comp = (u.clamp(-lim, lim) + 1) * (gc * torch.sigmoid(gc * alpha))             # torch's bf16 composition, on the GPU
    exact = model.exact_f64(xb, alpha, lim)
    keep = np.abs(exact) >= 2.0 ** -100
    err = lambda t: np.abs(model.bf16_to_f64(_np(t))[keep] - exact[keep]) / np.abs(exact[keep])
    eo, et = err(got), err(comp)
    print(f"rows {rows} I {inter}: op max {eo.max():.4g} mean {eo.mean():.4g} | torch bf16 max {et.max():.4g} mean {et.mean():.4g}  ({int(keep.sum())} outputs)")
    assert eo.max() <= et.max() and eo.mean() <= et.mean()


# ------------------------------------------------------------------------------------------------
# 3. the bias: torch's bf16 add under the row's expert
# ------------------------------------------------------------------------------------------------
def _biased_input(x, bias, offs):
    """x + bias[g(rows)] as torch adds bf16 tensors"""
    return x + bias[_experts(offs, x.size(0))]


def test_bias_equals_torch_add_then_the_op(q):
    gen = torch.Generator(device="cpu").manual_seed(31)
    for M in (1, 33, 140):
        for inter in (32, 96, 160):
            x = (torch.randn(M, 2 * inter, generator=gen) * 3.0).to(torch.bfloat16).to(DEV)
            for name, E, counts in _offs_patterns(M):
                bias, offs = _bias(E, 2 * inter, gen, 2.0), _offs(counts)
                got = q.swiglu_oai_and_mul(x, bias=bias, offs=offs)
                want = q.swiglu_oai_and_mul(_biased_input(x, bias, offs))
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (M, inter, name)
                # the precondition: expert 0's bias alone does not give another group's bytes
                base = q.swiglu_oai_and_mul(x + bias[0])
                e = _experts(offs, M)
                for g in torch.unique(e[e > 0]).tolist():
                    rows = e == g
                    assert not torch.equal(base[rows].view(torch.int16), want[rows].view(torch.int16)), (M, inter, name, "bias 0 gives group", g)
                if E == 1:   # one expert: offs is optional
                    assert torch.equal(q.swiglu_oai_and_mul(x, bias=bias).view(torch.int16), want.view(torch.int16))
    xb = (torch.randn(33, 64, generator=gen) * 3.0).to(torch.bfloat16)
    bb = (torch.randn(3, 64, generator=gen) * 2.0).to(torch.bfloat16)
    got = q.swiglu_oai_and_mul(xb.to(DEV), bias=bb.to(DEV), offs=torch.tensor([5, 5, 20], dtype=torch.int32, device=DEV))
    want = model.swiglu_oai(_np(xb), 1.702, 7.0, _np(bb), np.array([5, 5, 20]))       # and the model's own bias add, once
    assert np.array_equal(_np(got), want)
    torch.cuda.synchronize()


MALFORMED = [[-5, 2 ** 31 - 1, 3], [49, 0, 0], [7, 3, 20]]


@pytest.mark.parametrize("offs", MALFORMED)
def test_malformed_offs_select_some_expert(q, offs):
    gen = torch.Generator(device="cpu").manual_seed(sum(o % 97 for o in offs))
    M, inter, E = 70, 64, 3
    x = (torch.randn(M, 2 * inter, generator=gen) * 3.0).to(torch.bfloat16).to(DEV)
    bias, o = _bias(E, 2 * inter, gen, 2.0), torch.tensor(offs, dtype=torch.int32, device=DEV)
    h = _hadamard(32)
    got = q.swiglu_oai_and_mul(x, bias=bias, offs=o).view(torch.int16)
    fc, fs = q.fusedSwigluOaiQuantizeMx(x, h, bias=bias, offs=o, method="abs_max")
    fs = fs.view(torch.uint8).reshape(-1)[: M * inter // 32].view(M, -1)
    ok_act, ok_q = torch.zeros(M, dtype=torch.bool, device=DEV), torch.zeros(M, dtype=torch.bool, device=DEV)
    for e in range(E):
        want = q.swiglu_oai_and_mul(x + bias[e])
        ok_act |= (got == want.view(torch.int16)).all(dim=1)
        wc, ws = q.fusedQuantizeMx(want, h, method="abs_max")
        ws = ws.view(torch.uint8).reshape(-1)[: M * inter // 32].view(M, -1)
        ok_q |= (fc == wc).all(dim=1) & (fs == ws).all(dim=1)
    torch.cuda.synchronize()
    assert bool(ok_act.all()) and bool(ok_q.all()), (offs, (~ok_act).nonzero().flatten().tolist(), (~ok_q).nonzero().flatten().tolist())


# ------------------------------------------------------------------------------------------------
# 4. fusion is bit-exact
# ------------------------------------------------------------------------------------------------
def _assert_fused_equals_composition(q, x, h, method, bias, offs, ctx, alpha=1.702, limit=7.0):
    fc, fs = q.fusedSwigluOaiQuantizeMx(x, h, alpha=alpha, limit=limit, bias=bias, offs=offs, method=method)
    cc, cs = q.fusedQuantizeMx(q.swiglu_oai_and_mul(x, alpha=alpha, limit=limit, bias=bias, offs=offs), h, method=method)
    n = x.numel() // 2 // 32
    assert fc.shape == cc.shape and fs.shape == cs.shape and fs.dtype == cs.dtype == torch.float8_e8m0fnu, ctx
    assert torch.equal(fc, cc), (ctx, "codes", int((fc != cc).sum()))
    a, b = fs.view(torch.uint8).reshape(-1)[:n], cs.view(torch.uint8).reshape(-1)[:n]
    assert torch.equal(a, b), (ctx, "scales", int((a != b).sum()))


@pytest.mark.parametrize("rot", [32, 64])
@pytest.mark.parametrize("method", ["quest", "abs_max"])
def test_fused_equals_composition(q, rot, method):
    h = _hadamard(rot)
    gen = torch.Generator(device="cpu").manual_seed(rot * 7 + (method == "quest"))
    shapes = [(rows, 2 * k * rot) for rows in (1, 31, 33, 70) for k in (1, 3, 5)] + [(2, 35, 2 * 3 * rot)]
    for shape in shapes:
        x = (torch.randn(*shape, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
        M = x.numel() // shape[-1]
        _assert_fused_equals_composition(q, x, h, method, None, None, (rot, method, shape, "no bias"))
        for name, E, counts in _offs_patterns(M):
            bias = _bias(E, shape[-1], gen, 2.0)
            _assert_fused_equals_composition(q, x, h, method, bias, _offs(counts), (rot, method, shape, name))
            if E == 1:
                _assert_fused_equals_composition(q, x, h, method, bias, None, (rot, method, shape, "E1 without offs"))
    x = (torch.randn(33, 2 * 3 * rot, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    _assert_fused_equals_composition(q, x, h, method, None, None, (rot, method, "alpha 1, limit 2.5"), alpha=1.0, limit=2.5)
    torch.cuda.synchronize()


def test_fused_equals_composition_second_grid_round(q):
    """9.4 M outputs: more than one pass of the capped grid, so the grid-stride loop (and the look-ahead of the expert lookup) runs a second, partial round"""
    h = _hadamard(32)
    gen = torch.Generator(device="cpu").manual_seed(32)
    x = (torch.randn(2051, 2 * 4608, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    _assert_fused_equals_composition(q, x, h, "abs_max", None, None, "no bias")
    name, E, counts = _offs_patterns(2051)[2]
    _assert_fused_equals_composition(q, x, h, "abs_max", _bias(E, 2 * 4608, gen, 2.0), _offs(counts), name)


@pytest.mark.parametrize("rot", [32, 64])
def test_scale_bytes_past_the_flat_scales_are_untouched(q, rot):
    h = _hadamard(rot)
    gen = torch.Generator(device="cpu").manual_seed(5)
    M, inter = 33, 3 * rot
    x = (torch.randn(M, 2 * inter, generator=gen) * 4.0).to(torch.bfloat16).to(DEV)
    bias, offs = _bias(3, 2 * inter, gen), torch.tensor([10, 20, 33], dtype=torch.int32, device=DEV)
    codes, sf = q.ops.alloc_quant(q.ops.QUANT_OPS["swiglu_oai_quantize_mx"], x, h)
    n = M * inter // 32
    assert sf.numel() > n
    sf.view(torch.uint8).fill_(0xAB)
    torch.ops.qutlass_amd.fusedSwigluOaiQuantizeMx_(x, h, codes, sf, 1.702, 7.0, bias, offs, 1)
    want = q.fusedSwigluOaiQuantizeMx(x, h, bias=bias, offs=offs, method="abs_max")
    flat = sf.view(torch.uint8).reshape(-1)
    assert torch.equal(codes, want[0]) and torch.equal(flat[:n], want[1].view(torch.uint8).reshape(-1)[:n])
    assert bool((flat[n:] == 0xAB).all())


# ------------------------------------------------------------------------------------------------
# 5. graph capture: offs, bias and x are read on the device
# ------------------------------------------------------------------------------------------------
def test_graph_replay_follows_offs_bias_and_x(q):
    h = _hadamard(64)
    gen = torch.Generator(device="cpu").manual_seed(77)
    M, inter, E = 70, 192, 5
    n = M * inter // 32
    cases = []
    for counts in ([70, 0, 0, 0, 0], [10, 0, 25, 5, 30], [1, 1, 1, 1, 2]):
        cases.append(((torch.randn(M, 2 * inter, generator=gen) * 4.0).to(torch.bfloat16).to(DEV), _bias(E, 2 * inter, gen, 2.0), _offs(np.array(counts))))
    eager = []
    for x, b, o in cases:
        c, s = q.fusedSwigluOaiQuantizeMx(x, h, bias=b, offs=o, method="quest")
        eager.append((c.clone(), s.view(torch.uint8).reshape(-1)[:n].clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    sx, sb, so = (t.clone() for t in cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        q.fusedSwigluOaiQuantizeMx(sx, h, bias=sb, offs=so, method="quest")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = q.fusedSwigluOaiQuantizeMx(sx, h, bias=sb, offs=so, method="quest")
    for (x, b, o), (wc, ws) in zip(cases[::-1], eager[::-1]):
        sx.copy_(x)
        sb.copy_(b)
        so.copy_(o)
        cap[0].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap[0], wc) and torch.equal(cap[1].view(torch.uint8).reshape(-1)[:n], ws)


# ------------------------------------------------------------------------------------------------
# 6. a gpt-oss-shaped layer
# ------------------------------------------------------------------------------------------------
def test_gpt_oss_layer_equals_the_torch_bias_composition(q):
    T, E, topk, H, I, R = 40, 4, 2, 128, 128, 32
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(11)
    tok = torch.randn(T, H, generator=gen).to(torch.bfloat16).to(DEV)
    w13 = (torch.randn(E, 2 * I, H, generator=gen) * 0.2).to(torch.bfloat16).to(DEV)
    w2 = (torch.randn(E, H, I, generator=gen) * 0.2).to(torch.bfloat16).to(DEV)
    b1, b2 = _bias(E, 2 * I, gen), _bias(E, H, gen)
    alpha = torch.ones(1, device=DEV)
    logits = torch.randn(T, E, generator=gen)
    logits[:, 2] = -float("inf")                                          # expert 2 is never chosen: one empty group
    logits = logits.to(DEV)

    def quant_w(w):   # (E, N, K) -> codes (E, N, K/2), row-major scales (E * N * K / 32)
        c, s = q.fusedQuantizeMx(w.view(-1, w.size(-1)), h, method="abs_max")
        return c.view(w.size(0), w.size(1), -1), s.view(torch.uint8).reshape(-1)[: w.numel() // 32].clone().view(torch.float8_e8m0fnu)

    w13q, w13s = quant_w(w13)
    w2q, w2s = quant_w(w2)
    weights, ids, src_row, offs, pos = q.moe_route(logits, topk)
    counts = np.diff(np.concatenate([[0], _np(offs)]))
    assert counts[2] == 0 and (counts[[0, 1, 3]] > 0).all() and counts.sum() == T * topk
    aq, asf = q.fusedGatherQuantizeMx(tok, h, src_row, method="abs_max")
    gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)

    def tail(bias2):
        bq, bsf = q.fusedSwigluOaiQuantizeMx(gate_up, h, bias=b1, offs=offs, method="abs_max")
        return q.moe_combine(q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs), pos, weights, bias=bias2, offs=offs)

    out = tail(b2)
    e = _experts(offs, T * topk)
    cq, csf = q.fusedQuantizeMx(q.swiglu_oai_and_mul(gate_up + b1[e]), h, method="abs_max")      # the biases added by torch, the activation by the two calls
    ref = q.moe_combine(q.grouped_matmul_mxf4_bf16_tn(cq, w2q, csf, w2s, alpha, offs) + b2[e], pos, weights)
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    assert np.array_equal(_np(out), _np(ref)), int((_np(out) != _np(ref)).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0
    # changing expert 3's down bias changes exactly the tokens routed to it
    b2x = b2.clone()
    b2x[3] += 1.0
    changed = (tail(b2x).view(torch.int16) != out.view(torch.int16)).any(dim=1)
    assert torch.equal(changed, (ids == 3).any(dim=1)) and bool(changed.any()) and not bool(changed.all())
