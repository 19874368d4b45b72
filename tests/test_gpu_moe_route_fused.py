"""The one-launch routing on the GPU: moe_route_fused / moe_route_grouped_fused against the two-launch ops they must equal bit for bit (through the Python wrappers, on
both sides of the measured bound), the always-one-launch C entries against numpy at the shapes where one workgroup routing AND sorting can go wrong, expert_map,
non-finite rows inside the one workgroup, T = 0, graph capture, the write and read footprint, and a whole layer.  Every comparison is exact: no tolerance anywhere.
The numpy checkers are those of tests/test_gpu_moe_route.py and tests/test_moe_route_grouped_cpu.py.  The CPU half is tests/test_moe_route_fused_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _footprint as fp  # noqa: E402
from test_gpu_moe_route import _f64, _hadamard, _logits, _np, _sort_ref  # noqa: E402
from test_moe_route_grouped_cpu import grouped_topk_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32, F32, BF16 = torch.int32, torch.float32, torch.bfloat16
NAMES = ("weights", "ids", "src_row", "offs", "pos")
# moe_route_grouped's own test parameters: (E, n_group, topk_group, topk, scoring, bias, routed_scaling_factor)
GROUPED = {"deepseek_v3": (256, 8, 4, 8, "sigmoid", True, 2.5), "kimi_k2": (384, 1, 1, 8, "sigmoid", True, 2.827), "deepseek_v2": (160, 8, 3, 6, "softmax", False, 1.0)}


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _bound(q):
    b = q._lib.load().qutlass_amd_moe_route_fused_max_tokens()
    assert 0 <= b <= 64
    return b


def _tokens(q):
    b = _bound(q)
    return sorted({t for t in (1, 2, 7, 8, 9, b, b + 1, 64, 65, 200) if t > 0})


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _assert_same(got, want, ctx):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, name, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(_bits(g), _bits(w)), (ctx, name, int((_bits(g) != _bits(w)).sum()))


def _grouped_kw(cfg, seed=0):
    E, G, tg, topk, scoring, with_bias, scale = cfg
    bias = None
    if with_bias:   # a coarse grid, as tests/test_gpu_moe_route_grouped.py: exact ties in the choice values and the group scores
        bias = (torch.randint(-3, 4, (E,), generator=torch.Generator(device="cpu").manual_seed(E + seed)).float() / 8.0).to(DEV)
    return dict(n_group=G, topk_group=tg, bias=bias, scoring=scoring, routed_scaling_factor=scale)


def _mapped(flat, emap):
    """moe_sort_key's rule in numpy: an id outside [0, G) is dropped without reading the map"""
    G = emap.size
    return np.where((flat >= 0) & (flat < G), emap[np.clip(flat, 0, G - 1)], -1).astype(np.int64)


def _check_sort_numpy(res, num_experts, ctx, emap=None):
    """src_row, offs and pos of the five results against the _sort_ref rule on the ids they came with"""
    ids = res[1].cpu().numpy().astype(np.int64)
    flat = ids.reshape(-1) if emap is None else _mapped(ids.reshape(-1), emap)
    for name, g, w in zip(NAMES[2:], res[2:], _sort_ref(flat, num_experts, ids.shape[1])):
        g = g.cpu().numpy().reshape(-1)
        assert np.array_equal(g, w), (ctx, name, int((g != w).sum()))


# ------------------------------------------------------------------------------------------------
# 1. bit equality with the two-launch ops through the Python wrappers, below and above the bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("E", [1, 8, 60, 129, 1024])
def test_softmax_router_equals_moe_route(q, E, dtype):
    for topk in sorted({k for k in (1, 2, 8, 32) if k <= min(E, 32)}):
        for T in _tokens(q):
            x = _logits(T, E, dtype, topk, seed=E * 1000 + topk * 10 + T).to(DEV)
            for renorm in (True, False):
                _assert_same(q.moe_route_fused(x, topk, renormalize=renorm), q.moe_route(x, topk, renormalize=renorm), (E, topk, T, renorm))


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", list(GROUPED))
def test_grouped_router_equals_moe_route_grouped(q, shape, dtype):
    cfg = GROUPED[shape]
    E, topk = cfg[0], cfg[3]
    kw = _grouped_kw(cfg)
    for T in _tokens(q):
        x = _logits(T, E, dtype, topk, seed=E + T).to(DEV)
        for renorm in (True, False):
            _assert_same(q.moe_route_grouped_fused(x, topk, renormalize=renorm, **kw), q.moe_route_grouped(x, topk, renormalize=renorm, **kw), (shape, T, renorm))


# ------------------------------------------------------------------------------------------------
# 2. the C entries (always one launch) against numpy, where this kernel can go wrong and the two-launch ones cannot
# ------------------------------------------------------------------------------------------------
def _c_route(q, x, topk, num_experts=None, renorm=True, emap=None, grouped=None, ptr=None):
    """one call of qutlass_amd_moe_route_fused / _grouped_fused on results prefilled with a value no result can hold; x (T, E) on the device; ptr: the address to
    read the logits from instead of x's own"""
    lib = q._lib.load()
    T, E = x.shape
    L = E if num_experts is None else num_experts
    res = [torch.full((T, topk), float("nan"), dtype=F32, device=DEV), torch.full((T, topk), -7, dtype=I32, device=DEV), torch.full((T * topk,), -7, dtype=I32, device=DEV),
           torch.full((L,), -7, dtype=I32, device=DEV), torch.full((T, topk), -7, dtype=I32, device=DEV)]
    p = [r.data_ptr() for r in res]
    tail = (L, emap.data_ptr() if emap is not None else None, emap.numel() if emap is not None else 0, p[2], p[3], p[4], fp.stream())
    head = (ptr or x.data_ptr(), x.element_size(), T, E, topk)
    if grouped is None:
        rc = lib.qutlass_amd_moe_route_fused(*head, int(renorm), p[0], p[1], *tail)
    else:
        bias = grouped["bias"]
        rc = lib.qutlass_amd_moe_route_grouped_fused(*head, grouped["n_group"], grouped["topk_group"], q._lib.MOE_SCORING[grouped["scoring"]],
                                                     bias.data_ptr() if bias is not None else None, int(renorm), grouped["routed_scaling_factor"], p[0], p[1], *tail)
    fp.ok(lib, rc)
    torch.cuda.synchronize()
    return res


def _ties(T, E, dtype, seed):
    """rows built from three distinct logit values: ties decide the selection, and many slots share an expert"""
    return (torch.randint(-1, 2, (T, E), generator=torch.Generator(device="cpu").manual_seed(seed)).float() * 0.5).to(dtype)


SOFTMAX_C_CASES = {
    "second_trip_of_wave_0": (9, 8, 2, BF16, "randn"),          # T = 9: wave 0 routes tokens 0 and 8, waves 1-7 one each
    "2048_slots": (64, 128, 32, BF16, "randn"),                  # four chunks of 64 slots per wave
    "partial_chunk_idle_waves": (3, 8, 5, F32, "randn"),         # 15 slots: one partial chunk, seven waves without a slot
    "one_expert": (64, 1, 1, BF16, "randn"),                     # every slot in expert 0
    "1025_keys": (9, 1024, 8, BF16, "randn"),                    # three keys per thread in the scan
    "1025_keys_f32_full": (64, 1024, 32, F32, "ties"),
    "ties": (64, 128, 8, BF16, "ties"),
    "ties_E129": (33, 129, 8, F32, "ties"),
}


@pytest.mark.parametrize("case", list(SOFTMAX_C_CASES))
def test_c_entry_softmax_against_numpy(q, case):
    T, E, topk, dtype, kind = SOFTMAX_C_CASES[case]
    x = (_ties(T, E, dtype, 11) if kind == "ties" else _logits(T, E, dtype, topk, seed=T * 7 + E)).to(DEV)
    for renorm in (True, False):
        res = _c_route(q, x, topk, renorm=renorm)
        assert np.array_equal(res[1].cpu().numpy(), np.argsort(-_f64(x), axis=1, kind="stable")[:, :topk]), (case, "ids")
        _check_sort_numpy(res, E, case)
        w, ids = q.moe_topk_softmax(x, topk, renormalize=renorm)
        assert torch.equal(w.view(I32), res[0].view(I32)) and torch.equal(ids, res[1]), (case, "moe_topk_softmax")


def test_c_entry_reads_rows_off_the_16_byte_grid(q):
    """E = 60 bf16 from a base pointer offset by 2 bytes: the one-column-per-load path; the same bits as the aligned copy"""
    T, E, topk = 11, 60, 8
    buf = (torch.randn(1 + T * E, generator=torch.Generator(device="cpu").manual_seed(5)) * 3.0).to(BF16).to(DEV)
    view = buf[1:].view(T, E)
    assert view.data_ptr() % 16 == 2
    off, aligned = _c_route(q, view, topk, ptr=buf.data_ptr() + 2), _c_route(q, view.clone(), topk)
    _assert_same(off, aligned, "offset")
    assert np.array_equal(off[1].cpu().numpy(), np.argsort(-_f64(view), axis=1, kind="stable")[:, :topk])
    _check_sort_numpy(off, E, "offset")


@pytest.mark.parametrize("T,kind", [(9, "randn"), (64, "ties"), (3, "randn")])
@pytest.mark.parametrize("shape", list(GROUPED))
def test_c_entry_grouped_against_numpy(q, shape, T, kind):
    """ids from the scores moe_topk_grouped returns, by the numpy definition; weights bit-equal to moe_topk_grouped's; the sort by the _sort_ref rule"""
    cfg = GROUPED[shape]
    E, G, tg, topk, scoring, _, scale = cfg
    kw = _grouped_kw(cfg, seed=T)
    x = (_ties(T, E, BF16, T) if kind == "ties" else _logits(T, E, BF16, topk, seed=T + E)).to(DEV)
    res = _c_route(q, x, topk, grouped=kw)
    w, ids, s = q.moe_topk_grouped(x, topk, return_scores=True, **kw)
    bias_np = None if kw["bias"] is None else kw["bias"].cpu().numpy()
    want_ids, _ = grouped_topk_ref(s.cpu().numpy(), topk, n_group=G, topk_group=tg, bias=bias_np, routed_scaling_factor=scale)
    assert np.array_equal(res[1].cpu().numpy(), want_ids), (shape, T, "ids")
    assert torch.equal(w.view(I32), res[0].view(I32)) and torch.equal(ids, res[1]), (shape, T, "moe_topk_grouped")
    _check_sort_numpy(res, E, (shape, T))


# ------------------------------------------------------------------------------------------------
# 3. expert_map: -1 entries and an out-of-range value
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 64])
def test_expert_map(q, T):
    E, L, topk = 16, 8, 4
    emap_np = np.full(E, -1, dtype=np.int32)
    emap_np[8:] = np.arange(L)
    emap_np[3] = L              # an entry outside [0, L) other than -1 drops too
    emap_np[5] = 2              # two global experts on one local one
    emap = torch.from_numpy(emap_np).to(DEV)
    x = _logits(T, E, BF16, topk, seed=T).to(DEV)
    want = q.moe_route(x, topk, L, expert_map=emap)
    for got in (q.moe_route_fused(x, topk, L, expert_map=emap), _c_route(q, x, topk, num_experts=L, emap=emap)):
        _assert_same(got, want, ("softmax", T))
        _check_sort_numpy(got, L, ("softmax", T), emap=emap_np)
    assert int(want[3][-1]) < T * topk and (want[4] == -1).any()       # something was dropped
    cfg = (E, 4, 2, topk, "sigmoid", True, 2.5)
    kw = _grouped_kw(cfg)
    want = q.moe_route_grouped(x, topk, L, expert_map=emap, **kw)
    for got in (q.moe_route_grouped_fused(x, topk, L, expert_map=emap, **kw), _c_route(q, x, topk, num_experts=L, emap=emap, grouped=kw)):
        _assert_same(got, want, ("grouped", T))
        _check_sort_numpy(got, L, ("grouped", T), emap=emap_np)


# ------------------------------------------------------------------------------------------------
# 4. rows do not interact inside the one workgroup
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("router", ["softmax", "grouped"])
def test_non_finite_rows_do_not_leak(q, router):
    T, E, topk = 16, 160, 6
    kw = _grouped_kw(GROUPED["deepseek_v2"]) if router == "grouped" else None
    x = (torch.randn(T, E, generator=torch.Generator(device="cpu").manual_seed(E)) * 3.0).to(BF16)
    bad = x.clone()
    bad[2, E // 3] = float("nan")
    bad[2, 0] = float("nan")
    bad[6] = float("inf")
    bad[7] = float("-inf")
    r0, r1 = _c_route(q, x.to(DEV), topk, grouped=kw), _c_route(q, bad.to(DEV), topk, grouped=kw)
    good = [t for t in range(T) if t not in (2, 6, 7)]
    assert torch.equal(r0[0][good].view(I32), r1[0][good].view(I32)) and torch.equal(r0[1][good], r1[1][good])
    for r in (2, 6, 7):
        row = r1[1][r].cpu().numpy()
        assert len(set(row.tolist())) == topk and row.min() >= 0 and row.max() < E, (r, row)
    _check_sort_numpy(r1, E, router)      # the whole sort, the bad rows' slots included, on the ids that came back
    _check_sort_numpy(r0, E, router)


# ------------------------------------------------------------------------------------------------
# 5. T = 0
# ------------------------------------------------------------------------------------------------
def test_no_tokens(q):
    x = torch.empty(0, 8, dtype=BF16, device=DEV)
    for res in (q.moe_route_fused(x, 2), q.moe_route_grouped_fused(x, 2, n_group=2, topk_group=1)):
        assert [tuple(r.shape) for r in res] == [(0, 2), (0, 2), (0,), (8,), (0, 2)]
        assert [r.dtype for r in res] == [F32, I32, I32, I32, I32] and int(res[3].abs().sum()) == 0


def test_the_ops_reject_what_the_kernels_cannot_take(q):
    """the checks the two functional ops make themselves, each with its message, and the C entries' behind them"""
    amd = torch.ops.qutlass_amd
    x = torch.zeros(4, 8, dtype=BF16, device=DEV)
    emap, bias = torch.zeros(8, dtype=I32, device=DEV), torch.zeros(8, dtype=F32, device=DEV)
    soft = lambda **kw: amd.moe_route_fused(kw.get("x", x), kw.get("emap"), kw.get("topk", 2), kw.get("ne", 8), True)   # noqa: E731
    grp = lambda **kw: amd.moe_route_grouped_fused(kw.get("x", x), kw.get("bias"), kw.get("emap"), kw.get("topk", 2), kw.get("ne", 8), 2, 1, 0, True, 1.0)   # noqa: E731
    for op in (soft, grp):
        for kw, msg in (({"x": x.cpu()}, "Expected tensor to have cuda DeviceType"), ({"x": torch.zeros(4, 16, dtype=BF16, device=DEV)[:, ::2]}, "Expected contiguous tensor"),
                        ({"x": x.to(torch.float16)}, "logits must be bf16 or float32"), ({"x": torch.zeros(8, dtype=BF16, device=DEV)}, "logits must be 2D"),
                        ({"topk": 0}, "topk must be in"), ({"topk": 33}, "topk must be in"), ({"topk": 9}, "topk must be in"), ({"ne": 0}, "number of experts"),
                        ({"ne": 1025}, "number of experts"), ({"emap": emap.cpu()}, "Expected tensor to have cuda DeviceType"),
                        ({"emap": emap.long()}, "expert_map must be a 1D int32 tensor"), ({"emap": emap[:0]}, "expert_map must be a 1D int32 tensor")):
            with pytest.raises(RuntimeError, match=msg.replace("(", r"\(")):
                op(**kw)
    for b in (bias.double(), bias[:7], bias.cpu()):
        with pytest.raises(RuntimeError, match="bias must be a float32 tensor|cuda DeviceType"):
            grp(bias=b)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(soft(), q.moe_route(x, 2)))            # and the device is as usable as before


# ------------------------------------------------------------------------------------------------
# 6. graph capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("router", ["softmax", "grouped"])
def test_graph_capture_replays_the_eager_results(q, router):
    T = 4
    cfg = GROUPED["deepseek_v3"]
    E, topk = (cfg[0], cfg[3]) if router == "grouped" else (64, 8)
    kw = _grouped_kw(cfg)

    def step(lg):
        return q.moe_route_grouped_fused(lg, topk, **kw) if router == "grouped" else q.moe_route_fused(lg, topk)

    gen = torch.Generator(device="cpu").manual_seed(31)
    logits = [(torch.randn(T, E, generator=gen) * 3.0).to(BF16).to(DEV) for _ in range(3)]
    eager = [step(lg) for lg in logits]
    torch.cuda.synchronize()
    buf = logits[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        step(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step(buf)
    for j in (1, 2, 0):
        buf.copy_(logits[j])
        for t in cap:
            t.view(torch.uint8).zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(cap, eager[j], (router, j))


# ------------------------------------------------------------------------------------------------
# 7. footprint: every byte of the five results written, nothing else, the inputs read-only
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("router", ["softmax", "grouped"])
def test_footprint(q, router):
    T, topk, E, L = 9, 5, 129, 43
    lib = fp.cabi()
    x = _logits(T, E, BF16, topk, seed=3)
    emap_np = np.full(E, -1, dtype=np.int32)
    emap_np[40:40 + L] = np.arange(L)
    bias = torch.randint(-3, 4, (E,), generator=torch.Generator(device="cpu").manual_seed(1)).float() / 8.0
    lay = fp.Layout().input("logits", x).input("expert_map", torch.from_numpy(emap_np))
    if router == "grouped":
        lay.input("bias", bias)
    lay.output("weights", T * topk * 4).output("ids", T * topk * 4).output("src_row", T * topk * 4).output("offs", L * 4).output("pos", T * topk * 4)

    def call(a):
        tail = (L, a.ptr("expert_map"), E, a.ptr("src_row"), a.ptr("offs"), a.ptr("pos"), fp.stream())
        if router == "grouped":   # 129 = 3 groups of 43, the best two, sigmoid, bias, x 2.5
            fp.ok(lib, lib.qutlass_amd_moe_route_grouped_fused(a.ptr("logits"), 2, T, E, topk, 3, 2, 0, a.ptr("bias"), 1, 2.5, a.ptr("weights"), a.ptr("ids"), *tail))
        else:
            fp.ok(lib, lib.qutlass_amd_moe_route_fused(a.ptr("logits"), 2, T, E, topk, 1, a.ptr("weights"), a.ptr("ids"), *tail))

    res = fp.run_twice(lay, call, DEV)
    xd, emap = x.to(DEV), torch.from_numpy(emap_np).to(DEV)
    if router == "grouped":
        want = q.moe_route_grouped(xd, topk, L, n_group=3, topk_group=2, bias=bias.to(DEV), routed_scaling_factor=2.5, expert_map=emap)
    else:
        want = q.moe_route(xd, topk, L, expert_map=emap)
    for name, w in zip(NAMES, want):
        assert np.array_equal(res[name].view(np.int32), w.cpu().contiguous().view(I32).numpy().reshape(-1)), (router, name)


# ------------------------------------------------------------------------------------------------
# 8. a whole layer with the one-launch routing in front
# ------------------------------------------------------------------------------------------------
def test_moe_layer_is_byte_equal_to_the_chain_behind_moe_route(q):
    T, E, topk, H, I, R = 8, 4, 2, 256, 128, 32
    h = _hadamard(R)
    gen = torch.Generator(device="cpu").manual_seed(8)
    tok = torch.randn(T, H, generator=gen).to(BF16).to(DEV)
    w13 = torch.randn(E, 2 * I, H, generator=gen).to(BF16).to(DEV)
    w2 = torch.randn(E, H, I, generator=gen).to(BF16).to(DEV)
    alpha = torch.ones(1, device=DEV)
    logits = torch.randn(T, E, generator=gen).to(DEV)

    def quant_w(w):   # (E, N, K) -> codes (E, N, K/2), row-major scales (E * N * K / 32)
        c, s = q.fusedQuantizeMx(w.view(-1, w.size(-1)), h, method="abs_max")
        return c.view(w.size(0), w.size(1), -1), s.view(torch.uint8).reshape(-1)[: w.numel() // 32].clone().view(torch.float8_e8m0fnu)

    w13q, w13s = quant_w(w13)
    w2q, w2s = quant_w(w2)

    def layer(weights, ids, src_row, offs, pos):
        aq, asf = q.fusedGatherQuantizeMx(tok, h, src_row, method="abs_max")
        gate_up = q.grouped_matmul_mxf4_bf16_tn(aq, w13q, asf, w13s, alpha, offs)
        bq, bsf = q.fusedSiluMulQuantizeMx(gate_up, h, method="abs_max")
        return q.moe_combine(q.grouped_matmul_mxf4_bf16_tn(bq, w2q, bsf, w2s, alpha, offs), pos, weights)

    out, ref = layer(*q.moe_route_fused(logits, topk)), layer(*q.moe_route(logits, topk))
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == BF16
    assert np.array_equal(_np(out), _np(ref)), int((_np(out) != _np(ref)).sum())
    assert np.isfinite(out.float().cpu().numpy()).all() and float(out.float().abs().max()) > 0
