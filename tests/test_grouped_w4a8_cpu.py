"""W4A8 grouped GEMM (grouped_matmul_mxf8_mxf4_bf16_tn) on the host: the C entry's declaration, the boundary sweep of tests/test_grouped_formats_cpu.py through the new
entry and its debug plan entry (row bytes K for the tokens, K/2 for the weights), the form rule, the torch op's rejections, its fake kernel and the traces of the
quantise -> GEMM chain and of the dense wrapper.  No GPU needed; the GPU half is tests/test_gpu_grouped_w4a8.py."""
import ctypes
import os
import re

import pytest
import torch

import test_grouped_formats_cpu as sweep   # the shared boundary sweep: the same case ids, BASE and helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn"
PLAN = "qutlass_amd_debug_grouped_mxf8_mxf4_plan"
TILES = [(32, 32), (32, 16), (64, 32)]     # forms 602, 603, 604
FORM0 = 602
E4, E8M0 = torch.float8_e4m3fn, torch.float8_e8m0fnu


def _want(M, K, E):
    return 604 if M >= 32 * E and K > 1536 else 602   # mean rows per group and K


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    p = getattr(L, PLAN)
    p.restype = ctypes.c_int
    p.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    return L


def test_entry_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
    assert re.search(r"\b" + ENTRY + r"\s*\(", hdr)
    assert not re.search(r"\b" + PLAN + r"\b", hdr), "debug entries stay out of the public header"
    assert hasattr(lib, ENTRY) and hasattr(lib, PLAN)
    from qutlass_amd._lib import SYMBOLS
    from qutlass_amd import build

    assert SYMBOLS[ENTRY] == SYMBOLS["qutlass_amd_grouped_matmul_mxf4_bf16_tn"], "the MXFP8 entry's arguments without a_format"
    assert os.path.exists(build.BENCH_OUT) and hasattr(ctypes.CDLL(build.BENCH_OUT), ENTRY), "the lab library exports the entry too"


# ---- the boundary sweep of the three grouped formats, through the fourth ---------------------------------------------------------------------------------------

def _cases():
    """tests/test_grouped_formats_cpu.py's cases with this op's row bytes: the token matrix reaches 2 GiB at M * K, one expert's weight at N * K/2, and the workgroup
    bound sits where this op's three tiles put it"""
    fmt = "w4a8"
    sweep.FORMATS[fmt] = dict(entry=ENTRY, plan=PLAN, row_bytes=lambda K: K // 2, a_format=False, form0=FORM0, tiles=TILES, picks={602, 604}, want=_want)
    try:
        cases = sweep._cases(fmt)
    finally:
        del sweep.FORMATS[fmt]
    ids = [c[0] for c in cases]
    K = 131072
    m2g = (1 << 31) // K                     # the tokens are 8-bit: M * K bytes
    cases[ids.index("M at 2 GiB")] = ("M at 2 GiB", dict(M=m2g, K=K), "token matrix")
    cases[ids.index("M below 2 GiB")] = ("M below 2 GiB", dict(M=m2g - 1, K=K), sweep.OK)
    cases[ids.index("M below 2 GiB, K=128")] = ("M below 2 GiB, K=128", dict(M=(1 << 31) // 128 - 1, N=1024, K=128), "2^24 workgroups")
    return cases


def _entry(lib, a):
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch
    rc = getattr(lib, ENTRY)(d, d, d, d, d, a["n_alpha"], d, d, a["M"], a["N"], a["K"], a["E"], None)
    return rc, lib.qutlass_amd_last_error().decode() if rc else ""


def _plan(lib, a):
    grid = ctypes.c_int64(-1)
    v = getattr(lib, PLAN)(a["M"], a["N"], a["K"], a["E"], ctypes.byref(grid))
    return ("rejected", lib.qutlass_amd_last_error().decode()) if v == -1 else ("ok", v, grid.value)


def _check_plan(a, got):
    _, v, grid = got
    assert v == _want(a["M"], a["K"], a["E"]), (a, v)
    TM, TN = TILES[v - FORM0]
    assert grid == (0 if a["M"] == 0 else (sweep._cdiv(a["M"], TM) + a["E"]) * sweep._cdiv(a["N"], TN)), (a, v, grid)


def test_boundary_sweep(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    cases = _cases()
    assert [c[0] for c in cases] == [c[0] for c in sweep._cases("mxf8")], "the same case ids as the three formats"
    for cid, over, want in cases:
        a = dict(sweep.BASE, **over)
        if want is not sweep.OK or a["M"] == 0:   # the entry returns before a launch
            rc, msg = _entry(lib, a)
            if want is sweep.OK:
                assert rc == 0, (cid, rc, msg)
            else:
                assert rc == QAMD_ERR_INVALID and want in msg, (cid, rc, msg)
                assert ENTRY[len("qutlass_amd_"):] in msg, (cid, msg)   # the message names the op
        if a["n_alpha"] == 1:
            got = _plan(lib, a)
            if want is sweep.OK:
                assert got[0] == "ok", (cid, got)
                _check_plan(a, got)
            else:
                assert got[0] == "rejected" and want in got[1], (cid, got)


def test_same_outcomes_as_the_mxf8_entry(lib):
    """every case of the sweep ends in this entry as the same logical case ends in grouped_matmul_mxf8_bf16_tn: same return code, same message but for the op's name
    and the weight's row bytes"""
    mine, theirs = _cases(), sweep._cases("mxf8")
    for (cid, over, want), (_, over8, want8) in zip(mine, theirs):
        assert want == want8, cid
        a, a8 = dict(sweep.BASE, **over), dict(sweep.BASE, **over8)
        if want is not sweep.OK or a["M"] == 0:
            rc, msg = _entry(lib, a)
            rc8, msg8 = sweep._run_entry(lib, "mxf8", a8)
            assert rc == rc8, (cid, rc, rc8)
            strip = lambda m: re.sub(r"-?\d+", "#", m.split(": ", 1)[-1].replace("K/2", "K"))   # the words: without the op's name and the case's numbers
            assert strip(msg) == strip(msg8), (cid, msg, msg8)


def test_plan_workgroups_and_every_form_the_rule_picks(lib):
    forms = set()
    for E in (1, 8, 1024):
        for M in (1, 16 * E, 32 * E - 1, 32 * E, 48 * E, 64 * E):
            for K in (128, 768, 1536, 1664, 3072, 3200, 8192):
                for N in (8, 520, 2048):
                    a = dict(M=M, N=N, K=K, E=E)
                    got = _plan(lib, a)
                    assert got[0] == "ok", (a, got)
                    _check_plan(a, got)
                    forms.add(got[1])
    assert forms == {602, 604}   # every form the rule can pick was met
    p = getattr(lib, PLAN)
    assert p(128, 5888, 2944, 32, None) == 602       # gpt-oss-20b gate/up decode: 4 rows per expert
    assert p(8192, 2944, 2944, 32, None) == 604      # ... down, prefill
    assert p(64, 2048, 4000, 8, None) == -1 and p(64, 2044, 4096, 8, None) == -1 and p(64, 2048, 4096, 1025, None) == -1
    assert p(64, 32768, 131072, 8, None) == -1       # one expert of N * K/2 = 2 GiB
    assert p(64, 32760, 131072, 8, None) == 602      # ... just below: the MXFP8 entry rejects this N (its weight rows are K bytes)


# ---- the torch op -------------------------------------------------------------------------------------------------------------------------------------------

def _operands(M=96, N=64, K=512, E=4, adtype=E4, bdtype=torch.uint8):
    a = torch.zeros(M, K, dtype=torch.uint8).view(adtype)
    b = torch.zeros(E, N, K // 2, dtype=torch.uint8).view(bdtype)
    return [a, b, torch.zeros(M * K // 32, dtype=torch.uint8).view(E8M0), torch.zeros(E * N * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1),
            torch.full((E,), M, dtype=torch.int32)]


def test_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    import qutlass_amd as q

    f = q.grouped_matmul_mxf8_mxf4_bf16_tn
    with pytest.raises(ValueError, match=r"grouped_matmul_mxf8_mxf4_bf16_tn: a must be float8_e4m3fn, float8_e5m2 tokens are not supported"):
        f(*_operands(adtype=torch.float8_e5m2))
    with pytest.raises(ValueError, match=r"a must be float8_e4m3fn \(got torch.uint8\)"):
        f(*_operands(adtype=torch.uint8))
    with pytest.raises(ValueError, match=r"b must be uint8 or float4_e2m1fn_x2"):
        f(*_operands(bdtype=E4))               # the MXFP8 op's weights
    args = _operands()
    args[1] = torch.zeros(4, 64, 512, dtype=torch.uint8)   # (E, N, K) bytes: not packed
    with pytest.raises(ValueError, match=r"inner dimensions must match"):
        f(*args)
    args = _operands()
    args[2] = args[2][:-1]
    with pytest.raises(ValueError, match=r"a_sf has 1535 elements, the row-major scale layout needs 1536"):
        f(*args)
    args = _operands()
    args[3] = args[3][:-1]
    with pytest.raises(ValueError, match=r"b_sf has 4095 elements, the row-major scale layout needs 4096"):
        f(*args)
    with pytest.raises(ValueError, match=r"matmul_mxf8_mxf4_bf16_tn: a must be float8_e4m3fn, float8_e5m2"):
        a, b, asf, bsf, alpha, _ = _operands(E=1, adtype=torch.float8_e5m2)
        q.matmul_mxf8_mxf4_bf16_tn(a, b[0], asf, bsf, alpha)
    with pytest.raises(ValueError, match=r"b 2D \(N, K/2\)"):
        a, b, asf, bsf, alpha, _ = _operands(E=1)
        q.matmul_mxf8_mxf4_bf16_tn(a, b, asf, bsf, alpha)


def test_fake_kernel_and_quantise_gemm_trace():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass
    import qutlass_amd as q

    assert qutlass.grouped_matmul_mxf8_mxf4_bf16_tn is q.grouped_matmul_mxf8_mxf4_bf16_tn and qutlass.matmul_mxf8_mxf4_bf16_tn is q.matmul_mxf8_mxf4_bf16_tn
    assert q.grouped_matmul_mxf8_mxf4_bf16_tn.__doc__.startswith("EXTENSION") and q.matmul_mxf8_mxf4_bf16_tn.__doc__.startswith("EXTENSION")
    assert "grouped_matmul_mxf8_mxf4_bf16_tn" in q.__doc__ and "matmul_mxf8_mxf4_bf16_tn" in q.__doc__
    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_mxf8_mxf4").fake_impl.kernel is not None
    M, N, K, E = 96, 256, 512, 4
    for bdtype in (torch.uint8, torch.float4_e2m1fn_x2):
        with FakeTensorMode():
            a = torch.empty(M, K, dtype=E4, device=DEV)
            b = torch.empty(E, N, K // 2, dtype=bdtype, device=DEV)
            a_sf = torch.empty(M * K // 32, dtype=E8M0, device=DEV)
            b_sf = torch.empty(E * N * K // 32, dtype=E8M0, device=DEV)
            out = q.grouped_matmul_mxf8_mxf4_bf16_tn(a, b, a_sf, b_sf, torch.empty(E, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))
            assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"

    # quantise -> GEMM: the tokens go through fusedQuantizeMxf8 inside the traced function
    def layer(x, h, b, b_sf, alpha, offs):
        a, a_sf = q.fusedQuantizeMxf8(x, h)
        return q.grouped_matmul_mxf8_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs) * 2

    with FakeTensorMode():
        args = (torch.empty(M, K, dtype=torch.bfloat16, device=DEV), torch.empty(32, 32, dtype=torch.bfloat16, device=DEV),
                torch.empty(E, N, K // 2, dtype=torch.uint8, device=DEV), torch.empty(E * N * K // 32, dtype=E8M0, device=DEV),
                torch.empty(1, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))
        out = layer(*args)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16
        gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf8_mxf4.default" in targets, targets
    assert any("uantize" in t and "xf8" in t for t in targets), targets


def test_dense_wrapper_traces_without_a_host_sync():
    """the wrapper's offs is made on the device from a.size(0): the trace holds a fill and the grouped op, and nothing that reads a tensor's value on the host"""
    from torch._dynamo.backends.common import aot_autograd
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass_amd as q

    M, N, K = 48, 64, 256

    def layer(a, b, a_sf, b_sf, alpha):
        return q.matmul_mxf8_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha)

    args = (torch.zeros(M, K, dtype=torch.uint8).view(E4), torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(M * K // 32, dtype=torch.uint8).view(E8M0),
            torch.zeros(N * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1))
    gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf8_mxf4.default" in targets, targets
    assert not any(s in t for t in targets for s in ("item", "_local_scalar_dense", "nonzero", "_to_copy")), targets
    node = next(n for n in gm.graph.nodes if str(n.target) == "qutlass_amd.grouped_matmul_mxf8_mxf4.default")
    assert tuple(node.args[1].meta["val"].shape) == (1, N, K // 2) and tuple(node.args[5].meta["val"].shape) == (1,)
    assert tuple(node.meta["val"].shape) == (M, N)

    graphs = []

    def capture(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    torch._dynamo.reset()
    try:   # fullgraph: a host sync (.item()) would be a graph break and fail here; the run after the trace has no CPU kernel to call -- the graph exists by then
        torch.compile(layer, backend=aot_autograd(fw_compiler=capture), fullgraph=True)(*args)
    except (NotImplementedError, RuntimeError) as e:
        assert graphs and ("CPU" in str(e) or "backend" in str(e)), e
    assert graphs
    assert "qutlass_amd.grouped_matmul_mxf8_mxf4.default" in [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]
