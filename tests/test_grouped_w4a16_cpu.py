"""W4A16 grouped GEMM (grouped_matmul_bf16_mxf4_bf16_tn) on the host: the C entry's declaration, the boundary sweep of tests/test_grouped_formats_cpu.py through the new
entry and its debug plan entry (row bytes 2K for the tokens, K/2 for the weights), the form rule, the entry's rejections (the gather's among them), the torch op's
fake kernel, the Python wrappers' errors and the traces of the op and of the dense wrapper.  No GPU needed; the GPU half is tests/test_gpu_grouped_w4a16.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import test_grouped_formats_cpu as sweep   # the shared boundary sweep: the same case ids, BASE and helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn"
PLAN = "qutlass_amd_debug_grouped_bf16_mxf4_plan"
TILES = [(32, 32), (32, 16), (64, 32)]     # forms 606, 607, 608
FORM0 = 606
E8M0 = torch.float8_e8m0fnu


def _want(M, K, E):
    return 608 if M >= 32 * E and K > 512 else 606   # capi.hip grouped_w4a16_plan, re-fitted from profiles/calib_grouped_w4a16.txt: mean rows per group and K


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

    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert SYMBOLS[ENTRY] == (ctypes.c_int, [vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, vp]), "A, B, B_sf, alpha, n_alpha, offs, src_row, T, D, M, N, K, E, stream"
    assert os.path.exists(build.BENCH_OUT) and hasattr(ctypes.CDLL(build.BENCH_OUT), ENTRY), "the lab library exports the entry too"


# ---- the boundary sweep of the grouped formats, through this one ------------------------------------------------------------------------------------------------

def _cases():
    """tests/test_grouped_formats_cpu.py's cases with this op's row bytes: the token matrix reaches 2 GiB at M * 2K, one expert's weight at N * K/2, and the workgroup
    bound sits where this op's three tiles put it"""
    fmt = "w4a16"
    sweep.FORMATS[fmt] = dict(entry=ENTRY, plan=PLAN, row_bytes=lambda K: K // 2, a_format=False, form0=FORM0, tiles=TILES, picks={606, 608}, want=_want)
    try:
        cases = sweep._cases(fmt)
    finally:
        del sweep.FORMATS[fmt]
    ids = [c[0] for c in cases]
    K = 131072
    m2g = (1 << 31) // (2 * K)               # the tokens are 16-bit: M * 2K bytes
    cases[ids.index("M at 2 GiB")] = ("M at 2 GiB", dict(M=m2g, K=K), "token matrix")
    cases[ids.index("M below 2 GiB")] = ("M below 2 GiB", dict(M=m2g - 1, K=K), sweep.OK)
    cases[ids.index("M below 2 GiB, K=128")] = ("M below 2 GiB, K=128", dict(M=(1 << 31) // 256 - 1, N=2048, K=128), "2^24 workgroups")
    return cases


def _entry(lib, a, src_row=None, T=0, A=0x1000, B=0x1000, B_sf=0x1000, alpha=0x1000, offs=0x1000, D=0x1000):
    p = lambda v: ctypes.c_void_p(v) if v else None   # never dereferenced: every call here returns before a launch
    rc = getattr(lib, ENTRY)(p(A), p(B), p(B_sf), p(alpha), a["n_alpha"], p(offs), p(src_row), T, p(D), a["M"], a["N"], a["K"], a["E"], None)
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
    and the operands' row bytes"""
    mine, theirs = _cases(), sweep._cases("mxf8")
    for (cid, over, want), (_, over8, want8) in zip(mine, theirs):
        assert want == want8, cid
        a, a8 = dict(sweep.BASE, **over), dict(sweep.BASE, **over8)
        if want is not sweep.OK or a["M"] == 0:
            rc, msg = _entry(lib, a)
            rc8, msg8 = sweep._run_entry(lib, "mxf8", a8)
            assert rc == rc8, (cid, rc, rc8)
            strip = lambda m: re.sub(r"-?\d+", "#", m.split(": ", 1)[-1].replace("2K", "K").replace("K/2", "K"))   # the words: without the op's name and the case's numbers
            assert strip(msg) == strip(msg8), (cid, msg, msg8)


def test_plan_returns_only_its_three_forms_pinned_at_the_thresholds(lib):
    forms = set()
    for E in (1, 8, 1024):
        for M in (1, 16 * E, 32 * E - 1, 32 * E, 48 * E, 64 * E):
            for K in (128, 512, 640, 1024, 1152, 1536, 1664, 8192):
                for N in (8, 520, 2048):
                    a = dict(M=M, N=N, K=K, E=E)
                    got = _plan(lib, a)
                    assert got[0] == "ok", (a, got)
                    assert FORM0 <= got[1] < FORM0 + 3, (a, got)
                    _check_plan(a, got)
                    forms.add(got[1])
    assert forms == {606, 608}   # every form the rule can pick was met
    p = getattr(lib, PLAN)
    assert p(256, 64, 512, 8, None) == 606 and p(256, 64, 640, 8, None) == 608       # the K threshold, at 32 rows per expert
    assert p(255, 64, 640, 8, None) == 606 and p(255, 64, 8192, 8, None) == 606      # ... and the row threshold
    assert p(32768, 2048, 768, 128, None) == 608         # Qwen3-30B-A3B down, prefill: the shape the provisional rule (K > 1024) missed
    assert p(128, 5760, 2880 + 64, 32, None) == 606      # gpt-oss-20b gate/up decode (K padded to 2944): 4 rows per expert
    assert p(8192, 2944, 2944, 32, None) == 608          # ... down, prefill
    assert p(64, 2048, 4000, 8, None) == -1 and p(64, 2044, 4096, 8, None) == -1 and p(64, 2048, 4096, 1025, None) == -1
    assert p(64, 32768, 131072, 8, None) == -1           # one expert of N * K/2 = 2 GiB
    assert p(64, 32760, 131072, 8, None) == 606
    assert p(8192, 64, 131072, 8, None) == -1 and p(8191, 64, 131072, 8, None) == 608   # the token matrix: M * 2K = 2 GiB


def test_entry_rejections(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    ok = dict(M=64, N=64, K=512, E=4, n_alpha=1)
    for name in ("A", "B", "B_sf", "alpha", "offs", "D"):
        rc, msg = _entry(lib, ok, **{name: 0})
        assert rc == QAMD_ERR_INVALID and "null pointer" in msg, (name, rc, msg)
    for over, words in ((dict(K=448), "K must be a positive multiple of 128"), (dict(N=60), "N must be a multiple of 8"), (dict(E=1025), "E must be in [1, 1024]"),
                        (dict(n_alpha=2), "alpha must have 1 or E"), (dict(n_alpha=0), "alpha must have 1 or E"), (dict(n_alpha=5), "alpha must have 1 or E")):
        rc, msg = _entry(lib, dict(ok, **over))
        assert rc == QAMD_ERR_INVALID and words in msg and "grouped_matmul_bf16_mxf4_bf16_tn" in msg, (over, rc, msg)
    # the gather: the descriptor spans all T rows of 2K bytes
    K = 4096
    t2g = (1 << 31) // (2 * K)
    rc, msg = _entry(lib, dict(ok, K=K), src_row=0x1000, T=t2g)
    assert rc == QAMD_ERR_INVALID and "gathered token matrix" in msg and "2 GiB" in msg, (rc, msg)
    rc, msg = _entry(lib, dict(ok, K=K), src_row=0x1000, T=-1)
    assert rc == QAMD_ERR_INVALID and "T must be >= 0" in msg, (rc, msg)
    assert _entry(lib, dict(ok, K=K, M=0), src_row=0x1000, T=t2g - 1)[0] == 0      # just below, no rows: accepted, nothing launched
    assert _entry(lib, dict(ok, K=K, M=0), src_row=None, T=-1)[0] == 0             # T is not read without src_row


# ---- the torch op and the Python wrappers -------------------------------------------------------------------------------------------------------------------------

def _operands(M=96, N=64, K=512, E=4, adtype=torch.bfloat16, bdtype=torch.uint8):
    a = torch.zeros(M, K, dtype=adtype)
    b = torch.zeros(E, N, K // 2, dtype=torch.uint8).view(bdtype)
    return [a, b, torch.zeros(E * N * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1), torch.full((E,), M, dtype=torch.int32)]


def test_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    import qutlass_amd as q

    f = q.grouped_matmul_bf16_mxf4_bf16_tn
    with pytest.raises(ValueError, match=r"grouped_matmul_bf16_mxf4_bf16_tn: a must be bfloat16 \(got torch.float16"):
        f(*_operands(adtype=torch.float16))
    with pytest.raises(ValueError, match=r"a must be bfloat16 \(got torch.float8_e4m3fn"):
        f(*_operands(adtype=torch.float8_e4m3fn))
    with pytest.raises(ValueError, match=r"b must be uint8 or float4_e2m1fn_x2"):
        f(*_operands(bdtype=torch.float8_e4m3fn))
    args = _operands()
    args[1] = torch.zeros(4, 64, 512, dtype=torch.uint8)   # (E, N, K) bytes: not packed
    with pytest.raises(ValueError, match=r"inner dimensions must match"):
        f(*args)
    args = _operands()
    args[1] = args[1][0]
    with pytest.raises(ValueError, match=r"a must be 2D \(M, K\) and b 3D \(E, N, K/2\)"):
        f(*args)
    args = _operands()
    args[2] = args[2][:-1]
    with pytest.raises(ValueError, match=r"b_sf has 4095 elements, the row-major scale layout needs 4096"):
        f(*args)
    args = _operands()
    args[2] = args[2].view(torch.uint8)
    with pytest.raises(ValueError, match=r"b_sf must be float8_e8m0fnu"):
        f(*args)
    with pytest.raises(ValueError, match=r"src_row must be a 1D int32 tensor \(got torch.int64"):
        f(*_operands(), src_row=torch.zeros(96, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"src_row must be a 1D int32 tensor"):
        f(*_operands(), src_row=torch.zeros(96, 1, dtype=torch.int32))
    with pytest.raises(TypeError):
        f(*_operands(), torch.zeros(96, dtype=torch.int32))          # src_row is keyword-only
    with pytest.raises(ValueError, match=r"matmul_bf16_mxf4_bf16_tn: a must be bfloat16"):
        a, b, bsf, alpha, _ = _operands(E=1, adtype=torch.float32)
        q.matmul_bf16_mxf4_bf16_tn(a, b[0], bsf, alpha)
    with pytest.raises(ValueError, match=r"b 2D \(N, K/2\)"):
        a, b, bsf, alpha, _ = _operands(E=1)
        q.matmul_bf16_mxf4_bf16_tn(a, b, bsf, alpha)
    with pytest.raises((RuntimeError, NotImplementedError), match=r"cuda DeviceType|CPU"):   # well-formed CPU tensors reach the op, which has no CPU path
        f(*_operands())


def test_fake_kernel_shape_dtype_and_exports():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import qutlass
    import qutlass_amd as q

    assert qutlass.grouped_matmul_bf16_mxf4_bf16_tn is q.grouped_matmul_bf16_mxf4_bf16_tn and qutlass.matmul_bf16_mxf4_bf16_tn is q.matmul_bf16_mxf4_bf16_tn
    assert q.grouped_matmul_bf16_mxf4_bf16_tn.__doc__.startswith("EXTENSION") and q.matmul_bf16_mxf4_bf16_tn.__doc__.startswith("EXTENSION")
    assert "grouped_matmul_bf16_mxf4_bf16_tn" in q.__doc__ and "matmul_bf16_mxf4_bf16_tn" in q.__doc__
    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_bf16_mxf4_bf16_tn").fake_impl.kernel is not None
    schema = torch.ops.qutlass_amd.grouped_matmul_bf16_mxf4_bf16_tn.default._schema
    assert not any(a.alias_info is not None for a in schema.arguments) and len(schema.returns) == 1, str(schema)   # functional: allocates its result
    M, N, K, E, T = 96, 256, 512, 4, 24
    for bdtype in (torch.uint8, torch.float4_e2m1fn_x2):
        with FakeTensorMode():
            b = torch.empty(E, N, K // 2, dtype=bdtype, device=DEV)
            b_sf = torch.empty(E * N * K // 32, dtype=E8M0, device=DEV)
            alpha, offs = torch.empty(E, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV)
            out = q.grouped_matmul_bf16_mxf4_bf16_tn(torch.empty(M, K, dtype=torch.bfloat16, device=DEV), b, b_sf, alpha, offs)
            assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"
            out = q.grouped_matmul_bf16_mxf4_bf16_tn(torch.empty(T, K, dtype=torch.bfloat16, device=DEV), b, b_sf, alpha, offs,
                                                     src_row=torch.empty(M, dtype=torch.int32, device=DEV))
            assert out.shape == (M, N) and out.dtype == torch.bfloat16, "with src_row the rows are src_row's"
            out = q.matmul_bf16_mxf4_bf16_tn(torch.empty(M, K, dtype=torch.bfloat16, device=DEV), b[0], b_sf, alpha[:1])
            assert out.shape == (M, N) and out.dtype == torch.bfloat16


def test_gather_layer_and_dense_wrapper_trace_with_fullgraph():
    """route -> W4A16 with src_row traces as two ops; the dense wrapper's offs is made on the device from a.size(0): nothing reads a tensor's value on the host"""
    from torch._dynamo.backends.common import aot_autograd
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass_amd as q

    M, N, K, E = 48, 64, 256, 4
    OP = "qutlass_amd.grouped_matmul_bf16_mxf4_bf16_tn.default"

    def dense(a, b, b_sf, alpha):
        return q.matmul_bf16_mxf4_bf16_tn(a, b, b_sf, alpha)

    def gathered(x, b, b_sf, alpha, offs, src_row):
        return q.grouped_matmul_bf16_mxf4_bf16_tn(x, b, b_sf, alpha, offs, src_row=src_row) * 2

    dargs = (torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(N * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1))
    gargs = (torch.zeros(12, K, dtype=torch.bfloat16), torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.zeros(E * N * K // 32, dtype=torch.uint8).view(E8M0),
             torch.ones(1), torch.zeros(E, dtype=torch.int32), torch.zeros(M, dtype=torch.int32))
    gm = make_fx(dense, tracing_mode="fake")(*dargs)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert OP in targets, targets
    assert not any(s in t for t in targets for s in ("item", "_local_scalar_dense", "nonzero", "_to_copy")), targets
    node = next(n for n in gm.graph.nodes if str(n.target) == OP)
    assert tuple(node.args[1].meta["val"].shape) == (1, N, K // 2) and tuple(node.args[4].meta["val"].shape) == (1,) and node.args[5] is None
    assert tuple(node.meta["val"].shape) == (M, N)
    gm = make_fx(gathered, tracing_mode="fake")(*gargs)
    node = next(n for n in gm.graph.nodes if str(n.target) == OP)
    assert tuple(node.meta["val"].shape) == (M, N) and node.meta["val"].dtype == torch.bfloat16

    for fn, args in ((dense, dargs), (gathered, gargs)):
        graphs = []

        def capture(gm, example_inputs):
            graphs.append(gm)
            return gm.forward

        torch._dynamo.reset()
        try:   # fullgraph: a host sync would be a graph break and fail here; the run after the trace has no CPU path to call -- the graph exists by then
            torch.compile(fn, backend=aot_autograd(fw_compiler=capture), fullgraph=True)(*args)
        except (NotImplementedError, RuntimeError) as e:
            assert graphs and ("CPU" in str(e) or "backend" in str(e) or "cuda DeviceType" in str(e)), e
        assert graphs and OP in [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]


def test_exact_regime_holds_for_every_case_the_gpu_half_uses():
    """tests/_w4a16_model.py: the operands of every exact comparison of tests/test_gpu_grouped_w4a16.py are asserted exact here, on the CPU"""
    import _w4a16_model as W
    G = W   # the case lists live beside the model

    for K in G.LADDER_K:
        W.assert_exact(W.exact_problem(3, 40, K, 64, seed=K), G.LADDER_COUNTS)
    for N in G.RAGGED_N:
        W.assert_exact(W.exact_problem(9, N, 640, int(np.sum(G.RAGGED_COUNTS)), seed=N), G.RAGGED_COUNTS)
    for K, shift in G.ONE_HOT:
        p = W.one_hot_problem(K, shift)
        W.assert_exact(p, [p.M])
    assert W.token_amax(128) == 16.0 and W.token_amax(3200) < 6.0
