"""W4A6 (grouped_matmul_mxf6_mxf4_bf16_tn, fusedQuantizeMxf6, fusedGatherQuantizeMxf6) on the host: the C entries' declarations, the boundary sweep of
tests/test_grouped_formats_cpu.py through the new GEMM entry and its debug plan entry (row bytes 3K/4 for the tokens, K/2 for the weights), the form rule and the grid
formula, every argument rejection with its message, the torch ops' rejections, their fake kernels and the trace of the quantise -> GEMM chain.  No GPU needed; the
GPU half is tests/test_gpu_grouped_w4a6.py and tests/test_gpu_mxf6_quantize.py."""
import ctypes
import os
import re

import pytest
import torch

import test_grouped_formats_cpu as sweep   # the shared boundary sweep: the same case ids, BASE and helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ENTRY = "qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn"
PLAN = "qutlass_amd_debug_grouped_mxf6_mxf4_plan"
QUANT, GATHER = "qutlass_amd_fused_quantize_mxf6", "qutlass_amd_fused_gather_quantize_mxf6"
TILES = [(32, 32), (32, 16), (64, 32)]     # forms 610, 611, 612
FORM0 = 610
E8M0 = torch.float8_e8m0fnu


def _want(M, K, E):
    return 612 if (M >= 32 * E and K > 1536) or (M >= 48 * E and K <= 1024) else 610   # mean rows per group and K


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    p = getattr(L, PLAN)
    p.restype = ctypes.c_int
    p.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    return L


def test_entries_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
    for name in (ENTRY, QUANT, GATHER):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name), name
    assert not re.search(r"\b" + PLAN + r"\b", hdr), "debug entries stay out of the public header"
    assert hasattr(lib, PLAN)
    from qutlass_amd._lib import SYMBOLS
    from qutlass_amd import build

    assert SYMBOLS[ENTRY] == SYMBOLS["qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn"], "the W4A8 entry's arguments"
    mxf8 = SYMBOLS["qutlass_amd_fused_quantize_mxf8"]
    assert SYMBOLS[QUANT] == (mxf8[0], mxf8[1][:4] + mxf8[1][5:]), "the MXFP8 entry's arguments without fmt"
    g8 = SYMBOLS["qutlass_amd_fused_gather_quantize_mxf8"]
    assert SYMBOLS[GATHER] == (g8[0], g8[1][:7] + g8[1][8:]), "the MXFP8 entry's arguments without fmt"
    bench = ctypes.CDLL(build.BENCH_OUT)
    assert all(hasattr(bench, n) for n in (ENTRY, QUANT, GATHER)), "the lab library exports the entries too"


# ---- the boundary sweep of the grouped formats, through this one ---------------------------------------------------------------------------------------------

def _cases():
    """tests/test_grouped_formats_cpu.py's cases with this op's row bytes: the token matrix reaches 2 GiB at M * 3K/4, one expert's weight at N * K/2, and the
    workgroup bound sits where this op's three tiles put it"""
    fmt = "w4a6"
    sweep.FORMATS[fmt] = dict(entry=ENTRY, plan=PLAN, row_bytes=lambda K: K // 2, a_format=False, form0=FORM0, tiles=TILES, picks={610, 612}, want=_want)
    try:
        cases = sweep._cases(fmt)
    finally:
        del sweep.FORMATS[fmt]
    ids = [c[0] for c in cases]
    K = 131072
    m2g = sweep._cdiv(1 << 31, K * 3 // 4)   # the tokens are 6-bit: M * 3K/4 bytes
    assert (m2g - 1) * (K * 3 // 4) < 1 << 31 <= m2g * (K * 3 // 4)
    cases[ids.index("M at 2 GiB")] = ("M at 2 GiB", dict(M=m2g, K=K), "token matrix (M * 3K/4 bytes")
    cases[ids.index("M below 2 GiB")] = ("M below 2 GiB", dict(M=m2g - 1, K=K), sweep.OK)
    cases[ids.index("M below 2 GiB, K=128")] = ("M below 2 GiB, K=128", dict(M=sweep._cdiv(1 << 31, 96) - 1, N=1024, K=128), "2^24 workgroups")
    return cases


def _entry(lib, a, A=0x1000):
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch
    rc = getattr(lib, ENTRY)(ctypes.c_void_p(A), d, d, d, d, a["n_alpha"], d, d, a["M"], a["N"], a["K"], a["E"], None)
    return rc, lib.qutlass_amd_last_error().decode() if rc else ""


def _plan(lib, a):
    grid = ctypes.c_int64(-1)
    v = getattr(lib, PLAN)(a["M"], a["N"], a["K"], a["E"], ctypes.byref(grid))
    return ("rejected", lib.qutlass_amd_last_error().decode()) if v == -1 else ("ok", v, grid.value)


def _check_plan(a, got):
    _, v, grid = got
    assert v == _want(a["M"], a["K"], a["E"]), (a, v)
    TM, TN = TILES[v - FORM0]
    assert grid == (0 if a["M"] == 0 else (sweep._cdiv(a["M"], TM) + a["E"]) * sweep._cdiv(a["N"], TN)), (a, v, grid)   # the grid formula


def test_boundary_sweep(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    cases = _cases()
    assert [c[0] for c in cases] == [c[0] for c in sweep._cases("mxf8")], "the same case ids as the other formats"
    for cid, over, want in cases:
        a = dict(sweep.BASE, **over)
        if want is not sweep.OK or a["M"] == 0:   # the entry returns before a launch
            rc, msg = _entry(lib, a)
            if want is sweep.OK:
                assert rc == 0, (cid, rc, msg)
            else:
                assert rc == QAMD_ERR_INVALID and want in msg, (cid, rc, msg)
                assert msg.startswith(ENTRY[len("qutlass_amd_"):] + ": "), (cid, msg)   # the message names the op
        if a["n_alpha"] == 1:
            got = _plan(lib, a)
            if want is sweep.OK:
                assert got[0] == "ok", (cid, got)
                _check_plan(a, got)
            else:
                assert got[0] == "rejected" and want in got[1], (cid, got)


def test_same_outcomes_as_the_w4a8_entry(lib):
    """every case of the sweep ends in this entry as the same logical case ends in grouped_matmul_mxf8_mxf4_bf16_tn: same return code, same message but for the op's
    name and the tokens' row bytes"""
    import test_grouped_w4a8_cpu as w8

    for (cid, over, want), (cid8, over8, want8) in zip(_cases(), w8._cases()):
        assert cid == cid8 and (want is sweep.OK) == (want8 is sweep.OK), cid
        a, a8 = dict(sweep.BASE, **over), dict(sweep.BASE, **over8)
        if want is not sweep.OK or a["M"] == 0:
            rc, msg = _entry(lib, a)
            rc8, msg8 = w8._entry(lib, a8)
            assert rc == rc8, (cid, rc, rc8)
            strip = lambda m: re.sub(r"-?\d+", "#", m.split(": ", 1)[-1].replace("3K/4", "K"))   # the words: without the op's name and the case's numbers
            assert strip(msg) == strip(msg8), (cid, msg, msg8)


def test_alignment_of_the_token_matrix(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    a = dict(sweep.BASE, M=64)
    for addr in (0x1008, 0x1004, 0x1001):
        rc, msg = _entry(lib, a, A=addr)
        assert rc == QAMD_ERR_INVALID and msg == "grouped_matmul_mxf6_mxf4_bf16_tn: A must be 16-byte aligned", (addr, msg)
    rc, msg = _entry(lib, dict(a, K=192), A=0x1008)     # the shape checks come first
    assert rc == QAMD_ERR_INVALID and msg == "grouped_matmul_mxf6_mxf4_bf16_tn: K must be a positive multiple of 128 (got 192)", msg


def test_plan_workgroups_and_every_form_the_rule_picks(lib):
    forms = set()
    for E in (1, 8, 1024):
        for M in (1, 16 * E, 32 * E - 1, 32 * E, 48 * E, 64 * E):
            for K in (128, 768, 1024, 1152, 1536, 1664, 3584, 3712, 8192):
                for N in (8, 520, 2048):
                    a = dict(M=M, N=N, K=K, E=E)
                    got = _plan(lib, a)
                    assert got[0] == "ok", (a, got)
                    _check_plan(a, got)
                    forms.add(got[1])
    assert forms == {610, 612}   # every form the rule can pick was met
    p = getattr(lib, PLAN)
    assert p(128, 5888, 2944, 32, None) == 610       # gpt-oss-20b gate/up decode: 4 rows per expert
    assert p(8192, 2944, 2944, 32, None) == 612      # ... down, prefill
    assert p(32768, 2048, 768, 128, None) == 612 and p(4096, 2048, 768, 128, None) == 610 and p(16384, 2048, 1536, 128, None) == 610   # Qwen3 down prefill; 32 rows; K = 1536
    assert p(64, 2048, 4000, 8, None) == -1 and p(64, 2044, 4096, 8, None) == -1 and p(64, 2048, 4096, 1025, None) == -1
    assert p(64, 32768, 131072, 8, None) == -1       # one expert of N * K/2 = 2 GiB
    assert p(64, 32760, 131072, 8, None) == 610      # ... just below
    assert p(21846, 64, 131072, 8, None) == -1 and p(21845, 64, 131072, 8, None) == 612   # the tokens: M * 3K/4 at 2 GiB, and just below


# ---- the quantizer entries' rejections -----------------------------------------------------------------------------------------------------------------------

def test_quantizer_entries_reject_with_their_own_names(lib):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    d, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    err = lambda: lib.qutlass_amd_last_error().decode()
    qf, gf = getattr(lib, QUANT), getattr(lib, GATHER)
    for args, msg in (((None, d, 32, 1024, d, d, None), "fusedQuantizeMxf6: null pointer argument"),
                      ((d, d, 16, 1024, d, d, None), "fusedQuantizeMxf6: Unsupported rotation size 16; expected 32, 64, or 128."),
                      ((d, d, 256, 1024, d, d, None), "fusedQuantizeMxf6: Unsupported rotation size 256; expected 32, 64, or 128."),
                      ((d, d, 64, 1000, d, d, None), "fusedQuantizeMxf6: A must be divisible by 64"),
                      ((d, d, 32, 0, d, d, None), "fusedQuantizeMxf6: A must be divisible by 32"),
                      ((d, d, 32, 1 << 31, d, d, None), "fusedQuantizeMxf6: more than 2^31 elements is not supported"),
                      ((d, odd, 64, 1024, d, d, None), "fusedQuantizeMxf6: the rotation matrix must be 16-byte aligned for rotation sizes >= 64")):
        assert qf(*args) == QAMD_ERR_INVALID and err() == msg, (msg, err())
    for args, msg in (((d, d, 16, 8, 128, d, 4, d, d, None), "fusedGatherQuantizeMxf6: Unsupported rotation size 16; expected 32, 64, or 128."),
                      ((d, d, 32, -1, 128, d, 4, d, d, None), "fusedGatherQuantizeMxf6: bad shape (x (-1, 128), 4 indices)"),
                      ((d, d, 64, 8, 96, d, 4, d, d, None), "fusedGatherQuantizeMxf6: the row length 96 must be a multiple of 64"),
                      ((odd, d, 32, 8, 128, d, 4, d, d, None), "fusedGatherQuantizeMxf6: x must be 16-byte aligned (and src_row 4-byte aligned)"),
                      ((d, d, 32, 1 << 20, 1 << 10, d, 4, d, d, None), "fusedGatherQuantizeMxf6: x (rows * k * 2 = 2147483648 bytes) must stay below 2 GiB"),
                      ((d, d, 32, 8, 128, None, 4, d, d, None), "fusedGatherQuantizeMxf6: null pointer argument"),
                      ((d, odd, 128, 8, 128, d, 4, d, d, None), "fusedGatherQuantizeMxf6: the rotation matrix must be 16-byte aligned for rotation sizes >= 64")):
        assert gf(*args) == QAMD_ERR_INVALID and err() == msg, (msg, err())
    assert gf(d, d, 32, 8, 128, d, 0, d, d, None) == 0     # no indices: nothing to launch


# ---- the torch ops --------------------------------------------------------------------------------------------------------------------------------------------

def _operands(M=96, N=64, K=512, E=4, adtype=torch.uint8, bdtype=torch.uint8, awidth=None):
    a = torch.zeros(M, K * 3 // 4 if awidth is None else awidth, dtype=torch.uint8).view(adtype)
    b = torch.zeros(E, N, K // 2, dtype=torch.uint8).view(bdtype)
    return [a, b, torch.zeros(M * K // 32, dtype=torch.uint8).view(E8M0), torch.zeros(E * N * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1),
            torch.full((E,), M, dtype=torch.int32)]


def test_rejections_come_before_any_device_work():
    """CPU tensors on a machine that may have no GPU: each call raises its own message, so nothing was dispatched"""
    import qutlass_amd as q

    f = q.grouped_matmul_mxf6_mxf4_bf16_tn
    with pytest.raises(ValueError, match=r"grouped_matmul_mxf6_mxf4_bf16_tn: a must be uint8, packed e2m3 codes as fusedQuantizeMxf6 writes them \(got torch.float8_e4m3fn\)"):
        f(*_operands(adtype=torch.float8_e4m3fn))
    with pytest.raises(ValueError, match=r"b must be uint8 or float4_e2m1fn_x2"):
        f(*_operands(bdtype=torch.float8_e4m3fn))
    with pytest.raises(ValueError, match=r"inner dimensions must match, a is \(M, 3K/4 = 512\) and b \(.., K/2 = 256\)"):
        f(*_operands(awidth=512))              # the W4A8 op's width: one byte per element
    with pytest.raises(ValueError, match=r"inner dimensions must match"):
        f(*_operands(awidth=256))              # the MXFP4 op's
    args = _operands()
    args[2] = args[2][:-1]
    with pytest.raises(ValueError, match=r"a_sf has 1535 elements, the row-major scale layout needs 1536"):
        f(*args)
    args = _operands()
    args[3] = args[3][:-1]
    with pytest.raises(ValueError, match=r"b_sf has 4095 elements, the row-major scale layout needs 4096"):
        f(*args)
    args = _operands()
    args[2] = args[2].view(torch.uint8)
    with pytest.raises(ValueError, match=r"a_sf must be float8_e8m0fnu"):
        f(*args)
    with pytest.raises(ValueError, match=r"matmul_mxf6_mxf4_bf16_tn: a must be uint8"):
        a, b, asf, bsf, alpha, _ = _operands(E=1, adtype=torch.float8_e4m3fn)
        q.matmul_mxf6_mxf4_bf16_tn(a, b[0], asf, bsf, alpha)
    with pytest.raises(ValueError, match=r"b 2D \(N, K/2\)"):
        a, b, asf, bsf, alpha, _ = _operands(E=1)
        q.matmul_mxf6_mxf4_bf16_tn(a, b, asf, bsf, alpha)


def test_fake_kernels_and_quantise_gemm_trace():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass
    import qutlass_amd as q

    for name in ("grouped_matmul_mxf6_mxf4_bf16_tn", "matmul_mxf6_mxf4_bf16_tn", "fusedQuantizeMxf6", "fusedGatherQuantizeMxf6"):
        assert getattr(qutlass, name) is getattr(q, name) and getattr(q, name).__doc__.startswith("EXTENSION") and name in q.__doc__, name
    q.ops.register_torch_ops()
    assert torch._library.simple_registry.singleton.find("qutlass_amd::grouped_matmul_mxf6_mxf4").fake_impl.kernel is not None
    assert set(q.ops.QUANT_OPS_MXF6) == {"quantize_mxf6", "gather_quantize_mxf6"} and q.ops.QUANT_FORMATS["mxf6"] == (32, E8M0)
    M, N, K, E = 96, 256, 512, 4
    for bdtype in (torch.uint8, torch.float4_e2m1fn_x2):
        with FakeTensorMode():
            a = torch.empty(M, K * 3 // 4, dtype=torch.uint8, device=DEV)
            b = torch.empty(E, N, K // 2, dtype=bdtype, device=DEV)
            a_sf = torch.empty(M * K // 32, dtype=E8M0, device=DEV)
            b_sf = torch.empty(E * N * K // 32, dtype=E8M0, device=DEV)
            out = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, a_sf, b_sf, torch.empty(E, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))
            assert out.shape == (M, N) and out.dtype == torch.bfloat16 and out.device.type == "cuda"
    # the quantizers' allocator (the fake kernels of the functional ops): codes (.., 3K/4) uint8, scales as the MX ops'
    for dev in ("meta", "cpu"):
        x, h = torch.empty(2, 33, 256, dtype=torch.bfloat16, device=dev), torch.empty(64, 64, dtype=torch.bfloat16, device=dev)
        codes, sf = q.ops.alloc_quant(q.ops.QUANT_OPS_MXF6["quantize_mxf6"], x, h)
        ref = q.ops.alloc_quant(q.ops.QUANT_OPS["quantize_mxf8"], x, h, torch.float8_e4m3fn)
        assert codes.shape == (2, 33, 192) and codes.dtype == torch.uint8 and sf.shape == ref[1].shape and sf.dtype == E8M0 and codes.device.type == dev
        src = torch.empty(45, dtype=torch.int32, device=dev)
        codes, sf = q.ops.alloc_quant(q.ops.QUANT_OPS_MXF6["gather_quantize_mxf6"], x[0], h, src)
        assert codes.shape == (45, 192) and codes.dtype == torch.uint8 and sf.numel() >= 45 * 8

    # quantise -> GEMM: the tokens go through fusedGatherQuantizeMxf6 inside the traced function
    def layer(x, h, src, b, b_sf, alpha, offs):
        a, a_sf = q.fusedGatherQuantizeMxf6(x, h, src)
        y = q.grouped_matmul_mxf6_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha, offs)
        a2, a2_sf = q.fusedQuantizeMxf6(y[:, :K], h)
        return q.grouped_matmul_mxf6_mxf4_bf16_tn(a2, b, a2_sf, b_sf, alpha, offs) * 2

    with FakeTensorMode():
        args = (torch.empty(40, K, dtype=torch.bfloat16, device=DEV), torch.empty(32, 32, dtype=torch.bfloat16, device=DEV),
                torch.empty(M, dtype=torch.int32, device=DEV), torch.empty(E, K, K // 2, dtype=torch.uint8, device=DEV),
                torch.empty(E * K * K // 32, dtype=E8M0, device=DEV), torch.empty(1, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))
        out = layer(*args)
        assert out.shape == (M, K) and out.dtype == torch.bfloat16
        gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert targets.count("qutlass_amd.grouped_matmul_mxf6_mxf4.default") == 2, targets
    assert sum("uantize" in t and "xf6" in t for t in targets) == 2, targets


def test_dense_wrapper_traces_without_a_host_sync():
    """the wrapper's offs is made on the device from a.size(0): the trace holds a fill and the grouped op, and nothing that reads a tensor's value on the host"""
    from torch.fx.experimental.proxy_tensor import make_fx

    import qutlass_amd as q

    M, N, K = 48, 64, 256

    def layer(a, b, a_sf, b_sf, alpha):
        return q.matmul_mxf6_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha)

    args = (torch.zeros(M, K * 3 // 4, dtype=torch.uint8), torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(M * K // 32, dtype=torch.uint8).view(E8M0),
            torch.zeros(N * K // 32, dtype=torch.uint8).view(E8M0), torch.ones(1))
    gm = make_fx(layer, tracing_mode="fake")(*args)
    targets = [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]
    assert "qutlass_amd.grouped_matmul_mxf6_mxf4.default" in targets, targets
    assert not any(s in t for t in targets for s in ("item", "_local_scalar_dense", "nonzero", "_to_copy")), targets
    node = next(n for n in gm.graph.nodes if str(n.target) == "qutlass_amd.grouped_matmul_mxf6_mxf4.default")
    assert tuple(node.args[1].meta["val"].shape) == (1, N, K // 2) and tuple(node.args[5].meta["val"].shape) == (1,)
    assert tuple(node.meta["val"].shape) == (M, N)
