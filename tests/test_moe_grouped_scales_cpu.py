"""Per-expert global scales in the NVFP4 MoE quantizers (fusedGatherQuantizeNvGrouped, fusedSiluMulQuantizeNvGrouped) without a GPU: the row -> expert function of the
two kernels run on the CPU (qutlass_amd_debug_group_of_row) against numpy.searchsorted, the two C entries' check chains with dummy addresses -- the single-scale
sibling's chain under the new name, then the three checks the grouped form adds, return code and full qutlass_amd_last_error() text pinned --, the torch ops' fake
kernels and schemas, tracing, and the names.  Nothing here reaches HIP.  The GPU half is tests/test_gpu_moe_grouped_scales.py."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import _lib

DEV = "cuda"
OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it
P31 = 1 << 31
GATHER, GATED = "qutlass_amd_fused_gather_quantize_nv_grouped", "qutlass_amd_fused_silu_mul_quantize_nv_grouped"
ARGS = {GATHER: ("x", "h", "rot", "t", "k", "src_row", "m", "method", "gs", "offs", "e", "out", "sf"),
        GATED: ("x", "h", "rot", "rows", "k", "method", "gs", "offs", "e", "out", "sf")}
NAME = {GATHER: "fusedGatherQuantizeNvGrouped", GATED: "fusedSiluMulQuantizeNvGrouped"}
BASE = dict(x=X, h=X, out=X, sf=X, gs=X, src_row=X, offs=X, rot=32, method=1, rows=4, k=256, t=4, m=4, e=8)


# ---- the row -> expert function ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def group_of_row():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.qutlass_amd_debug_group_of_row
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int]
    return lambda offs, m: fn(offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(offs), int(m))


@pytest.mark.parametrize("E", [1, 2, 63, 64, 65, 1024])
def test_group_of_row_is_the_capped_upper_bound(group_of_row, E):
    rng = np.random.default_rng(E)
    for M, live in ((0, E), (1, E), (40, E), (140, E), (140, max(1, E // 8)), (5000, E)):
        counts = np.zeros(E, dtype=np.int64)
        owners = rng.choice(E, size=live, replace=False)
        counts[owners] = np.bincount(rng.integers(0, live, M), minlength=live)
        for tail in (0, 3):   # tail > 0: offs[E - 1] < M + tail, the rows past it belong to expert E - 1
            offs = np.cumsum(counts).astype(np.int32)
            rows = np.arange(0, M + tail + 3)
            want = np.minimum(E - 1, np.searchsorted(offs, rows, side="right"))
            got = np.array([group_of_row(offs, m) for m in rows])
            assert np.array_equal(got, want), (E, M, live, tail, np.nonzero(got != want)[0][:5])


def test_group_of_row_stays_in_range_on_malformed_offs(group_of_row):
    M = 40
    for seq in ([-5, 2 ** 31 - 1, 3], [M + 9, 0, 0], [7, 3, 20]):
        offs = np.array(seq, dtype=np.int32)
        for m in list(range(-2, M + 3)) + [2 ** 31 - 1, -(2 ** 31)]:
            assert 0 <= group_of_row(offs, m) < 3, (seq, m)
    rng = np.random.default_rng(7)
    for E in (2, 65, 1024):
        offs = rng.integers(-(2 ** 31), 2 ** 31 - 1, E).astype(np.int32)
        for m in rng.integers(-(2 ** 31), 2 ** 31 - 1, 200):
            assert 0 <= group_of_row(offs, int(m)) < E
    fn = ctypes.CDLL(_lib.LIB_PATH).qutlass_amd_debug_group_of_row
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    one = np.zeros(1, dtype=np.int32)
    assert fn(None, 1, 0) == -1 and fn(one.ctypes.data, 0, 0) == -1 and fn(one.ctypes.data, 1025, 0) == -1   # rejected, not read


# ---- the check chains -------------------------------------------------------------------------------------------------------------------------------------------
def expect(entry, a):
    """(return code, message) the entry must give, or None where every check passes (the call would go on to HIP and is never made): the sibling's checks in the
    sibling's order (tests/test_quantize_family_cpu.py states them for the siblings), a null offs with the other null pointers, then E, then the alignment of offs"""
    rot, method, h, x, offs = a["rot"], a["method"], a["h"] or 0, a["x"] or 0, a["offs"] or 0
    rp = max(rot, 32)
    bad = lambda text: (INVALID, f"{NAME[entry]}: {text}")
    if rot not in (16, 32, 64, 128):
        return bad(f"Unsupported rotation size {rot}; expected 16, 32, 64, or 128.")
    if method not in (0, 1):
        return bad(f"invalid method {method}")
    outs_null = not a["h"] or not a["out"] or not a["sf"] or not a["gs"] or not a["offs"]
    if entry == GATED:
        rows, inter = a["rows"], a["k"]
        if rows < 0 or inter <= 0 or rows >= P31 or inter >= P31:
            return bad(f"bad shape ({rows}, 2 * {inter})")
        if inter % rp:
            return bad(f"the gate / up width {inter} must be a multiple of {rp}")
        if x % 16:
            return bad("x must be 16-byte aligned")
        if rows * inter >= 1 << 29:
            return bad(f"x (rows * 2 * inter * 2 = {rows * inter * 4} bytes) must stay below 2 GiB")
        if rows == 0:
            return OK, None
        if not a["x"] or outs_null:
            return bad("null pointer argument")
    else:
        t, k, m, src = a["t"], a["k"], a["m"], a["src_row"] or 0
        if t < 0 or m < 0 or k <= 0 or t >= P31 or m >= P31 or k >= P31:
            return bad(f"bad shape (x ({t}, {k}), {m} indices)")
        if k % rp:
            return bad(f"the row length {k} must be a multiple of {rp}")
        if x % 16 or src % 4:
            return bad("x must be 16-byte aligned (and src_row 4-byte aligned)")
        if t * k >= 1 << 30:
            return bad(f"x (rows * k * 2 = {t * k * 2} bytes) must stay below 2 GiB")
        if m * k >= P31:
            return bad("more than 2^31 elements is not supported")
        if m == 0:
            return OK, None
        if (not a["x"] and t > 0) or not a["src_row"] or outs_null:
            return bad("null pointer argument")
    if rot >= 64 and h % 16:
        return bad("the rotation matrix must be 16-byte aligned for rotation sizes >= 64")
    if not 1 <= a["e"] <= 1024:
        return bad(f"E must be in [1, 1024] (got {a['e']})")
    if offs % 4:
        return bad("offs must be 4-byte aligned")
    return None


def call(entry, a):
    lib = _lib.load()
    rc = getattr(lib, entry)(*[a[n] for n in ARGS[entry]], None)
    return rc, (lib.qutlass_amd_last_error().decode() if rc != OK else None)


POINTERS = [dict(), dict(x=None), dict(h=None), dict(out=None), dict(sf=None), dict(gs=None), dict(src_row=None), dict(offs=None), dict(h=X + 8), dict(x=X + 4),
            dict(src_row=X + 2), dict(offs=X + 2), dict(offs=X + 1, h=X + 2), dict(offs=None, x=X + 4)]
EXPERTS = (8, 1, 1024, 0, -1, 1025, 1 << 40)
SHAPES = {GATED: [dict(rows=r, k=k) for r, k in ((4, 256), (0, 256), (0, 48), (-1, 256), (4, 0), (P31, 256), (4, 48), (4, 32), (1 << 15, 1 << 14), ((1 << 21) - 1, 256))],
          GATHER: [dict(t=t, k=k, m=m) for t, k, m in ((4, 256, 4), (4, 256, 0), (0, 256, 4), (-1, 256, 4), (4, 0, 4), (4, 256, -1), (4, 256, P31), (4, 48, 4), (4, 32, 4),
                                                        (1 << 15, 1 << 15, 4), (4, 1 << 20, 1 << 11), (4, 1 << 20, (1 << 11) - 1))]}


@pytest.mark.parametrize("entry", [GATHER, GATED])
def test_every_check_of_the_entry_in_its_order(entry):
    made = accepted = 0
    seen = set()
    for rot, method, e, shape, ptr in itertools.product((0, 16, 32, 48, 64, 128, 256), (-1, 0, 1, 2), EXPERTS, SHAPES[entry], POINTERS):
        if any(key not in ARGS[entry] for key in ptr):
            continue
        a = {**BASE, **shape, **ptr, "rot": rot, "method": method, "e": e}
        want = expect(entry, a)
        if want is None:
            continue
        assert call(entry, a) == want, (entry, a)
        made += 1
        accepted += want[0] == OK
        seen.add(re.sub(r"-?\d+", "#", (want[1] or "accepted").split(": ", 1)[-1]))
    # every way the chain can end did end some call: the sibling's (9 gated, 10 gathering, the zero-row accept among them) and the two new messages
    assert made >= 2000 and accepted > 0 and len(seen) == {GATED: 9, GATHER: 10}[entry] + 2, (made, sorted(seen))


def _one(entry, **kw):
    return call(entry, {**BASE, **kw})


def test_the_new_checks_come_after_the_siblings_chain():
    for entry, zero in ((GATHER, dict(m=0)), (GATED, dict(rows=0))):
        n = NAME[entry]
        assert _one(entry, e=0) == (INVALID, f"{n}: E must be in [1, 1024] (got 0)")
        assert _one(entry, e=1025) == (INVALID, f"{n}: E must be in [1, 1024] (got 1025)")
        assert _one(entry, e=-3, offs=X + 2) == (INVALID, f"{n}: E must be in [1, 1024] (got -3)")
        assert _one(entry, offs=X + 2) == (INVALID, f"{n}: offs must be 4-byte aligned")
        assert _one(entry, offs=None) == (INVALID, f"{n}: null pointer argument")
        assert _one(entry, offs=None, e=0) == (INVALID, f"{n}: null pointer argument")                       # the pointers before E
        assert _one(entry, e=0, rot=64, h=X + 8) == (INVALID, f"{n}: the rotation matrix must be 16-byte aligned for rotation sizes >= 64")
        assert _one(entry, e=0, method=2) == (INVALID, f"{n}: invalid method 2")
        assert _one(entry, e=0, rot=8) == (INVALID, f"{n}: Unsupported rotation size 8; expected 16, 32, 64, or 128.")
        assert _one(entry, e=0, k=48) == (INVALID, f"{n}: " + ("the row length 48" if entry == GATHER else "the gate / up width 48") + " must be a multiple of 32")
        # zero rows: accepted where the sibling accepts them -- before any pointer, E or offs is looked at -- and for quest as for abs_max
        for method in (0, 1):
            assert _one(entry, **zero, method=method) == (OK, None)
            assert _one(entry, **zero, method=method, x=None, h=None, out=None, sf=None, gs=None, src_row=None, offs=None, e=0) == (OK, None)
    assert _one(GATHER, t=0, x=None, offs=None) == (INVALID, "fusedGatherQuantizeNvGrouped: null pointer argument")
    assert _one(GATHER, t=1 << 15, k=1 << 15, m=0, e=0) == (INVALID, "fusedGatherQuantizeNvGrouped: x (rows * k * 2 = 2147483648 bytes) must stay below 2 GiB")
    assert _one(GATED, rows=1 << 15, k=1 << 14, offs=None) == (INVALID, "fusedSiluMulQuantizeNvGrouped: x (rows * 2 * inter * 2 = 2147483648 bytes) must stay below 2 GiB")


def test_header_exports_and_ctypes_table_agree():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ((GATHER, 14), (GATED, 12)):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        decl = re.search(name + r"\(([^;]*)\);", header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]) == len(ARGS[name]) + 1
        assert "const float* global_scales, const int32_t* offs, int64_t e," in re.sub(r"\s+", " ", decl.group(1))
    assert hasattr(lib, "qutlass_amd_debug_group_of_row") and "qutlass_amd_debug_group_of_row" not in header   # exported for the tests, not part of the interface


# ---- the torch and Python layers --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [70, 140])
def test_fake_kernels_give_the_single_scale_ops_shapes(m):
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    t, k, E = 33, 384, 5
    with FakeTensorMode():
        x = torch.empty(t, k, dtype=torch.bfloat16, device=DEV)
        xg = torch.empty(m, 2 * k, dtype=torch.bfloat16, device=DEV)
        src = torch.empty(m, dtype=torch.int32, device=DEV)
        h = torch.empty(32, 32, dtype=torch.bfloat16, device=DEV)
        gs, one = torch.empty(E, device=DEV), torch.empty(1, device=DEV)
        offs = torch.empty(E, dtype=torch.int32, device=DEV)
        pairs = [(amd.gather_quantize_nv_grouped(x, h, src, gs, offs, 1), amd.gather_quantize_nv(x, h, src, one, 1)),
                 (amd.silu_mul_quantize_nv_grouped(xg, h, gs, offs, 1), amd.silu_mul_quantize_nv(xg, h, one, 1, False)),
                 (q.fusedGatherQuantizeNvGrouped(x, h, gs, src, offs), q.fusedGatherQuantizeNv(x, h, one, src)),
                 (q.fusedGatherQuantizeNvGrouped(x, h, gs, src, offs, method="quest"), q.fusedGatherQuantizeNv(x, h, one, src, method="quest")),
                 (q.fusedSiluMulQuantizeNvGrouped(xg, h, gs, offs), q.fusedSiluMulQuantizeNv(xg, h, one)),
                 (q.fusedSiluMulQuantizeNvGrouped(xg, h, gs, offs, method="quest"), q.fusedSiluMulQuantizeNv(xg, h, one, method="quest"))]
        for got, want in pairs:
            assert [(a.shape, a.dtype, a.device.type) for a in got] == [(a.shape, a.dtype, a.device.type) for a in want]
            assert got[0].shape == (m, k // 2) and got[0].dtype == torch.uint8 and got[1].shape == ((m + 127) // 128 * 128, 24) and got[1].dtype == torch.float8_e4m3fn


def test_in_place_twins_declare_their_two_writes():
    q.ops.register_torch_ops()
    for n in ("fusedGatherQuantizeNvGrouped_", "fusedSiluMulQuantizeNvGrouped_"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert written == ["OUT", "OUT_sf"] and len(schema.returns) == 0, str(schema)
        assert [a.name for a in schema.arguments][-3:] == ["global_scales", "offs", "method"], str(schema)
        assert torch._library.simple_registry.singleton.find(f"qutlass_amd::{n}").fake_impl.kernel is not None
    for n in ("gather_quantize_nv_grouped", "silu_mul_quantize_nv_grouped"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments) and len(schema.returns) == 2, str(schema)
        assert n in q.ops.QUANT_OPS and "Tensor global_scales, Tensor offs" in q.ops.QUANT_OPS[n].schema


def test_the_two_functions_trace_with_fullgraph():
    E, H, I, T, topk = 4, 256, 128, 35, 2

    def layer(x, logits, h, a13_gs, a2_gs, w13q, w13s, w2q, w2s, alpha13, alpha2):
        w, ids, src_row, offs, pos = q.moe_route(logits, topk)
        aq, asf = q.fusedGatherQuantizeNvGrouped(x, h, a13_gs, src_row, offs)
        gate_up = q.grouped_matmul_nvf4_bf16_tn(aq, w13q, asf, w13s, alpha13, offs)
        bq, bsf = q.fusedSiluMulQuantizeNvGrouped(gate_up, h, a2_gs, offs)
        y = q.grouped_matmul_nvf4_bf16_tn(bq, w2q, bsf, w2s, alpha2, offs)
        return q.moe_combine(y, pos, w)

    with FakeTensorMode():
        args = (torch.empty(T, H, dtype=torch.bfloat16, device=DEV), torch.empty(T, E, device=DEV), torch.empty(32, 32, dtype=torch.bfloat16, device=DEV),
                torch.empty(E, device=DEV), torch.empty(E, device=DEV),
                torch.empty(E, 2 * I, H // 2, dtype=torch.uint8, device=DEV), torch.empty(E * 2 * I * H // 16, dtype=torch.float8_e4m3fn, device=DEV),
                torch.empty(E, H, I // 2, dtype=torch.uint8, device=DEV), torch.empty(E * H * I // 16, dtype=torch.float8_e4m3fn, device=DEV),
                torch.empty(E, device=DEV), torch.empty(E, device=DEV))
        out = torch.compile(layer, backend="eager", fullgraph=True)(*args)
        assert out.shape == (T, H) and out.dtype == torch.bfloat16
        for fn, fargs in ((q.fusedGatherQuantizeNvGrouped, (args[0], args[2], args[3], torch.empty(70, dtype=torch.int32, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))),
                          (q.fusedSiluMulQuantizeNvGrouped, (torch.empty(70, 2 * I, dtype=torch.bfloat16, device=DEV), args[2], args[3], torch.empty(E, dtype=torch.int32, device=DEV)))):
            for method in ("abs_max", "quest"):
                c, s = torch.compile(lambda *a, _fn=fn, _m=method: _fn(*a, method=_m), backend="eager", fullgraph=True)(*fargs)
                assert c.shape == (70, (H if fn is q.fusedGatherQuantizeNvGrouped else I) // 2) and s.dtype == torch.float8_e4m3fn


def test_names_and_wrapper_errors():
    import qutlass

    for n in ("fusedGatherQuantizeNvGrouped", "fusedSiluMulQuantizeNvGrouped"):
        assert getattr(qutlass, n) is getattr(q, n) and getattr(q, n).__doc__
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    h = torch.zeros(32, 32, dtype=torch.bfloat16)
    gs, offs, src = torch.ones(2), torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    for fn in (lambda: q.fusedGatherQuantizeNvGrouped(x, h, gs, src, offs, method="nope"), lambda: q.fusedSiluMulQuantizeNvGrouped(x, h, gs, offs, method="nope")):
        with pytest.raises(ValueError, match="invalid method 'nope', must be 'quest' or 'abs_max'"):
            fn()
    with pytest.raises(ValueError, match="the last dimension of x must be 2 \\* I"):
        q.fusedSiluMulQuantizeNvGrouped(torch.zeros(4, 127, dtype=torch.bfloat16), h, gs, offs)
