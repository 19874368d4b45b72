"""The MXFP8 rotate-and-quantize ops without a GPU: (1) the numpy model of their contract (tests/_mxf8_quant_model.py) against the two pinned oracle functions that
state the same rule, (2) the argument checks of the four C entries, which all come before any launch (dummy addresses only, as in tests/test_quantize_family_cpu.py),
(3) the fake kernels: every wrapper traces with the right shapes and dtypes.  The GPU half is tests/test_gpu_mxf8_quantize.py."""
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import oracle
import qutlass_amd as q
from qutlass_amd import _lib
from qutlass_amd.utils import get_padded_shape_mx

import _mxf8_quant_model as model

OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it
P31 = 1 << 31
DTYPES = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _bf16_bits(v: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.bfloat16).view(torch.uint16).numpy()


def planted(groups: int, seed: int) -> np.ndarray:
    """(groups, 32) bf16 bit patterns: values of magnitude below 2^k around one planted maximum +-m 2^k per group, m in {1, 1.25, 1.5, 1.75}, k in [-8, 8] -- log2 of
    such a maximum lies at least 0.19 below the next integer, far from where the oracle's bf16 rounding of log2(amax) could lift it into the next binade (that quirk,
    at mantissas >= 1 + 123/128, is deliberately not part of the contract), so no group needs excluding"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-8, 9, size=(groups, 1))
    v = rng.uniform(-1, 1, size=(groups, 32)) * 0.999
    v[np.arange(groups), rng.integers(0, 32, size=groups)] = rng.choice([1.0, 1.25, 1.5, 1.75], size=groups) * rng.choice([-1.0, 1.0], size=groups)
    return _bf16_bits(np.ldexp(v, k))


# ---- 1. the model against the pinned oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_model_equals_pseudoquant_mxfp8_on_planted_maxima(fmt):
    x = planted(384, 11).reshape(12, 1024)
    want_q, want_s = oracle.pseudoquant_mxfp8(x, e5m2=fmt == "e5m2")
    got_q, got_s = model.quantize(model.bf16_to_f64(x), fmt)
    print(f"{fmt}: {int((got_s != want_s).sum())} of {want_s.size} scales and {int((got_q != want_q).sum())} of {want_q.size} codes differ, "
          f"{np.unique(got_q).size} distinct codes, scale bytes {int(got_s.min())} .. {int(got_s.max())}")
    assert want_q.size == 12288 and want_s.size == 384
    assert np.array_equal(got_s, want_s) and np.array_equal(got_q, want_q)
    # the planting exercises the encoder and the scale rule, not one corner of them: half (e4m3) / a quarter (e5m2, 4 codes per binade) of the 256 codes, 15 scale bytes
    assert np.unique(got_q).size >= (128 if fmt == "e4m3" else 64) and np.unique(got_s).size >= 15


def test_model_equals_square_double_mxfp8_on_block_constant_maxima():
    """every row of a 32 x 32 block holds the block's maximum: the row-wise groups of 32 then have the block's scale, and e8m0_shift7 is this rule"""
    rng = np.random.default_rng(12)
    m, n = 64, 256
    bm, bn = m // 32, n // 32
    f = rng.uniform(-1, 1, size=(bm, 32, bn, 32)) * 0.999                               # (block row, row, block column, column)
    peak = rng.choice([1.0, 1.25, 1.5, 1.75], size=(bm, 1, bn)) * rng.choice([-1.0, 1.0], size=(bm, 32, bn))
    r, i, c = np.meshgrid(np.arange(bm), np.arange(32), np.arange(bn), indexing="ij")
    f[r, i, c, rng.integers(0, 32, size=(bm, 32, bn))] = peak                           # one planted +-m per row of every block, m the block's
    x = _bf16_bits(np.ldexp(f, rng.integers(-8, 9, size=(bm, 1, bn, 1))).reshape(m, n))   # times the block's 2^k
    want_y, want_rs, _ = oracle.backward_bf16_square_double_mxfp8(x)
    got_q, got_s = model.quantize(model.bf16_to_f64(x), "e4m3")
    assert np.array_equal(got_s, want_rs) and np.array_equal(got_q, want_y)
    assert np.unique(want_rs).size >= 8


def test_model_edge_rows():
    z = np.zeros(32, dtype=np.float32)
    for fmt in ("e4m3", "e5m2"):
        codes, e8 = model.quantize(z, fmt)
        assert e8.tolist() == [127] and not codes.any()
        y = z.copy(); y[3] = -0.0; y[5] = np.nan
        codes, e8 = model.quantize(y, fmt)
        assert e8.tolist() == [127] and codes[3] == 0x80 and np.isnan(model.decode(codes, fmt)[5])
        y = z.copy(); y[0] = 2.0 ** -125
        assert model.quantize(y, fmt)[1].tolist() == [0]                                       # the clamp at 0
        y = z.copy(); y[0] = np.float32(2.0 ** 127 * (2 - 2.0 ** -7))                           # bf16 0x7f7f
        codes, e8 = model.quantize(y, fmt)
        assert e8.tolist() == [254 - model.SH[fmt]] and model.decode(codes, fmt)[0] == (256.0 if fmt == "e4m3" else 2.0 ** 15)   # [128, 256) rounds up to 256: no saturation
    assert oracle.e4m3_decode(0x7e) == 448.0 and oracle.e5m2_decode(0x7b) == 57344.0


# ---- 2. the C entries' checks, all before any launch ------------------------------------------------------------------------------------------------------------
ENTRIES = {
    "qutlass_amd_fused_quantize_mxf8": ("x", "h", "rot", "numel", "fmt", "out", "sf"),
    "qutlass_amd_fused_quantize_mxf8_blocked": ("x", "h", "rot", "rows", "k", "fmt", "out", "sf"),
    "qutlass_amd_fused_silu_mul_quantize_mxf8": ("x", "h", "rot", "rows", "k", "fmt", "blocked", "out", "sf"),
    "qutlass_amd_fused_gather_quantize_mxf8": ("x", "h", "rot", "t", "k", "src_row", "m", "fmt", "out", "sf"),
}
PLAIN, BLOCKED, GATED, GATHER = ENTRIES
BASE = dict(x=X, h=X, out=X, sf=X, src_row=X, rot=32, fmt=0, blocked=0, numel=1024, rows=4, k=256, t=4, m=4)


def _one(entry, **kw):
    lib = _lib.load()
    a = {**BASE, **kw}
    rc = getattr(lib, entry)(*[a[n] for n in ENTRIES[entry]], None)
    return rc, (lib.qutlass_amd_last_error().decode() if rc != OK else None)


def test_the_entries_are_declared_everywhere():
    lib = _lib.load()
    for name, args in ENTRIES.items():
        assert hasattr(lib, name) and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == len(args) + 1, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    for name, args in ENTRIES.items():
        decl = re.search(name + r"\(([^)]*)\);", header)
        assert decl is not None and len(decl.group(1).split(",")) == len(args) + 1, name


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers(entry):
    name = {PLAIN: "fusedQuantizeMxf8", BLOCKED: "fusedQuantizeMxf8Blocked", GATED: "fusedSiluMulQuantizeMxf8", GATHER: "fusedGatherQuantizeMxf8"}[entry]
    for ptr in ("x", "h", "out", "sf") + (("src_row",) if entry == GATHER else ()):
        assert _one(entry, **{ptr: None}) == (INVALID, f"{name}: null pointer argument"), ptr


@pytest.mark.parametrize("entry", ENTRIES)
def test_rotation_and_format_are_rejected_by_name(entry):
    name = {PLAIN: "fusedQuantizeMxf8", BLOCKED: "fusedQuantizeMxf8Blocked", GATED: "fusedSiluMulQuantizeMxf8", GATHER: "fusedGatherQuantizeMxf8"}[entry]
    for rot in (16, 48, 0, 256):
        assert _one(entry, rot=rot, numel=rot * 96 or 96) == (INVALID, f"{name}: Unsupported rotation size {rot}; expected 32, 64, or 128."), rot
    want = "0 (e4m3)" if entry == GATED else "0 (e4m3) or 1 (e5m2)"
    for fmt in (2, -1) + ((1,) if entry == GATED else ()):
        assert _one(entry, fmt=fmt) == (INVALID, f"{name}: invalid fmt {fmt}; expected {want}"), fmt
    if entry == GATED:
        assert _one(entry, fmt=2, blocked=1) == (INVALID, "fusedSiluMulQuantizeMxf8Blocked: invalid fmt 2; expected 0 (e4m3)")


def test_shape_checks_in_the_family_words():
    assert _one(PLAIN, numel=1000) == (INVALID, "fusedQuantizeMxf8: A must be divisible by 32")
    assert _one(PLAIN, rot=64, numel=96) == (INVALID, "fusedQuantizeMxf8: A must be divisible by 64")
    assert _one(PLAIN, numel=0) == (INVALID, "fusedQuantizeMxf8: A must be divisible by 32")
    assert _one(PLAIN, numel=P31) == (INVALID, "fusedQuantizeMxf8: more than 2^31 elements is not supported")
    assert _one(PLAIN, numel=P31, fmt=2) == (INVALID, "fusedQuantizeMxf8: more than 2^31 elements is not supported")     # the size before the format, as before the method
    assert _one(BLOCKED, rows=0) == (INVALID, "fusedQuantizeMxf8Blocked: bad shape (0, 256)")
    assert _one(BLOCKED, rot=64, k=96, rows=2) == (INVALID, "fusedQuantizeMxf8Blocked: the row length 96 must be a multiple of the rotation size 64 and divide numel")
    assert _one(BLOCKED, rot=128, k=192, rows=2) == (INVALID, "fusedQuantizeMxf8Blocked: the row length 192 must be a multiple of the rotation size 128 and divide numel")
    assert _one(BLOCKED, rows=1 << 20, k=1 << 11) == (INVALID, "fusedQuantizeMxf8Blocked: more than 2^31 elements is not supported")
    assert _one(GATED, k=48) == (INVALID, "fusedSiluMulQuantizeMxf8: the gate / up width 48 must be a multiple of 32")
    assert _one(GATED, rot=64, k=96) == (INVALID, "fusedSiluMulQuantizeMxf8: the gate / up width 96 must be a multiple of 64")
    assert _one(GATED, rows=1 << 15, k=1 << 14) == (INVALID, "fusedSiluMulQuantizeMxf8: x (rows * 2 * inter * 2 = 2147483648 bytes) must stay below 2 GiB")
    assert _one(GATED, rows=(1 << 21) - 1, k=256, h=None) == (INVALID, "fusedSiluMulQuantizeMxf8: null pointer argument")     # one row below the limit: the chain goes on
    assert _one(GATED, rows=0, x=None, h=None, out=None, sf=None) == (OK, None)
    assert _one(GATHER, k=48) == (INVALID, "fusedGatherQuantizeMxf8: the row length 48 must be a multiple of 32")
    assert _one(GATHER, t=1 << 15, k=1 << 15) == (INVALID, "fusedGatherQuantizeMxf8: x (rows * k * 2 = 2147483648 bytes) must stay below 2 GiB")
    assert _one(GATHER, k=1 << 20, m=1 << 11) == (INVALID, "fusedGatherQuantizeMxf8: more than 2^31 elements is not supported")
    assert _one(GATHER, m=0, h=None, src_row=None, out=None, sf=None) == (OK, None)
    assert _one(GATHER, t=-1) == (INVALID, "fusedGatherQuantizeMxf8: bad shape (x (-1, 256), 4 indices)")


def test_misaligned_pointers():
    for entry, name in ((PLAIN, "fusedQuantizeMxf8"), (BLOCKED, "fusedQuantizeMxf8Blocked"), (GATED, "fusedSiluMulQuantizeMxf8"), (GATHER, "fusedGatherQuantizeMxf8")):
        for rot in (64, 128):
            got = _one(entry, rot=rot, h=X + 8, numel=rot * 32)
            assert got == (INVALID, f"{name}: the rotation matrix must be 16-byte aligned for rotation sizes >= 64"), (entry, rot)
    assert _one(GATED, x=X + 4) == (INVALID, "fusedSiluMulQuantizeMxf8: x must be 16-byte aligned")
    assert _one(GATHER, x=X + 4) == (INVALID, "fusedGatherQuantizeMxf8: x must be 16-byte aligned (and src_row 4-byte aligned)")
    assert _one(GATHER, src_row=X + 2) == (INVALID, "fusedGatherQuantizeMxf8: x must be 16-byte aligned (and src_row 4-byte aligned)")


# ---- 3. tracing -----------------------------------------------------------------------------------------------------------------------------------------------
def _expect(codes, sf, operand_shape, dtype, blocked):
    probe = torch.empty(operand_shape, device="meta")
    pr, pc = get_padded_shape_mx(probe)
    assert tuple(codes.shape) == tuple(operand_shape) and codes.dtype == dtype and codes.device.type == "cuda", (codes.shape, codes.dtype)
    assert tuple(sf.shape) == ((pr * pc,) if blocked else (pr, pc)) and sf.dtype == torch.float8_e8m0fnu and sf.device.type == "cuda", (sf.shape, sf.dtype)


@pytest.mark.parametrize("compiled", [False, True])
def test_every_wrapper_traces_with_the_right_shapes_and_dtypes(compiled):
    wrap = (lambda fn: torch.compile(fn, backend="eager", fullgraph=True)) if compiled else (lambda fn: fn)
    with FakeTensorMode():
        for R in (32, 128):
            x = torch.empty(2, 35, 768, dtype=torch.bfloat16, device="cuda")
            x2 = x.view(-1, 768)
            h = torch.empty(R, R, dtype=torch.bfloat16, device="cuda")
            src = torch.empty(45, dtype=torch.int32, device="cuda")
            for fmt, dt in DTYPES.items():
                _expect(*wrap(lambda a, b: q.fusedQuantizeMxf8(a, b, dtype=dt))(x, h), (2, 35, 768), dt, False)
                _expect(*wrap(lambda a, b: q.fusedQuantizeMxf8Blocked(a, b, dtype=dt))(x, h), (2, 35, 768), dt, True)
                _expect(*wrap(lambda a, b, s: q.fusedGatherQuantizeMxf8(a, b, s, dtype=dt))(x2, h, src), (45, 768), dt, False)
            _expect(*wrap(q.fusedQuantizeMxf8)(x, h), (2, 35, 768), torch.float8_e4m3fn, False)   # the default dtype
            _expect(*wrap(q.fusedSiluMulQuantizeMxf8)(x, h), (2, 35, 384), torch.float8_e4m3fn, False)
            _expect(*wrap(q.fusedSiluMulQuantizeMxf8Blocked)(x, h), (2, 35, 384), torch.float8_e4m3fn, True)


def test_the_twins_declare_their_writes_and_the_functional_forms_none():
    q.ops.register_torch_ops()
    for n in ("fusedQuantizeMxf8_", "fusedQuantizeMxf8Blocked_", "fusedSiluMulQuantizeMxf8_", "fusedGatherQuantizeMxf8_"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert written == ["OUT", "OUT_sf"] and len(schema.returns) == 0, str(schema)
        assert n in {row.twin for row in q.ops.QUANT_OPS.values()}
    for n in ("quantize_mxf8", "quantize_mxf8_blocked", "silu_mul_quantize_mxf8", "gather_quantize_mxf8"):
        schema = getattr(torch.ops.qutlass_amd, n).default._schema
        assert not any(a.alias_info is not None for a in schema.arguments) and len(schema.returns) == 2, str(schema)


def test_the_quantizer_feeds_the_grouped_gemm_in_a_traced_graph():
    def layer(x, h, src, w, w_sf, alpha, offs):
        a, a_sf = q.fusedGatherQuantizeMxf8(x, h, src, dtype=torch.float8_e5m2)
        return q.grouped_matmul_mxf8_bf16_tn(a, w, a_sf, w_sf, alpha, offs)

    with FakeTensorMode():
        x = torch.empty(7, 256, dtype=torch.bfloat16, device="cuda")
        h = torch.empty(64, 64, dtype=torch.bfloat16, device="cuda")
        src = torch.empty(37, dtype=torch.int32, device="cuda")
        w = torch.empty(3, 64, 256, dtype=torch.float8_e4m3fn, device="cuda")
        w_sf = torch.empty(3 * 64 * 8, dtype=torch.float8_e8m0fnu, device="cuda")
        out = torch.compile(layer, backend="eager", fullgraph=True)(x, h, src, w, w_sf, torch.empty(1, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda"))
        assert out.shape == (37, 64) and out.dtype == torch.bfloat16


def test_the_wrappers_refuse_a_bad_dtype_by_name():
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    h = torch.zeros(32, 32, dtype=torch.bfloat16)
    src = torch.zeros(4, dtype=torch.int32)
    for fn, args in ((q.fusedQuantizeMxf8, (x, h)), (q.fusedQuantizeMxf8Blocked, (x, h)), (q.fusedGatherQuantizeMxf8, (x, h, src))):
        with pytest.raises(ValueError) as e:
            fn(*args, dtype=torch.float16)
        assert str(e.value) == "invalid dtype torch.float16, must be torch.float8_e4m3fn or torch.float8_e5m2", fn.__name__
    import qutlass
    for n in ("fusedQuantizeMxf8", "fusedQuantizeMxf8Blocked", "fusedGatherQuantizeMxf8", "fusedSiluMulQuantizeMxf8", "fusedSiluMulQuantizeMxf8Blocked"):
        assert getattr(qutlass, n) is getattr(q, n), n
