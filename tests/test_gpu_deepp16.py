"""The one-tile form of the persistent MXFP4 256x256 kernel on the 16x16x128 scaled MFMA (csrc/gemm_mx_deepp16.hip.h).

Through the lab library with the form forced ("gemm_variant" 191; 190 forces the 32x32x64 one-tile form, so small grids reach either): byte equality with the oracle
and with the 32x32x64 form on quantised random operands -- one tile with two stages (no steady-state loop), four stages, several tiles, ragged M / N % 8 / a K tail
inside an even stage count, one row, a 40-tile grid (every XCD share of the remap runs), alpha = 0.37; the per-lane scale-byte selection over the whole e8m0 range and
with the NaN byte 255 as a tracer in single rows and K blocks; the footprint (D between sentinel rows, the operand buffers and what lies around them byte-identical
after the call, nothing around them ever read).  Through the product: the smallest shape its rule sends to the one-tile form.

Operands, oracle references and the guarded call are those of tests/_mx_cases.py (shared with tests/test_gpu_mx_scale_range.py).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
import _benchlib as lab  # noqa: E402
import _mx_cases as mc  # noqa: E402

F16, F32 = 191, 190   # "gemm_variant": the one-tile form on 16x16x128 / 32x32x64 MFMAs
SHAPES = [(256, 256, 512), (256, 256, 1024), (512, 768, 1536), (257, 264, 896), (1, 8, 512), (1280, 2048, 512)]
RAGGED = (257, 264, 896)
DEV = "cuda:0"


def _case(variant, shape):
    return mc.Case("mxf4", False, variant, (), *shape)


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def test_forced_forms_are_one_tile_launches_of_an_even_stage_count():
    """what makes 190 / 191 reach the one-tile kernels: at most 256 tiles (grid == tile count) and an even number of 128-byte K stages (or one, which runs as two)"""
    assert -(-1280 // 256) * -(-2048 // 256) == 40
    for m, n, k in SHAPES:
        kt = -(-(k // 2) // 128)
        assert -(-m // 256) * -(-n // 256) <= 256 and (kt % 2 == 0 or kt == 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_oracle_and_the_32x32x64_form(q, shape):
    c = _case(F16, shape)
    d = mc.dataset(c, "plain")
    r16, r32 = mc.run(c, d), mc.run(_case(F32, shape), d)
    mc.assert_footprint(r16)
    mc.assert_equals_reference(r16.out, d.ref)
    assert np.array_equal(r16.out, r32.out), f"{int((r16.out != r32.out).sum())} outputs differ between the two MFMA shapes"


def test_alpha_that_is_no_power_of_two(q):
    c = _case(F16, RAGGED)
    d = mc.dataset(c, "plain")
    d = d._replace(alpha=0.37, ref=mc._reference(c, d.a, d.b, d.sa, d.sb, 0.37))
    r16, r32 = mc.run(c, d), mc.run(_case(F32, RAGGED), d)
    mc.assert_equals_reference(r16.out, d.ref)
    assert np.array_equal(r16.out, r32.out)


@pytest.mark.parametrize("layout", ["sweep", "extremes"])
def test_scale_bytes_over_the_whole_e8m0_range(q, layout):
    """bytes 0, 1, ... 254 in adjacent K blocks of single rows: a lane that took another K block's byte of its row's dword is off by a power of two"""
    c = _case(F16, RAGGED)
    d = mc.dataset(c, layout)
    r = mc.run(c, d)
    mc.assert_footprint(r)
    mc.assert_equals_reference(r.out, d.ref)
    assert not mc.isnan_bf16(r.out).any()


@pytest.mark.parametrize("shape", [RAGGED, (512, 768, 1536)], ids=lambda s: "x".join(map(str, s)))
def test_nan_scale_byte_reaches_exactly_its_rows_and_columns(q, shape):
    c = _case(F16, shape)
    d = mc.dataset(c, "nan")
    r = mc.run(c, d)
    mc.assert_footprint(r)
    mc.assert_equals_reference(r.out, d.ref)
    assert np.array_equal(mc.isnan_bf16(r.out), mc.nan_pattern(c))


def test_footprint(q, monkeypatch):
    """D between untouched sentinel rows; A, B, both scale images and the 4 KiB before / the tile of rows behind each byte-identical after the call; what surrounds
    them (0x00 against 0xff = NaN scale bytes) never reaches the output"""
    made = []

    class Spy(mc.Embedded):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append((self, self.buf.clone()))

    monkeypatch.setattr(mc, "Embedded", Spy)
    c = _case(F16, RAGGED)
    d = mc.dataset(c, "plain")
    zero, ones = mc.run(c, d, fill=0x00), mc.run(c, d, fill=0xFF)
    assert len(made) == 8
    for e, before in made:
        assert torch.equal(e.buf, before), "an operand buffer was written"
    mc.assert_footprint(zero)
    mc.assert_footprint(ones)
    assert np.array_equal(zero.out, ones.out), f"{int((zero.out != ones.out).sum())} outputs depend on bytes outside the operands"
    mc.assert_equals_reference(ones.out, d.ref)


def test_smallest_shape_the_product_sends_to_the_one_tile_form(q):
    """3584 x 3584 x 512: 196 tiles (>= 3/4 of the CUs) on 196 workgroups, two K stages -- plan 90 by the dry-run hook; sampled rows against the oracle, the whole
    output against both forced forms"""
    from qutlass_amd.utils import to_blocked

    m = n = 3584
    k = 512
    f = q._lib.load().qutlass_amd_debug_gemm_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    out = (ctypes.c_int * 24)()
    assert f(4, m, n, k, 0, out, 8) == 1 and (out[0], out[1], out[2]) == (90, n, 1)
    torch.manual_seed(16)
    h = torch.tensor([[1.0]], device=DEV)
    for _ in range(5):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    h = (h / 32 ** 0.5).to(torch.bfloat16)
    a = torch.randn(m, k, dtype=torch.bfloat16, device=DEV) * 25.0
    b = torch.randn(n, k, dtype=torch.bfloat16, device=DEV) * 25.0
    a_q, a_s = q.fusedQuantizeMx(a, h, method="abs_max")
    b_q, b_s = q.fusedQuantizeMx(b, h, method="abs_max")
    asf, bsf, alpha = to_blocked(a_s), to_blocked(b_s), torch.tensor([1.0], device=DEV)
    got = q.matmul_mxf4_bf16_tn(a_q, b_q, asf, bsf, alpha)
    rows = torch.cat([torch.arange(0, 3), torch.arange(255, 258), torch.arange(m - 3, m), torch.randperm(m)[:39]]).unique()
    npy = lambda t: t.detach().cpu().contiguous().view(torch.uint8).numpy()   # noqa: E731
    ref = oracle.gemm_blockscaled(oracle.KIND_MXFP4, npy(a_q[rows.to(DEV)]), npy(b_q), oracle.to_blocked(npy(a_s)[rows.numpy()]), oracle.to_blocked(npy(b_s)), 1.0,
                                  len(rows), n, k)
    assert np.array_equal(npy(got[rows.to(DEV)]).view(np.uint16).reshape(len(rows), n), ref)
    for variant in (F16, F32):
        with lab.forced(gemm_variant=variant):
            assert torch.equal(lab.matmul_mxf4_bf16_tn(a_q, b_q, asf, bsf, alpha), got), variant
