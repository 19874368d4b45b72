"""MX GEMMs beyond the narrow data every other GPU file feeds them (tests/_mx_cases.py: the forms, their shapes and the operand builders; tests/test_mx_scale_range_cpu.py
checks the data itself with the oracle alone).  Every kernel form the product's plans can return -- MXFP4 / MXFP8 TN with e4m3 and e5m2 A, split-K through the _ws entries,
the row-major-scale op, both operand paths of the NN op, the grouped forms with offs[-1] == M -- forced through the lab library's C entries:

  1. scale bytes over the whole e8m0 range 0 ... 254 with ordinary block products: byte equality with the oracle;
  2. scale byte 255 (NaN) as a tracer: isnan(D) is exactly the predicted row / column pattern over the whole output, every other element equals the oracle;
  3. fp8 special operand codes (e4m3 NaN, e5m2 +-inf / NaN): the oracle's NaN / +-inf pattern over the whole output, every other element byte-equal (exact-regime codes,
     so the MXFP8 tolerance of the neighbouring files is not needed);
  5. read independence: bytes around the operands and around the blocked scale images (0xff against 0x00), and finite bytes in the scale columns past K, never reach D.

Every call here also runs inside the guards of part 4 (tests/test_gpu_gemm_footprint.py): D between sentinel rows, the workspace before a sentinel tail.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402,F401  (the checker, through _mx_cases)
import _benchlib as lab  # noqa: E402,F401  (the LAB library: forced forms)
import _mx_cases as mc  # noqa: E402

IDS = lambda c: c.id   # noqa: E731


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _run_and_compare(c, part):
    d = mc.dataset(c, part)
    r = mc.run(c, d)
    mc.assert_footprint(r)
    mc.assert_equals_reference(r.out, d.ref)
    return d, r


@pytest.mark.parametrize("layout", ["sweep", "extremes"])
@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_whole_e8m0_byte_range_equals_the_oracle(q, c, layout):
    d, r = _run_and_compare(c, layout)
    assert not mc.isnan_bf16(r.out).any()


@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_nan_scale_bytes_poison_exactly_their_rows_and_columns(q, c):
    d, r = _run_and_compare(c, "nan")
    assert np.array_equal(mc.isnan_bf16(r.out), mc.nan_pattern(c))


@pytest.mark.parametrize("c", mc.FP8_CASES, ids=IDS)
def test_fp8_special_operand_codes_propagate_as_in_the_oracle(q, c):
    d, r = _run_and_compare(c, "special")
    assert mc.isnan_bf16(r.out)[2].all() and mc.isnan_bf16(r.out)[c.m - 1].all()
    if c.a5:
        assert ((r.out[17] & 0x7FFF) >= 0x7F80).all() and ((r.out[40] & 0x7FFF) == 0x7F80).sum() > c.n // 2


@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_bytes_around_the_operands_never_reach_the_output(q, c):
    d = mc.dataset(c, "plain")
    zero, ones = mc.run(c, d, fill=0x00), mc.run(c, d, fill=0xFF)
    mc.assert_footprint(ones)
    assert np.array_equal(zero.out, ones.out), f"{int((zero.out != ones.out).sum())} outputs depend on bytes outside the operands"
    mc.assert_equals_reference(ones.out, d.ref)


def _with_k(c, k):
    return c._replace(k=k)


PAST_K = [_with_k(c, c.k + extra) for c in mc.CASES if c.op in ("mxf8", "nn") and c.k % 128 == 32 and c.k < 2000 for extra in (0, 32, 64)]


@pytest.mark.parametrize("c", PAST_K, ids=IDS)
def test_finite_scale_bytes_past_k_contribute_nothing(q, c):
    """K % 128 == 32 / 64 / 96: the blocked image's last 4-column block has columns past K, zero by to_blocked's definition -- random finite bytes there give the same D"""
    d = mc.dataset(c, "plain")
    zero, rand = mc.run(c, d), mc.run(c, d, past_k=np.random.default_rng(c.k))
    assert np.array_equal(zero.out, rand.out), f"{int((zero.out != rand.out).sum())} outputs depend on scale bytes past K"
    mc.assert_equals_reference(zero.out, d.ref)
