"""NVFP4 GEMMs beyond the narrow scale bytes every other GPU file feeds them (tests/_nv_cases.py: the forms, their shapes and the operand builders;
tests/test_nv_scale_range_cpu.py checks the data itself with the oracle alone).  Every kernel form the product's plans can return -- the skinny split-K kernel, the
wave-owned forms, the persistent and the per-tile 256x256 kernel, the 256x128 / 128x128 / 128x64 / 64x64 tiles in one pass and split over caller scratch with every
reduce instantiation, the four grouped forms with offs[-1] == M -- forced through the lab library's C entries:

  1. scale bytes over the whole finite e4m3 range, both signs, subnormals and zero, on either operand, with ordinary block products: byte equality with the oracle
     (the sign bit of a scale is the oracle's reading of e4m3: no reference vector exists for it and fusedQuantizeNv never emits it);
  2. the scale bytes 0x7f and 0xff (NaN) as tracers: isnan(D) is exactly the predicted row / column pattern over the whole output, every other element equals the oracle;
  3. read independence: bytes around the operands and around the scale images (0xff, a NaN scale, against 0x00), and finite bytes in the scale columns past K, never reach D;
  4. the product library, whose rule picks the form, returns the bits of the form its plan names.

Every call runs inside the guards of tests/test_gpu_gemm_footprint.py: D between sentinel rows, the workspace before a sentinel tail.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402,F401  (the checker, through _nv_cases)
import _benchlib as lab  # noqa: E402,F401  (the LAB library: forced forms)
import _nv_cases as nc  # noqa: E402

IDS = lambda c: c.id   # noqa: E731


@pytest.fixture(scope="module")
def q():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import qutlass_amd

    return qutlass_amd


def _check(c, r):
    nc.assert_footprint(r)
    if c.splits > 1:
        assert r.ws_bytes > 0


def _run_and_compare(c, part, walk_a=True):
    d = nc.dataset(c, part, walk_a)
    r = nc.run(c, d)
    _check(c, r)
    nc.assert_equals_reference(r.out, nc.reference(c, part, walk_a))
    return d, r


@pytest.mark.parametrize("walk_a", [True, False], ids=["a-walks", "b-walks"])
@pytest.mark.parametrize("layout", ["sweep", "extremes"])
@pytest.mark.parametrize("c", nc.CASES, ids=IDS)
def test_whole_e4m3_byte_range_equals_the_oracle(q, c, layout, walk_a):
    d, r = _run_and_compare(c, layout, walk_a)
    assert not nc.isnan_bf16(r.out).any()


@pytest.mark.parametrize("c", nc.CASES, ids=IDS)
def test_nan_scale_bytes_poison_exactly_their_rows_and_columns(q, c):
    d, r = _run_and_compare(c, "nan")
    assert np.array_equal(nc.isnan_bf16(r.out), nc.nan_pattern(c))


@pytest.mark.parametrize("c", nc.CASES, ids=IDS)
def test_bytes_around_the_operands_never_reach_the_output(q, c):
    d = nc.dataset(c, "plain")
    zero, ones = nc.run(c, d, fill=0x00), nc.run(c, d, fill=0xFF)
    _check(c, zero)
    _check(c, ones)
    assert np.array_equal(zero.out, ones.out), f"{int((zero.out != ones.out).sum())} outputs depend on bytes outside the operands"
    nc.assert_equals_reference(ones.out, nc.reference(c, "plain"))


PAST_K = [c for c in nc.CASES if c.op == "nv" and c.k % 64]


@pytest.mark.parametrize("c", PAST_K, ids=IDS)
def test_finite_scale_bytes_past_k_contribute_nothing(q, c):
    """K % 64 == 32: the blocked image's last 4-column block has two columns past K, zero by to_blocked's definition -- random finite bytes there give the same D"""
    d = nc.dataset(c, "plain")
    zero, rand = nc.run(c, d), nc.run(c, d, past_k=np.random.default_rng(c.k))
    _check(c, rand)
    assert np.array_equal(zero.out, rand.out), f"{int((zero.out != rand.out).sum())} outputs depend on scale bytes past K"
    nc.assert_equals_reference(zero.out, nc.reference(c, "plain"))


PRODUCT_SHAPES = [(7, 120, 2016), (37, 40, 4064), (37, 120, 2176), (83, 200, 2432), (83, 200, 8736), (147, 168, 2432), (147, 168, 8160), (211, 72, 4640),
                  (275, 296, 2432), (275, 168, 5088), (531, 552, 2304), (531, 552, 2464)]


def test_product_rule_reaches_each_form_with_the_same_bits(q):
    from qutlass_amd import _lib

    product = _lib.load()
    plan = product.qutlass_amd_debug_nvf4_plan
    plan.restype = ctypes.c_int
    plan.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int]
    assert product.qutlass_amd_set_option(b"nvf4_variant", 5) == -1          # the product library knows no kernel-selecting key
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256   # the plan entry answers for a 256-CU part
    reached = set()
    for m, n, k in PRODUCT_SHAPES:
        key = nc.Case("nv", 0, (), m, n, k)
        assert key in nc.KEYS
        d, ref = nc.dataset(key, "plain"), nc.reference(key, "plain")
        for with_ws in (False, True):
            r = plan(m, n, k, int(with_ws))
            cfg, splits = (r % 256, r // 256) if r >= 256 else (r, 1)
            v, s = nc.plan_variant(cfg, splits, k)
            named = key._replace(variant=v + s if s > 1 else v)
            assert named.splits == s
            got = nc.run(key, d, lib=product, workspace=with_ws)
            nc.assert_footprint(got)
            assert (got.ws_bytes > 0) == (s > 1)
            want = nc.run(named, d)
            assert np.array_equal(got.out, want.out), f"{m}x{n}x{k}, workspace {with_ws}: the product's bits are not those of form {named.variant}"
            nc.assert_equals_reference(got.out, ref)
            reached.add(v)
    assert len(reached) >= 4, reached
