"""CPU half of tests/test_gpu_nv_scale_range.py (no GPU): the test data of tests/_nv_cases.py itself, checked with the oracle alone, and the list of covered kernel
forms against what the product's plan entries can return.

  * the whole-range scale layouts are in the EXACT regime: every term a multiple of one quantum, sum |terms| < 2^24 quanta for every output, K groups summed forward
    and reversed in fp32 give the same bits, which are the oracle's;
  * both operands of every case carry every byte of the extremes list, and most of the 254 finite e4m3 bytes of both signs over the two orientations of the sweep;
  * the oracle's isnan(D) of the tracer data is the predicted row / column pattern;
  * every form and every number of K ranges that qutlass_amd_debug_nvf4_plan returns over a shape sweep is one the GPU file runs, likewise the grouped NVFP4 and the
    W4A8 plans (the latter against tests/_mx_cases.py).
"""
import ctypes

import numpy as np
import pytest

import _mx_cases as mc
import _nv_cases as nc
from test_mx_scale_range_cpu import KS, MS, NS

SMALL_KEYS = [c for c in nc.KEYS if c.m * c.n * c.k <= 83 * 200 * 4352]          # (CPU time of the oracle: the large tiles' shapes run on the GPU side against the same builder)
IDS = lambda c: c.id   # noqa: E731


def _ulp_exponent(byte):
    """exponent of the lowest set bit of an e4m3 byte's value: the value is an odd multiple of 2^that; a zero byte is a multiple of everything"""
    e, m = (byte.astype(np.int64) >> 3) & 15, byte.astype(np.int64) & 7
    sig = np.where(e == 0, m, 8 + m)                                        # value = sig 2^(max(e, 1) - 10)
    ctz = np.log2(np.where(sig == 0, 1, sig & -sig)).astype(np.int64)
    return np.where(sig == 0, 99, np.maximum(e, 1) - 10 + ctz)


@pytest.mark.parametrize("walk_a", [True, False], ids=["a-walks", "b-walks"])
@pytest.mark.parametrize("layout", ["sweep", "extremes"])
@pytest.mark.parametrize("c", nc.KEYS, ids=IDS)
def test_whole_range_layouts_keep_every_sum_below_2_to_24_quanta(c, layout, walk_a):
    """every key, the large shapes included (no oracle call): terms are multiples of QUANTUM and sum |terms| < 2^24 QUANTUM, so fp32 sums in any order are exact"""
    d = nc.dataset(c, layout, walk_a)
    assert not (d.sa & 0x7F == 0x7F).any() and not (d.sb & 0x7F == 0x7F).any()
    ad, bd = nc.dequantised(c, d)
    for e, r0, r1 in nc.segments(c):
        sbe = d.sb[e * c.n:(e + 1) * c.n]
        # an e2m1 value is a multiple of 2^-1: a term is a multiple of 2^(ulp(sA) + ulp(sB) - 2)
        assert (_ulp_exponent(d.sa[r0:r1]).min(axis=0) + _ulp_exponent(sbe).min(axis=0)).min() - 2 >= np.log2(nc.QUANTUM)
        be = bd[e * c.n:(e + 1) * c.n]
        assert np.isfinite(ad).all() and np.isfinite(be).all()
        total = np.abs(ad[r0:r1]) @ np.abs(be).T
        assert total.max() < 2.0 ** 24 * nc.QUANTUM, (total.max() / nc.QUANTUM, 2.0 ** 24)
        assert np.abs(ad).max() <= 2688 and np.abs(ad[ad != 0]).min() >= 2.0 ** -10      # exact in f16, where the kernels form e2m1 x e4m3


@pytest.mark.parametrize("walk_a", [True, False], ids=["a-walks", "b-walks"])
@pytest.mark.parametrize("layout", ["sweep", "extremes"])
@pytest.mark.parametrize("c", SMALL_KEYS, ids=IDS)
def test_whole_range_layouts_are_in_the_exact_regime(c, layout, walk_a):
    d, ref = nc.dataset(c, layout, walk_a), nc.reference(c, layout, walk_a)
    rows, cols, fwd = nc.sums_in_fp32(c, d, reverse=False)
    _, _, rev = nc.sums_in_fp32(c, d, reverse=True)
    assert np.array_equal(fwd.view(np.uint32), rev.view(np.uint32))
    assert np.array_equal(mc.f32_to_bf16_bits(fwd * np.float32(d.alpha)), ref[np.ix_(rows, cols)])
    assert not mc.isnan_bf16(ref).any() and len(np.unique(ref)) > 100


@pytest.mark.parametrize("c", nc.KEYS, ids=IDS)
def test_both_operands_carry_the_extremes_and_most_of_the_finite_range(c):
    kb = c.k // 16
    for layout in ("sweep", "extremes"):
        walker_a, walker_b = nc.dataset(c, layout, True).sa[:c.m], nc.dataset(c, layout, False).sb[:c.n]     # each operand in the orientation where its byte walks
        for s in (walker_a, walker_b):
            seen = set(np.unique(s).tolist())
            assert 0x7F not in seen and 0xFF not in seen
            if layout == "extremes":
                assert set(nc.EXTREMES) <= seen
            else:
                assert len(seen) >= min(kb, 200) and min(len([b for b in seen if b < 0x80]), len([b for b in seen if b >= 0x80])) >= min(kb, 200) // 3
        # the compensating side holds powers of two only
        comp = nc.dataset(c, layout, True).sb
        assert set(np.unique(comp).tolist()) <= set(nc.pow2_byte(np.arange(-9, 9)).tolist())


@pytest.mark.parametrize("c", SMALL_KEYS, ids=IDS)
def test_oracle_nan_pattern_of_the_tracer_data_is_the_predicted_one(c):
    d = nc.dataset(c, "nan")
    want = mc.nan_pattern(c)
    assert np.array_equal(mc.isnan_bf16(nc.reference(c, "nan")), want)
    assert 0.4 < want.mean() < 0.6
    na, nb = nc.nan_byte_pattern(c, d)
    assert {0x7F, 0xFF} <= set(d.sa[na].tolist()) and {0x7F, 0xFF} <= set(d.sb[nb].tolist())
    assert na[c.m:].any() == (mc.pad128(c.m) > c.m and c.op != "gnv")            # ... a NaN in the padding rows of the blocked image
    assert na[:, c.k // 16 - 1].any()                                            # ... and in the last scale column of a row
    # NaN x code 0 = NaN in the oracle: a poisoned group poisons its row whatever the codes are
    plain = nc.reference(c, "plain")
    assert not mc.isnan_bf16(plain).any()


# ------------------------------------------------------------------------------------------------
# covered forms == what the plans can return
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()
    return _lib.load()


# small batches against wide weights: the decode forms with 32 / 48 / 56 columns per workgroup (cfg -6 ... -9) and -7's N >= 20480 arm
WIDE = [(m, n, k) for m in (1, 4, 8, 9, 16) for n in (6144, 8192, 11008, 12288, 14336, 16384, 20480, 24576, 28672, 36864) for k in (2048, 4096, 5120, 8192)]


def plan_forms(lib, shapes):
    """{(form as in _nv_cases.covered, K ranges)} of nvf4_plan over the shapes, with and without scratch, and the raw cfg values"""
    f = lib.qutlass_amd_debug_nvf4_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int]
    forms, cfgs = set(), set()
    for m, n, k in shapes:
        for may_split in (0, 1):
            r = f(m, n, k, may_split)
            assert r > -20
            cfg, splits = (r % 256, r // 256) if r >= 256 else (r, 1)
            assert may_split or splits == 1
            cfgs.add(cfg)
            forms.add(nc.plan_variant(cfg, splits, k))
    return forms, cfgs


def _check_dense_coverage(lib):
    forms, cfgs = plan_forms(lib, [(m, n, k) for m in MS for n in NS for k in KS + (2432, 4128, 5632, 6144)] + WIDE)
    variants, splits = {v for v, _ in forms}, {s for _, s in forms if s > 1}
    assert -3 not in cfgs and 47 not in variants                 # the 16-column form stays lab-only
    missing = variants - nc.covered("nv")
    assert not missing, f"forms {sorted(missing)} are planned but not run by tests/test_gpu_nv_scale_range.py"
    assert splits <= nc.covered_splits(), f"split counts {sorted(splits - nc.covered_splits())} are planned but not run"
    return variants, splits


def test_every_form_the_dense_plan_returns_is_run_on_the_gpu(lib):
    variants, splits = _check_dense_coverage(lib)
    # the sweep must not go blind: it reaches every form of the table on a 256-CU part, and every reduce instantiation
    assert variants == nc.covered("nv"), f"never planned over the sweep: {sorted(nc.covered('nv') - variants)}"
    assert splits == {2, 3, 4, 5, 6, 7, 8}


def test_a_form_missing_from_the_table_fails_the_coverage_check(lib, monkeypatch):
    every = list(nc.CASES)
    monkeypatch.setattr(nc, "CASES", [c for c in every if c.variant != 52])
    with pytest.raises(AssertionError, match="forms \\[52\\] are planned but not run"):
        _check_dense_coverage(lib)
    monkeypatch.setattr(nc, "CASES", [c for c in every if c.splits != 3])
    with pytest.raises(AssertionError, match="split counts \\[3\\] are planned but not run"):
        _check_dense_coverage(lib)


def test_every_form_the_grouped_nvfp4_and_w4a8_plans_return_is_run_on_the_gpu(lib):
    o3 = (ctypes.c_int64 * 8)()
    for name, want, have in (("qutlass_amd_debug_grouped_nvf4_plan", {598, 600, 601}, nc.covered("gnv")),
                             ("qutlass_amd_debug_grouped_mxf8_mxf4_plan", None, mc.covered("g48"))):
        g = getattr(lib, name)
        g.restype = ctypes.c_int
        g.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
        seen = set()
        for m in (8, 128, 512, 4096, 16384):
            for n in (512, 2048, 4096):
                for k in (768, 1024, 4096, 8192, 14336):
                    for e in (1, 8, 128):
                        v = g(m, n, k, e, o3)
                        assert v >= 0
                        seen.add(v)
        assert seen <= have, (name, sorted(seen - have))
        assert seen == want if want else len(seen) >= 2, (name, seen)
    assert nc.covered("gnv") == {598, 599, 600, 601}             # (599 is run although no plan returns it)
    assert mc.covered("g48") == {602, 603, 604}
