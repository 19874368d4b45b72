"""CPU half of tests/test_gpu_mx_scale_range.py and tests/test_gpu_gemm_footprint.py (no GPU): the test data itself, checked with the oracle alone, and the list of
covered kernel forms against what the product's plan entries can return.

  * the whole-range scale layouts are in the EXACT regime: K groups summed forward and reversed in fp32 give the same bits, which are the oracle's;
  * both operands of every such case carry the scale bytes 0, 1, 127, 253 and 254;
  * the oracle's isnan(D) of the tracer data is the predicted row / column pattern, and the fp8 special codes give NaN / +-inf rows and columns where they were placed;
  * every (variant, split or not) that qutlass_amd_debug_gemm_plan / _ada_plan / the grouped plan entries return over a shape sweep is one the GPU files run.
"""
import ctypes

import numpy as np
import pytest

import _mx_cases as mc

DENSE = [c for c in mc.CASES if c.op in ("mxf4", "mxf8")]
W4A8 = sorted({c._replace(variant=0, opts=()) for c in mc.CASES if c.op == "g48"}, key=lambda c: c.id)      # (their reference is numpy's fp64 matmul: no size cut)
KEYS = sorted({c._replace(variant=0, opts=()) for c in DENSE}, key=lambda c: c.id) + W4A8
SMALL_KEYS = [c for c in KEYS if c.m * c.n * c.k <= 83 * 200 * 4352]          # (CPU time: the large tiles' shapes run on the GPU side against the same builder)


@pytest.mark.parametrize("layout", ["sweep", "extremes"])
@pytest.mark.parametrize("c", KEYS, ids=lambda c: c.id)
def test_whole_range_layouts_are_in_the_exact_regime(c, layout):
    d = mc.dataset(c, layout)
    for s, rows in ((d.sa, c.m), (d.sb, c.n * (mc.GROUPED_E if c.grouped else 1))):
        seen = set(np.unique(s[:rows]).tolist())
        if layout == "extremes":
            assert {0, 1, 127, 253, 254} <= seen
        else:   # (the shortest K here has 21 groups: they still spread over most of the range, far apart from one group to the next)
            assert max(seen) - min(seen) >= 200 and len(seen) >= 20
        assert int(s.max()) <= 254
    e = d.sa[:c.m].astype(int)[:, None, :] + d.sb[:c.n].astype(int)[None, :, :] - 254
    assert e.min() == -1 and e.max() == 1                      # every block's scale product is 2^-1 ... 2^1
    rows, cols, fwd = mc.sums_in_fp32(c, d, reverse=False)
    _, _, rev = mc.sums_in_fp32(c, d, reverse=True)
    assert np.array_equal(fwd.view(np.uint32), rev.view(np.uint32))
    assert np.array_equal(mc.f32_to_bf16_bits(fwd * np.float32(d.alpha)), d.ref[np.ix_(rows, cols)])
    assert not mc.isnan_bf16(d.ref).any() and len(np.unique(d.ref)) > 100


@pytest.mark.parametrize("c", [k for k in {c._replace(variant=0, opts=()) for c in mc.CASES} if k.m * k.n * k.k <= 83 * 200 * 4352 or k in W4A8], ids=lambda c: c.id)
def test_oracle_nan_pattern_of_the_tracer_data_is_the_predicted_one(c):
    d = mc.dataset(c, "nan")
    want = mc.nan_pattern(c)
    assert np.array_equal(mc.isnan_bf16(d.ref), want)
    assert 0.4 < want.mean() < 0.6 and (d.sa[c.m:] == 255).any() == (mc.pad128(c.m) > c.m and not c.grouped)


@pytest.mark.parametrize("c", [k for k in {c._replace(variant=0, opts=()) for c in mc.FP8_CASES} if k.m * k.n * k.k <= 300 * 200 * 1184], ids=lambda c: c.id)
def test_oracle_on_fp8_special_codes(c):
    d = mc.dataset(c, "special")
    nan, bits = mc.isnan_bf16(d.ref), d.ref
    special_rows = [2, 17, 40, 64, c.m - 2, c.m - 1]
    bounds = np.r_[0, np.cumsum(mc.group_counts(c))] if c.op == "g8" else np.array([0, c.m])
    assert nan[2].all() and nan[c.m - 1].all() and nan[c.m - 3, c.n - 1]
    for s, e in zip(bounds[:-1], bounds[1:]):                                         # per expert (dense: one segment): its own B columns
        plain = [r for r in range(s, e) if r not in special_rows]
        if not plain:
            continue
        quiet = ~nan[plain[0]]                                                        # columns no NaN code of this expert's B touches
        assert quiet.sum() >= c.n - 2 and np.array_equal(nan[plain], np.broadcast_to(~quiet, (len(plain), c.n)))
        if c.a5 and s <= 17 and e > 64:
            col = np.arange(c.n)
            assert nan[64].all()                                                      # +inf and -inf in one row
            assert np.array_equal(nan[17] & quiet, (col % 11 == 4) & quiet)           # inf x 0
            assert (bits[17][quiet & (col % 11 != 4)] == 0x7F80).all()                # +inf
            assert np.array_equal(bits[40][quiet], np.where(col % 2 == 0, 0xFF80, 0x7F80)[quiet])   # -inf x +-1.0
    if c.a5:
        assert nan[c.m - 2].all()                                                     # the other two e5m2 NaN codes
    if c.op != "g8":
        assert nan[:, 3].all() and nan[:, c.n - 1].all()


# ------------------------------------------------------------------------------------------------
# covered forms == what the plans can return
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()
    return _lib.load()


MS = (1, 8, 16, 17, 24, 32, 33, 48, 64, 65, 96, 128, 160, 200, 256, 384, 512, 768, 1024, 2048, 2560, 4096, 5120, 8192)
NS = (8, 64, 512, 1024, 2048, 4096, 5120, 6144, 8192, 11008, 12288, 14336, 16384, 28672, 57344)
KS = (256, 768, 1024, 2048, 3072, 4096, 5120, 8192, 11008, 14336, 16384, 28672)


def test_every_form_the_dense_plans_return_is_run_on_the_gpu(lib):
    f = lib.qutlass_amd_debug_gemm_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    out = (ctypes.c_int * 24)()
    for ebits, op in ((4, "mxf4"), (8, "mxf8")):
        single, split = set(), set()
        for m in MS:
            for n in NS:
                for k in KS:
                    for ws in (0, 1 << 40):
                        cnt = f(ebits, m, n, k, ws, out, 8)
                        assert cnt >= 1
                        for i in range(cnt):
                            (split if out[3 * i + 2] > 1 else single).add(out[3 * i])
        assert len(single) >= 15 and split, (single, split)
        assert single <= mc.covered(op), f"{op}: forms {sorted(single - mc.covered(op))} are planned but not run by tests/test_gpu_mx_scale_range.py"
        assert split <= mc.covered(op, split=True), f"{op}: split-K forms {sorted(split - mc.covered(op, split=True))} are planned but not run"
        assert 89 not in single | split          # stream-K stays a lab form (left out of the GPU cases)
    # the NN op: its own persistent kernel (63) or the pre-pass (62) + the TN plan above
    assert {62, 63} <= mc.covered("nn")


def test_every_form_the_ada_and_grouped_plans_return_is_run_on_the_gpu(lib):
    f = lib.qutlass_amd_debug_ada_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    out = (ctypes.c_int * 24)()
    seen = set()
    for m in MS:
        for n in NS:
            for k in KS:
                if k % 128 == 0:
                    cnt = f(m, n, k, out, 8)
                    assert cnt >= 1
                    seen |= {out[3 * i] for i in range(cnt)}
    assert len(seen) >= 6 and seen <= mc.covered("ada"), sorted(seen - mc.covered("ada"))
    o3 = (ctypes.c_int64 * 8)()
    for name, op in (("qutlass_amd_debug_grouped_plan", "g4"), ("qutlass_amd_debug_grouped_mxf8_plan", "g8"), ("qutlass_amd_debug_grouped_mxf8_mxf4_plan", "g48")):
        g = getattr(lib, name)
        g.restype = ctypes.c_int
        g.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
        seen = set()
        for m in (8, 128, 512, 4096, 16384):
            for k in (768, 1024, 4096, 8192, 14336):
                for e in (1, 8, 128):
                    v = g(m, 2048, k, e, o3)
                    assert v >= 0
                    seen.add(v)
        assert len(seen) == 2 and seen <= mc.covered(op), (op, seen)
