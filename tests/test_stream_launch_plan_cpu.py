"""The launch plan of the four QAT-backward data-prep ops (quartet_bwd.hip.h: STREAM_FORMS, stream_launch_plan) through qutlass_amd_debug_stream_launch_plan, no GPU:
the one function the C entries and both debug entries read.  The entry writes {form, workgroups, threads per workgroup} for a part of `cus` CUs; ops 0 ... 3 =
backward_t_bf16 (B, N, M), backward_qt_bf16 (B, N, M), backward_bf16_square_double_mxfp8_rows (m_pad, n, m), mxfp4_transpose_mxfp8_rows (m_pad, n, m).  The formulas
below are the grid computations of the C entries as they stood before the plan existed, written out again here -- not read from the code under test."""
import ctypes
import os
import re

import numpy as np
import pytest

T, QT, SQ, TR = 0, 1, 2, 3
CUS = (1, 2, 8, 64, 256, 304)


def _bind(L):
    L.qutlass_amd_debug_stream_launch_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_stream_launch_plan.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    L.qutlass_amd_debug_stream_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_stream_plan.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 3
    return L


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()
    return _bind(_lib.load())


@pytest.fixture(scope="module")
def lab():
    from qutlass_amd import build

    assert os.path.exists(build.BENCH_OUT), build.BENCH_OUT
    return _bind(ctypes.CDLL(build.BENCH_OUT))


def plan(L, op, a, b, c, cus, variant=0, ring=1):
    out = (ctypes.c_int * 3)(-7, -7, -7)
    rc = L.qutlass_amd_debug_stream_launch_plan(op, a, b, c, cus, variant, ring, out)
    assert rc in (1, -1)
    return tuple(out) if rc == 1 else None


def cdiv(a, b):
    return -(-a // b)


def want_bwd(op, B, N, M, C, ring):
    G, tm = N // 32, cdiv(M, 64)
    u = B * tm * cdiv(G, 8)
    if op == T:
        return (3, min(cdiv(u, 4), 2 * C), 256) if u >= 6 * C else (1, min(u, 2 * C), 512)
    if ring and M % 128 == 0 and u >= 12 * C:
        return 5, min(B * cdiv(M, 256) * cdiv(G, 4), max(8, 3 * C // 8 * 8)), 256
    if u >= 3 * C:
        return 2, min(cdiv(B * tm * cdiv(G, 4), 4), 4 * C), 256
    v = B * cdiv(tm, 4) * 4 * cdiv(G, 8)
    per = 3 if 1.24 * cdiv(v, 3 * C) < cdiv(v, 2 * C) else 2
    return 1, max(32, min(cdiv(v, 32) * 32, C * per // 32 * 32)), 512


def want_rows(op, m_pad, n, C):
    if op == TR:
        return 128, (m_pad // 128) * (n // 128), 256
    rb = m_pad // 128
    ct = 4 if n % 512 == 0 and rb * (n // 512) >= C else 1
    return ct, rb * n // (128 * ct), 256 * ct


def _dim(rng, unit, top):
    """a multiple of `unit` up to ~top: small and ragged, or large enough for the rules of a 256-CU part"""
    k = int(rng.integers(0, 3))
    hi = (8, 64, top // unit)[k]
    return int(rng.integers(1, hi + 1)) * unit


@pytest.mark.parametrize("op", [T, QT])
def test_backward_t_and_qt_launches_agree_with_the_entries_formulas(lib, op):
    rng = np.random.default_rng(31 + op)
    seen = set()
    for i in range(3000):
        B = int(rng.choice([1, 1, 1, 2, 3, 7]))
        N = _dim(rng, 32, 16384)
        M = _dim(rng, 128 if (op == QT and i % 2) else (32 if op == QT else 8), 16384)
        for C in CUS:
            for ring in ((1, 0) if op == QT else (1,)):
                got = plan(lib, op, B, N, M, C, 0, ring)
                assert got == want_bwd(op, B, N, M, C, ring) and got[1] >= 1, (op, B, N, M, C, ring, got, want_bwd(op, B, N, M, C, ring))
                if C == 256 and ring:
                    seen.add(got[0])
                    assert got[0] == lib.qutlass_amd_debug_stream_plan(op, B, N, M), (op, B, N, M)
                if not ring:
                    assert got[0] != 5
    assert seen == ({1, 3} if op == T else {1, 2, 5}), seen


@pytest.mark.parametrize("op", [SQ, TR])
def test_rows_ops_launches_agree_with_the_entries_formulas(lib, op):
    rng = np.random.default_rng(41 + op)
    seen = set()
    for _ in range(3000):
        m_pad = _dim(rng, 128, 16384)
        n = _dim(rng, 128 if op == SQ else 256, 16384)
        m = int(rng.integers(1, m_pad + 1))
        for C in CUS:
            got = plan(lib, op, m_pad, n, m, C)
            assert got == want_rows(op, m_pad, n, C) and got[1] >= 1, (op, m_pad, n, m, C, got, want_rows(op, m_pad, n, C))
            if C == 256:
                seen.add(got[0])
                if op == SQ:
                    assert got[0] == lib.qutlass_amd_debug_stream_plan(op, m_pad, n, 0), (m_pad, n)
    assert seen == ({1, 4} if op == SQ else {128}), seen


def test_a_small_part_never_gets_an_empty_grid(lib):
    """the persistent grids are cut down to multiples of 8 (ring) / 32 (QT on the round-3 kernel) workgroups: never to none, on 1 ... 10 CUs"""
    for C in range(1, 11):
        for B, N, M in [(1, 32, 128), (1, 8192, 8192), (2, 4096 + 32, 2048 + 128), (1, 256, 32)]:
            for op in (T, QT):
                got = plan(lib, op, B, N, M, C)
                assert got == want_bwd(op, B, N, M, C, 1) and got[1] >= 1, (op, B, N, M, C, got)
    assert plan(lib, QT, 1, 8192, 8192, 1) == (5, 8, 256) and plan(lib, QT, 1, 32, 32, 1) == (1, 32, 512)


def test_launch_plan_rejects_what_the_entries_reject(lib):
    ok = {T: (1, 64, 8), QT: (1, 64, 32), SQ: (128, 128, 1), TR: (128, 256, 128)}
    for op, args in ok.items():
        assert plan(lib, op, *args, 256) is not None
        for v in (1, 2, 3, 4, 5, 9, 128, -1):   # the product library knows the product rules only
            assert plan(lib, op, *args, 256, v) is None, (op, v)
    big = 1 << 40
    for op, mult in ((T, 8), (QT, 32)):
        for B, N, M in [(0, 64, 64), (1, 0, 64), (1, 64, 0), (-1, 64, 64), (1, 48, 64), (1, 64, mult // 2), (1, 64, mult + 4),
                        (1, 32, 1 << 24), (1, 1 << 26, 32), (1 << 16, 1 << 12, 1 << 12), (big, 32, 32)]:
            assert plan(lib, op, B, N, M, 256) is None, (op, B, N, M)
    assert plan(lib, T, 1, 64, 40, 256) is not None and plan(lib, QT, 1, 64, 40, 256) is None   # M % 8 against M % 32
    assert plan(lib, T, 1 << 11, 1 << 25, 8, 256) is None    # 2^39 elements, but 2^31 tiles of 32 x 64: the second bound alone
    assert plan(lib, T, 1 << 9, 1 << 20, 1 << 9, 256) is not None   # 2^38 elements, 2^27 tiles of 32 x 64: just inside both bounds
    for op, nm in ((SQ, 128), (TR, 256)):
        for m_pad, n, m in [(128, nm, 0), (128, nm, -3), (128, 0, 1), (128, nm // 2, 1), (128, nm + 64, 1), (64, nm, 1), (192, nm, 1), (128, nm, 129), (0, nm, 1),
                            (1 << 31, nm, 1), (128, 1 << 31, 1), (1 << 24, 1 << 24, 1)]:
            assert plan(lib, op, m_pad, n, m, 256) is None, (op, m_pad, n, m)
        assert plan(lib, op, 256, 2 * nm, 129, 256) is not None
    assert plan(lib, SQ, 128, 384, 1, 256) is not None and plan(lib, TR, 128, 384, 1, 256) is None   # n % 128 against n % 256
    out = (ctypes.c_int * 3)()
    f = lib.qutlass_amd_debug_stream_launch_plan
    assert f(4, 128, 256, 128, 256, 0, 1, out) == -1 and f(-1, 1, 64, 64, 256, 0, 1, out) == -1 and f(T, 1, 64, 64, 0, 0, 1, out) == -1
    assert f(T, 1, 64, 64, 256, 0, 1, None) == -1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    assert not re.search(r"\bqutlass_amd_debug_stream_launch_plan\b", hdr), "debug entries stay out of the public header"


# STREAM_FORMS as the lab options see it: (op, forcing value = form, threads) and a shape the form takes.  bwd_variant 1 ... 9 for T / QT (T has no form 4 ... 8),
# transpose_nc 1 / 4 / 8 for square-double and 128 / 256 / 3 / 4 / 2 / 5 ... 8 for the transposer.
LAB_ROWS = [(T, 1, 512), (T, 2, 256), (T, 3, 256), (T, 9, 256),
            (QT, 1, 512), (QT, 2, 256), (QT, 3, 256), (QT, 4, 512), (QT, 5, 256), (QT, 6, 256), (QT, 7, 256), (QT, 8, 256), (QT, 9, 256),
            (SQ, 1, 256), (SQ, 4, 1024), (SQ, 8, 1024),
            (TR, 128, 256), (TR, 256, 256), (TR, 3, 512), (TR, 4, 256), (TR, 2, 256), (TR, 5, 256), (TR, 6, 256), (TR, 7, 256), (TR, 8, 256)]


def test_lab_library_reaches_every_row_of_the_form_list_by_its_forcing_value(lab):
    for op, v, threads in LAB_ROWS:
        for args in ([(1, 64, 128), (2, 4096 + 32, 2048 + 128)] if op <= QT else [(256, 1024, 200), (4096, 5120, 4000)]):
            got = plan(lab, op, *args, 256, v)
            assert got is not None and got[0] == v and got[2] == threads and got[1] >= 1, (op, v, args, got)
    # unforced, the lab library plans as the product does
    for op, args in [(T, (1, 8192, 8192)), (QT, (1, 8192, 8192)), (QT, (1, 4096, 4096)), (SQ, (8192, 8192, 8192)), (TR, (256, 512, 256))]:
        want = want_bwd(op, *args, 256, 1) if op <= QT else want_rows(op, args[0], args[1], 256)
        assert plan(lab, op, *args, 256) == want
    # a value that names no form of the op leaves the call to the product rules; a forced whole-line QT form refuses M % 128 != 0; a forced form of the _rows ops whose
    # unit does not divide the tensor leaves the call to the product rules
    assert plan(lab, T, 1, 8192, 8192, 256, 5) == want_bwd(T, 1, 8192, 8192, 256, 1) and plan(lab, SQ, 256, 1024, 256, 256, 128) == want_rows(SQ, 256, 1024, 256)
    for v in (4, 5, 6, 7, 8):
        assert plan(lab, QT, 1, 64, 160, 256, v) is None and plan(lab, QT, 1, 64, 160, 256, 2) is not None
    assert plan(lab, TR, 384, 512, 384, 256, 3) == want_rows(TR, 384, 512, 256) and plan(lab, SQ, 256, 1536, 256, 256, 8) == want_rows(SQ, 256, 1536, 256)
