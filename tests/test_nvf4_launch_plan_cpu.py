"""matmul_nvf4_bf16_tn's launch plan (gemm_nvf4.hip.h: nvf4_launch_plan) through qutlass_amd_debug_nvf4_launch_plan, no GPU: the one function the launcher, the workspace
query and the debug entries read.  Per launch the entry writes {form, columns, rows, K ranges, stages per range, workgroups}; the forms are NvForm's values, which are
what qutlass_amd_debug_nvf4_plan reports (tests/test_cabi_and_host.py asserts them on named shapes)."""
import ctypes

import numpy as np
import pytest

# tile rows x columns of a workgroup per form (NV_FORMS): -11 / -10 96x32 / 64x32, -9 ... -6 the decode form with 56 / 56 / 48 / 32 columns, -5 / -4 32x16 / 16x16,
# -3 / -2 wave-owned 16 / 32 columns, -1 skinny, 0 256x256, 1 128x128, 2 128x64, 3 64x64, 4 256x128
TILE = {-11: (96, 32), -10: (64, 32), -9: (16, 56), -8: (16, 56), -7: (16, 48), -6: (16, 32), -5: (32, 16), -4: (16, 16), -3: (32, 16), -2: (32, 32), -1: (32, 32),
        0: (256, 256), 1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (256, 128)}
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()
    L = _lib.load()
    L.qutlass_amd_debug_nvf4_plan.restype, L.qutlass_amd_debug_nvf4_plan.argtypes = ctypes.c_int, [ctypes.c_int64] * 3 + [ctypes.c_int]
    L.qutlass_amd_debug_nvf4_pk_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_nvf4_pk_plan.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.qutlass_amd_debug_nvf4_launch_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_nvf4_launch_plan.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return L


def launches(lib, m, n, k, ws, cap=8):
    out = (ctypes.c_int * (6 * cap))()
    cnt = lib.qutlass_amd_debug_nvf4_launch_plan(m, n, k, ws, out, cap)
    return cnt, [tuple(out[6 * i:6 * i + 6]) for i in range(max(0, min(cnt, cap)))]


def cdiv(a, b):
    return -(-a // b)


def test_launch_plan_agrees_with_the_rule_and_the_workspace_query(lib):
    rule, query, pk = lib.qutlass_amd_debug_nvf4_plan, lib.qutlass_amd_nvf4_splitk_workspace_bytes, lib.qutlass_amd_debug_nvf4_pk_plan
    rng = np.random.default_rng(23)
    out3 = (ctypes.c_int * 3)()
    split = forms = 0
    seen = set()
    for _ in range(4000):
        m = int(rng.choice([1, 7, 8, 16, 17, 33, 64, 96, 128, 160, 200, 256, 384, 512, 768, 1000, 2048, 4096]))
        n = int(rng.integers(1, 2048)) * 8
        k = int(rng.integers(1, 1024)) * 32
        kt = cdiv(k // 2, 128)
        r0, r1 = rule(m, n, k, 0), rule(m, n, k, 1)
        q = query(m, n, k)
        want = r1 if r1 >= 256 else r0   # (a shape that does not split runs the plan without scratch)
        cnt, ls = launches(lib, m, n, k, BIG)
        assert cnt == 1, (m, n, k, cnt)
        form, cols, rows, splits, kt_per, grid = ls[0]
        assert (cols, rows) == (n, m)
        assert form == (want % 256 if want >= 256 else want) and splits == max(1, want // 256 if want >= 256 else 1), (m, n, k, ls[0], r0, r1)
        assert (splits * m * n * 4 if splits > 1 else 0) == q, (m, n, k, ls[0], q)
        seen.add(form)
        # missing or undersized scratch: the single pass
        for ws in (0, max(q - 1, 0), -5):
            c1, l1 = launches(lib, m, n, k, ws)
            assert c1 == 1 and l1[0][0] == r0 and l1[0][3:5] == (1, 0), (m, n, k, ws, l1, r0)
            if q == 0:
                assert l1[0] == ls[0]
        assert launches(lib, m, n, k, q)[1] == ls   # exactly the queried bytes suffice
        if splits > 1:
            split += 1
            assert form in (1, 2, 3) and kt_per % 2 == 0 and kt_per >= 4 and kt_per * (splits - 1) < kt <= kt_per * splits, (m, n, k, ls[0])
            assert 2 * cdiv(kt, 2 * splits) == kt_per, (m, n, k, ls[0])   # the launcher's former recomputation: a fixed point of the plan's values
        else:
            assert kt_per == 0
        tm, tn = TILE[form]
        if form == 0 and pk(m, n, k, 0, out3):
            assert grid == out3[0] and splits == 1, (m, n, k, ls[0], out3[0])
        else:
            assert grid == cdiv(m, tm) * cdiv(n, tn) * splits, (m, n, k, ls[0])
    assert split > 100 and seen >= {-11, -10, -5, -4, -2, -1, 0, 1, 2, 3, 4}, (split, sorted(seen))


def test_split_range_is_a_fixed_point_for_every_stage_count():
    """nvf4_plan takes kt_per = 2 ceil(KT / 2 S) and S2 = ceil(KT / kt_per) ranges for S asked; computing the range again from S2, as the launcher once did, gives kt_per back"""
    for kt in range(1, 2049):
        for s in (1, 2, 4, 8):
            per = 2 * cdiv(kt, 2 * s)
            s2 = cdiv(kt, per)
            assert 2 * cdiv(kt, 2 * s2) == per and cdiv(kt, 2 * cdiv(kt, 2 * s2)) == s2, (kt, s, per, s2)


@pytest.mark.parametrize("m,n,k", [(8, 262400, 16384), (262400, 8, 16384), (128, 262400, 28672), (262400, 128, 28672)])
def test_operands_of_2_gib_run_as_ranges_without_scratch(lib, m, n, k):
    """an operand of >= 2 GiB: column ranges of B / row ranges of A of whole 256-tiles, each planned on its own and never split, whatever the workspace"""
    for ws in (0, 1 << 20, BIG):
        cnt, ls = launches(lib, m, n, k, ws)
        assert cnt == len(ls) > 1, (cnt, ls)
        if n > m:   # column ranges of B, A shared
            assert sum(l[1] for l in ls) == n and all(l[2] == m for l in ls) and all(l[1] % 256 == 0 for l in ls[:-1])
        else:       # row ranges of A, B shared
            assert sum(l[2] for l in ls) == m and all(l[1] == n for l in ls) and all(l[2] % 256 == 0 for l in ls[:-1])
        for form, cols, rows, splits, kt_per, grid in ls:
            assert splits == 1 and kt_per == 0 and grid >= 1 and form in TILE and form == lib.qutlass_amd_debug_nvf4_plan(rows, cols, k, 0)
    assert lib.qutlass_amd_nvf4_splitk_workspace_bytes(m, n, k) == 0


def test_launch_plan_rejects_what_the_op_rejects(lib):
    out = (ctypes.c_int * 6)()
    f = lib.qutlass_amd_debug_nvf4_launch_plan
    assert f(0, 128, 128, 0, out, 1) == -1 and f(128, 12, 128, 0, out, 1) == -1 and f(128, 128, 48, 0, out, 1) == -1 and f(128, 128, 0, 0, out, 1) == -1
    assert f(8, 1 << 20, 1 << 30, 0, out, 1) == -1   # K too large for a 256-column range
    assert f(128, 128, 32, 0, out, 1) == 1 and f(128, 128, 32, 0, out, 0) == 1
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    assert not re.search(r"\bqutlass_amd_debug_nvf4_launch_plan\b", hdr), "debug entries stay out of the public header"
