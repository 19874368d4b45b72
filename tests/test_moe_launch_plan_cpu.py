"""The launch plans of the ops around the grouped GEMMs through qutlass_amd_debug_moe_launch_plan, no GPU: row_stream_plan (quantize.hip.h: silu_and_mul,
swiglu_oai_and_mul, the two moe_combine forms), moe_topk_plan and moe_sort_plan (moe_route.hip.h: the two routers, the expert sort), fusedq_plan and activation_path_plan
(capi.hip: the one-launch activation path) -- the functions the C entries read.  op 0: (chunks) -> {workgroups, threads}; op 1: (elem_bytes, E, T | aligned << 62) ->
{R, vector loads, workgroups, threads}; op 2: (n, E, one-launch bound or 0) -> {launches, slots per workgroup, rows, workspace bytes}; op 3: (M) -> {rows per rotation
tile}; op 4: (M, N, K) -> {launches}.  The formulas below are the entries' computations as they stood before the plans existed, written out again here -- not read from
the code under test; the error texts of the combine entries are copied from that source too."""
import ctypes
import os
import re

import numpy as np
import pytest

ROW, TOPK, SORT, FUSEDQ, ACT = 0, 1, 2, 3, 4
CUS = (1, 2, 8, 64, 256, 304)
X = 0x10000   # a 16-byte aligned dummy address: nothing below dereferences it
INVALID = 1   # QAMD_ERR_INVALID (include/qutlass_amd.h)


def _bind(L):
    L.qutlass_amd_debug_moe_launch_plan.restype = ctypes.c_int
    L.qutlass_amd_debug_moe_launch_plan.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.qutlass_amd_moe_sort_workspace_bytes.restype = ctypes.c_int64
    L.qutlass_amd_moe_sort_workspace_bytes.argtypes = [ctypes.c_int64] * 2
    L.qutlass_amd_activation_path_launches.restype = ctypes.c_int
    L.qutlass_amd_activation_path_launches.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int]
    L.qutlass_amd_set_option.restype = ctypes.c_int
    L.qutlass_amd_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
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


def plan(L, op, a, b, c, cus, cap=4):
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = L.qutlass_amd_debug_moe_launch_plan(op, a, b, c, cus, out, cap)
    assert rc in (-1, 1, 2, 4)
    return tuple(out[:rc]) if rc > 0 else None


def cdiv(a, b):
    return -(-a // b)


# ---- row stream ------------------------------------------------------------------------------------------------------------------------------------------

def test_row_stream_launch_agrees_with_the_entries_formula(lib):
    rng = np.random.default_rng(5)
    for C in CUS:
        edge = [1, 255, 256, 257, 2048 * C - 1, 2048 * C, 2048 * C + 1, (1 << 31) - 1]
        rand = [int(v) for v in rng.integers(1, 1 << 31, 150)] + [int(v) for v in rng.integers(1, 4096 * C, 150)]
        for chunks in edge + rand:
            assert plan(lib, ROW, chunks, 0, 0, C) == (min(cdiv(chunks, 256), 8 * C), 256), (chunks, C)
    assert plan(lib, ROW, 0, 0, 0, 256) is None and plan(lib, ROW, -1, 0, 0, 256) is None   # the entries return before the launch (rows == 0) or refuse the shape


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------------------------

def topk(L, eb, e, t, aligned, cus):
    return plan(L, TOPK, eb, e, t | (int(aligned) << 62), cus)


def test_topk_launch_agrees_with_the_entries_formulas(lib):
    seen = set()
    for e in range(1, 1025):
        for eb in (2, 4):
            for aligned in (True, False):
                R = 4 if eb == 4 and cdiv(e, 64) <= 4 else 8 if cdiv(e, 64) <= 8 else 16
                vec = int(aligned and (e * eb) % 16 == 0)
                assert topk(lib, eb, e, 1000, aligned, 256) == (R, vec, 250, 256), (e, eb, aligned)
                assert R * 64 >= e
                seen.add((eb, R, vec))
    assert seen == {(eb, R, v) for eb in (2, 4) for R in (4, 8, 16) for v in (0, 1)} - {(2, 4, 0), (2, 4, 1)}   # R = 4: fp32 logits only
    for C in CUS:
        for t in (1, 3, 4, 5, 64 * C - 1, 64 * C, 64 * C + 1, (1 << 31) - 1):
            for eb, e in ((2, 128), (4, 7), (4, 1024)):
                got = topk(lib, eb, e, t, True, C)
                assert got[2:] == (min(cdiv(t, 4), 16 * C), 256), (t, C, got)
    assert topk(lib, 2, 128, 0, True, 256) == (8, 1, 0, 256)   # T == 0 passes the checks (the entry returns before the launch)


def test_topk_plan_rejects_what_the_entries_reject(lib):
    for e in (0, 1025, -1):
        assert topk(lib, 2, e, 16, True, 256) is None
    for eb in (0, 1, 3, 8, -2):
        assert topk(lib, eb, 64, 16, True, 256) is None
    for t in (-1, 1 << 31, 1 << 40):
        for aligned in (True, False):
            assert topk(lib, 4, 64, t, aligned, 256) is None, t


# ---- sort ------------------------------------------------------------------------------------------------------------------------------------------------

BOUND = 6144


def want_sort(n, E, bound=BOUND):
    if n <= bound:
        return 1, cdiv(n, 512) * 512, 1, 0
    spb = cdiv(max(4096, cdiv(n, 256)), 512) * 512
    return 3, spb, cdiv(n, spb), (min(256, cdiv(n, 4096)) + 1) * (E + 1) * 4


def _check_sort(L, n, E, arg=0, bound=BOUND):
    got = plan(L, SORT, n, E, arg, 256)
    assert got == want_sort(n, E, bound), (n, E, arg, got, want_sort(n, E, bound))
    launches, spb, rows, nbytes = got
    assert rows <= 256 and (nbytes == 0 or (rows + 1) * (E + 1) * 4 <= nbytes) and (launches == 1) == (nbytes == 0)
    assert spb % 512 == 0 and rows * spb >= n
    return nbytes


def test_sort_plan_agrees_with_the_entries_formulas_and_the_scratch_holds_the_geometry(lib):
    for E in (1, 8, 128, 1024):
        last = 0
        for n in range(0, 20001):
            nbytes = _check_sort(lib, n, E)
            assert nbytes >= last and nbytes == lib.qutlass_amd_moe_sort_workspace_bytes(n, E), (n, E)
            last = nbytes
    for E in (1, 8, 128, 1024):
        last = 0
        for n in (BOUND, BOUND + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 256 * 4096, 256 * 4096 + 1, (1 << 31) - 1):
            nbytes = _check_sort(lib, n, E)
            assert nbytes >= last and nbytes == lib.qutlass_amd_moe_sort_workspace_bytes(n, E), (n, E)
            last = nbytes
    for n, E, arg in [(-1, 8, 0), (1 << 31, 8, 0), (100, 0, 0), (100, 1025, 0), (100, 8, -1)]:
        assert plan(lib, SORT, n, E, arg, 256) is None, (n, E, arg)


def test_a_forced_one_launch_bound_moves_the_plan_and_the_workspace_alike(lib, lab):
    ns = [0, 1, 2, 511, 513, 4096, 4097, BOUND, BOUND + 1, 8191, 8192, 8193, 20000, 1 << 20, (1 << 31) - 1]
    for forced in (1, 8192):
        for L in (lib, lab):   # as the argument: the plan reads no global, so the product library takes it too
            for n in ns:
                for E in (1, 128, 1024):
                    _check_sort(L, n, E, forced, forced)
        try:               # as the lab option: the entry that sizes the caller's scratch passes it to the same plan
            lab.qutlass_amd_set_option(b"moe_sort_one_launch_max", forced)
            for n in ns:
                for E in (1, 128, 1024):
                    assert lab.qutlass_amd_moe_sort_workspace_bytes(n, E) == want_sort(n, E, forced)[3], (forced, n, E)
        finally:
            lab.qutlass_amd_set_option(b"moe_sort_one_launch_max", 0)
    for n in ns:
        assert lab.qutlass_amd_moe_sort_workspace_bytes(n, 128) == want_sort(n, 128)[3] == lib.qutlass_amd_moe_sort_workspace_bytes(n, 128)
        assert plan(lab, SORT, n, 128, 0, 256) == want_sort(n, 128)


# ---- the one-launch activation path --------------------------------------------------------------------------------------------------------------------

def test_fusedq_rows_per_rotation_tile(lib):
    for M in range(1, 33):
        assert plan(lib, FUSEDQ, M, 0, 0, 256) == (4 if M <= 4 else 8 if M <= 8 else 16 if M <= 16 else 32,), M
    for M in (0, 33, -1, 1 << 31):
        assert plan(lib, FUSEDQ, M, 0, 0, 256) is None, M


def want_act(M, N, K, C):
    if M <= 0 or N <= 0 or K <= 0 or M > 16 or N >= 32 * C or K % 128:
        return 2
    return 1 if K <= (4096 if M <= 4 else 2048 if M <= 8 else 0) else 2


def test_activation_path_plan_agrees_with_the_written_out_rule(lib):
    seen = set()
    for C in CUS:
        for M in range(1, 18):
            for N in (8, 4096, 32 * C - 8, 32 * C):
                for K in (128, 2048, 2176, 4096, 4224, 8192, 100):
                    got = plan(lib, ACT, M, N, K, C)
                    assert got == (want_act(M, N, K, C),), (M, N, K, C, got)
                    seen.add(got[0])
    assert seen == {1, 2}
    for M, N, K in [(0, 64, 128), (4, 0, 128), (4, 64, 0), (-1, 64, 128)]:
        assert plan(lib, ACT, M, N, K, 256) == (2,)


def test_the_public_activation_path_entry_runs_the_same_plan(lib):
    import torch

    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    else:
        # no device to read a CU count from: the entry then plans for 256 CUs (chip_cus), which is all that can be compared here
        cus = 256
    for M in (1, 4, 5, 8, 9, 16, 17):
        for N in (8, 4096, 32 * cus - 8, 32 * cus):
            for K in (128, 2048, 2176, 4096, 4224, 100):
                assert (lib.qutlass_amd_activation_path_launches(M, N, K, 32),) == plan(lib, ACT, M, N, K, cus), (M, N, K, cus)
        assert lib.qutlass_amd_activation_path_launches(M, 4096, 2048, 64) == 2   # the debug entry plans rot = 32 only


# ---- the entry itself ------------------------------------------------------------------------------------------------------------------------------------

def test_entry_hygiene(lib, lab):
    ok = {ROW: (1000, 0, 0, 2), TOPK: (2, 128, 16, 4), SORT: (10000, 8, 0, 4), FUSEDQ: (4, 0, 0, 1), ACT: (4, 4096, 4096, 1)}
    for L in (lib, lab):
        f = L.qutlass_amd_debug_moe_launch_plan
        out = (ctypes.c_int * 4)()
        for op, (a, b, c, n) in ok.items():
            assert f(op, a, b, c, 256, out, 4) == n and f(op, a, b, c, 256, out, n) == n, op
            assert f(op, a, b, c, 256, None, 4) == -1 and f(op, a, b, c, 256, out, n - 1) == -1, op
            assert f(op, a, b, c, 0, out, 4) == -1 and f(op, a, b, c, -256, out, 4) == -1, op
        for op in (-1, 5, 6, 1 << 20):
            assert f(op, 4, 4096, 4096, 256, out, 4) == -1, op
    guard = (ctypes.c_int * 4)(-7, -7, -7, -7)
    assert lib.qutlass_amd_debug_moe_launch_plan(ROW, 1000, 0, 0, 256, guard, 2) == 2 and tuple(guard[2:]) == (-7, -7)   # writes what it returns, no more
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qutlass_amd.h")).read()
    assert not re.search(r"\bqutlass_amd_debug_moe_launch_plan\b", hdr), "debug entries stay out of the public header"
    from qutlass_amd import _lib

    assert "qutlass_amd_debug_moe_launch_plan" not in _lib.SYMBOLS


# ---- the two combine entries share their checks --------------------------------------------------------------------------------------------------------
# (arguments, the full qutlass_amd_last_error() text) of every rejected argument, in the entries' order; each case breaks one thing of GOOD.  bias_only: a check the
# bias form adds -- the plain form takes no such argument and accepts the call.
GOOD = dict(y=X, m=4, hdim=64, pos=X, w=X, t=3, topk=2, bias=X, offs=X, e=2, out=X)
COMBINE_REJECTS = [
    (dict(m=-1), "moe_combine: bad shape (y (-1, 64), 3 tokens)", False),
    (dict(t=-1), "moe_combine: bad shape (y (4, 64), -1 tokens)", False),
    (dict(hdim=0), "moe_combine: bad shape (y (4, 0), 3 tokens)", False),
    (dict(m=1 << 31), "moe_combine: bad shape (y (2147483648, 64), 3 tokens)", False),
    (dict(t=1 << 31), "moe_combine: bad shape (y (4, 64), 2147483648 tokens)", False),
    (dict(hdim=1 << 31), "moe_combine: bad shape (y (4, 2147483648), 3 tokens)", False),
    (dict(hdim=12), "moe_combine: the row length 12 must be a multiple of 8", False),
    (dict(topk=0), "moe_combine: bad shape: topk must be in [1, 32] (got 0)", False),
    (dict(topk=33), "moe_combine: bad shape: topk must be in [1, 32] (got 33)", False),
    (dict(y=X + 2), "moe_combine: y and out must be 16-byte aligned", False),
    (dict(out=X + 8), "moe_combine: y and out must be 16-byte aligned", False),
    (dict(e=0), "moe_combine: E must be in [1, 1024] (got 0)", True),
    (dict(e=1025), "moe_combine: E must be in [1, 1024] (got 1025)", True),
    (dict(bias=X + 8), "moe_combine: bias must be 16-byte aligned", True),
    (dict(offs=None), "moe_combine: a bias of E = 2 experts needs offs", True),
    (dict(offs=X + 2), "moe_combine: offs must be 4-byte aligned", True),
    (dict(y=None), "moe_combine: null pointer argument", False),
    (dict(pos=None), "moe_combine: null pointer argument", False),
    (dict(w=None), "moe_combine: null pointer argument", False),
    (dict(out=None), "moe_combine: null pointer argument", False),
    (dict(bias=None), "moe_combine: null pointer argument", True),
    # the order of the checks: shape before row length before topk before alignment before the bias checks before the T == 0 exit before the null pointers
    (dict(hdim=0, topk=0), "moe_combine: bad shape (y (4, 0), 3 tokens)", False),
    (dict(hdim=12, topk=0, y=X + 2), "moe_combine: the row length 12 must be a multiple of 8", False),
    (dict(topk=0, y=X + 2, e=0), "moe_combine: bad shape: topk must be in [1, 32] (got 0)", False),
    (dict(out=X + 8, e=0, pos=None), "moe_combine: y and out must be 16-byte aligned", False),
    (dict(e=0, t=0), "moe_combine: E must be in [1, 1024] (got 0)", True),
    (dict(e=0, pos=None), "moe_combine: E must be in [1, 1024] (got 0)", True),
]


def _combine(L, bias_form, a):
    if bias_form:
        return L.qutlass_amd_moe_combine_bias_bf16(a["y"], a["m"], a["hdim"], a["pos"], a["w"], a["t"], a["topk"], a["bias"], a["offs"], a["e"], a["out"], None)
    return L.qutlass_amd_moe_combine_bf16(a["y"], a["m"], a["hdim"], a["pos"], a["w"], a["t"], a["topk"], a["out"], None)


@pytest.mark.parametrize("case", range(len(COMBINE_REJECTS)))
def test_the_two_combine_entries_reject_alike_with_the_texts_they_always_had(case):
    from qutlass_amd import _lib

    L = _lib.load()
    bad, text, bias_only = COMBINE_REJECTS[case]
    args = {**GOOD, **bad}
    assert _combine(L, True, args) == INVALID and L.qutlass_amd_last_error().decode() == text
    if not bias_only:
        assert _combine(L, False, args) == INVALID and L.qutlass_amd_last_error().decode() == text
    elif args["t"] == 0:   # only the bias form sees this argument: the plain form has nothing to refuse and returns at once (with T > 0 it would go on to launch)
        assert _combine(L, False, args) == 0


def test_the_combine_entries_leave_at_t_zero_before_the_null_pointer_check():
    from qutlass_amd import _lib

    L = _lib.load()
    args = {**GOOD, "t": 0, "y": None, "pos": None, "w": None, "out": None}
    assert _combine(L, False, args) == 0 and _combine(L, True, {**args, "bias": None, "e": 1, "offs": None}) == 0
    assert _combine(L, True, {**args, "m": 0}) == 0 and _combine(L, False, {**args, "m": 0}) == 0
