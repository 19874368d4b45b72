"""The three grouped GEMMs (grouped_matmul_mxf4 / mxf8 / nvf4_bf16_tn) share one host path described by a format table (gemm_mx_grouped.hip.h: GroupedFormat):
the same boundary sweep goes through each C entry and each debug plan entry, every case must end the same way in all three, and a plan entry's workgroup count is
(cdiv(M, TM) + E) * cdiv(N, TN) for the tile of the form it picked.  No GPU needed: an entry is called only where it returns before a launch (rejected, or M == 0),
the accepted cases with M > 0 go through the plan entries, which run the same checks."""
import ctypes

import pytest

# per format: C entry, debug plan entry, bytes of a K-element row, whether the entry takes a_format, and the tiles of its four forms as the form documentation gives
# them (capi.hip / DESIGN.md section 5): MX 32x32, 32x16, 64x32 wave-owned and the 64x64 ring; NVFP4 32x32, 64x32 wave-owned and 64x64, 128x128 tile kernel
MX_TILES = [(32, 32), (32, 16), (64, 32), (64, 64)]
FORMATS = {
    "mxf4": dict(entry="qutlass_amd_grouped_matmul_mxf4_bf16_tn", plan="qutlass_amd_debug_grouped_plan", row_bytes=lambda K: K // 2, a_format=False,
                 form0=590, tiles=MX_TILES, picks={590, 593}, want=lambda M, K, E: 590 if M <= 32 * E and K <= 1024 else 593),
    "mxf8": dict(entry="qutlass_amd_grouped_matmul_mxf8_bf16_tn", plan="qutlass_amd_debug_grouped_mxf8_plan", row_bytes=lambda K: K, a_format=True,
                 form0=594, tiles=MX_TILES, picks={594, 597}, want=lambda M, K, E: 594 if M <= 32 * E and K >= 8192 else 597),
    "nvf4": dict(entry="qutlass_amd_grouped_matmul_nvf4_bf16_tn", plan="qutlass_amd_debug_grouped_nvf4_plan", row_bytes=lambda K: K // 2, a_format=False,
                 form0=598, tiles=[(32, 32), (64, 32), (64, 64), (128, 128)], picks={598, 600, 601},
                 want=lambda M, K, E: 598 if M <= 16 * E and K >= 8192 else 600 if M <= 48 * E else 601),
}
BASE = dict(M=0, N=256, K=512, E=8, n_alpha=1)
OK = None   # a case's expectation: accepted, or the words its rejection must carry


def _cdiv(a, b):
    return -(-a // b)


def _max_grid(fmt, M, N, E):
    return max((_cdiv(M, tm) + E) * _cdiv(N, tn) for tm, tn in FORMATS[fmt]["tiles"])


def _first_n_at_2p24(fmt, M, E):
    """the first N (a multiple of 8) at which some form of the format needs 2^24 workgroups"""
    lo, hi = 8, 1 << 30   # the grid grows with N: bisect over N / 8
    while lo < hi:
        mid = (lo + hi) // 16 * 8
        if _max_grid(fmt, M, mid, E) >= 1 << 24:
            hi = mid
        else:
            lo = mid + 8
    assert _max_grid(fmt, M, lo, E) >= 1 << 24 > _max_grid(fmt, M, lo - 8, E)
    return lo


def _cases(fmt):
    """(id, arguments over BASE, expectation): the same ids for every format; the 2 GiB and workgroup boundaries sit where that format's row bytes / tiles put them"""
    rb = FORMATS[fmt]["row_bytes"]
    c = []
    for E, want in ((0, "E must be in [1, 1024]"), (1, OK), (1024, OK), (1025, "E must be in [1, 1024]")):
        c.append((f"E={E}", dict(E=E), want))
    for name, n_alpha, want in (("0", 0, "alpha must have 1 or E"), ("1", 1, OK), ("E", BASE["E"], OK), ("E+1", BASE["E"] + 1, "alpha must have 1 or E")):
        c.append((f"n_alpha={name}", dict(n_alpha=n_alpha), want))
    for K, want in ((0, "K must be a positive multiple of 128"), (64, "K must be a positive multiple of 128"), (128, OK), (192, "K must be a positive multiple of 128")):
        c.append((f"K={K}", dict(K=K), want))
    for N, want in ((0, "N positive"), (8, OK), (12, "N must be a multiple of 8")):
        c.append((f"N={N}", dict(N=N), want))
    for M, want in ((-1, "M must be >= 0"), (0, OK)):
        c.append((f"M={M}", dict(M=M), want))
    # 2 GiB of row bytes, at K = 131072 (the grid stays small)
    K = 131072
    n2g = _cdiv(1 << 31, rb(K))
    assert n2g % 8 == 0
    c.append(("N at 2 GiB", dict(N=n2g, K=K), "one expert's weight"))
    c.append(("N below 2 GiB", dict(N=n2g - 8, K=K), OK))
    m2g = _cdiv(1 << 31, rb(K))
    c.append(("M at 2 GiB", dict(M=m2g, K=K), "token matrix"))
    c.append(("M below 2 GiB", dict(M=m2g - 1, K=K), OK))
    # ... and at K = 128 the last row count below 2 GiB passes that check and stops at the grid bound (an entry can be called on it: rejected)
    c.append(("M below 2 GiB, K=128", dict(M=_cdiv(1 << 31, rb(128)) - 1, N=1024, K=128), "2^24 workgroups"))
    # an output of 2^40 elements (K = 128: 2^20 rows are far below 2 GiB); one row less passes that check and stops at the grid bound
    c.append(("2^40 outputs", dict(M=1 << 20, N=1 << 20, K=128), "2^40"))
    c.append(("below 2^40 outputs", dict(M=(1 << 20) - 1, N=1 << 20, K=128), "2^24 workgroups"))
    # 2^24 workgroups, without rows (an entry returns before a launch) and with 32 rows per expert
    for M in (0, 32 * 1024):
        n = _first_n_at_2p24(fmt, M, 1024)
        c.append((f"2^24 workgroups, M={M}", dict(M=M, N=n, K=128, E=1024), "2^24 workgroups"))
        c.append((f"below 2^24 workgroups, M={M}", dict(M=M, N=n - 8, K=128, E=1024), OK))
    # N * row bytes = 2^69: the product does not fit in 64 bits, the comparison must not form it
    c.append(("N * K overflows", dict(M=0, N=1 << 40, K=1 << 30), "below 2 GiB"))
    return c


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()  # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    L = _lib.load()
    for f in FORMATS.values():
        p = getattr(L, f["plan"])
        p.restype = ctypes.c_int
        p.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int64)]
    return L


def _run_entry(lib, fmt, a):
    """(return code, the rejection's message)"""
    d = ctypes.c_void_p(0x1000)   # never dereferenced: every call here returns before a launch
    args = [d, d, d, d, d, a["n_alpha"], d, d, a["M"], a["N"], a["K"], a["E"]] + ([0] if FORMATS[fmt]["a_format"] else []) + [None]
    rc = getattr(lib, FORMATS[fmt]["entry"])(*args)
    return rc, lib.qutlass_amd_last_error().decode() if rc else ""


def _run_plan(lib, fmt, a):
    """('ok', form, workgroups) or ('rejected', message)"""
    grid = ctypes.c_int64(-1)
    v = getattr(lib, FORMATS[fmt]["plan"])(a["M"], a["N"], a["K"], a["E"], ctypes.byref(grid))
    if v == -1:
        return "rejected", lib.qutlass_amd_last_error().decode()
    return "ok", v, grid.value


def _check_plan(fmt, a, got):
    f = FORMATS[fmt]
    _, v, grid = got
    assert v == f["want"](a["M"], a["K"], a["E"]), (fmt, a, v)
    TM, TN = f["tiles"][v - f["form0"]]
    assert grid == (0 if a["M"] == 0 else (_cdiv(a["M"], TM) + a["E"]) * _cdiv(a["N"], TN)), (fmt, a, v, grid)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_boundary_sweep(lib, fmt):
    from qutlass_amd._lib import QAMD_ERR_INVALID

    for cid, over, want in _cases(fmt):
        a = dict(BASE, **over)
        if want is not OK or a["M"] == 0:   # the entry returns before a launch
            rc, msg = _run_entry(lib, fmt, a)
            if want is OK:
                assert rc == 0, (fmt, cid, rc, msg)
            else:
                assert rc == QAMD_ERR_INVALID and want in msg, (fmt, cid, rc, msg)
                assert FORMATS[fmt]["entry"][len("qutlass_amd_"):] in msg, (fmt, cid, msg)   # the message names the op
        if a["n_alpha"] == 1:   # (a plan entry has no alpha)
            got = _run_plan(lib, fmt, a)
            if want is OK:
                assert got[0] == "ok", (fmt, cid, got)
                _check_plan(fmt, a, got)
            else:
                assert got[0] == "rejected" and want in got[1], (fmt, cid, got)


def test_the_three_formats_agree(lib):
    """the same logical case ends the same way, with the same return code, in every entry and every plan entry"""
    per_fmt = {fmt: _cases(fmt) for fmt in FORMATS}
    assert len({tuple(cid for cid, _, _ in cs) for cs in per_fmt.values()}) == 1
    for i, (cid, _, want) in enumerate(per_fmt["mxf4"]):
        entry_rcs, plan_rejects = set(), set()
        for fmt, cs in per_fmt.items():
            a = dict(BASE, **cs[i][1])
            assert cs[i][2] == want
            if want is not OK or a["M"] == 0:
                entry_rcs.add(_run_entry(lib, fmt, a)[0])
            if a["n_alpha"] == 1:
                plan_rejects.add(_run_plan(lib, fmt, a)[0])
        assert len(entry_rcs) <= 1 and len(plan_rejects) <= 1, (cid, entry_rcs, plan_rejects)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_plan_workgroups_are_the_picked_forms_tile(lib, fmt):
    forms = set()
    for E in (1, 8, 1024):
        for M in (1, 16 * E, 16 * E + 1, 32 * E, 32 * E + 1, 48 * E, 48 * E + 1, 64 * E):
            for K in (768, 1024, 1152, 8064, 8192):
                for N in (8, 520, 2048):
                    a = dict(M=M, N=N, K=K, E=E)
                    got = _run_plan(lib, fmt, a)
                    assert got[0] == "ok", (fmt, a, got)
                    _check_plan(fmt, a, got)
                    forms.add(got[1])
    assert forms == FORMATS[fmt]["picks"]   # every form the rule can pick was met
