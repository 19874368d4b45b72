"""The dense MX GEMMs' form list (csrc/gemm_mx_forms.hip.h MX_FORMS, read through qutlass_amd_debug_mx_forms; no GPU):

  * the table is well-formed, and its product rows are the numbers the plans are documented to return;
  * every variant qutlass_amd_debug_gemm_plan (MXFP4, MXFP8) and qutlass_amd_debug_ada_plan return over a seeded sweep is a product row whose ops mask holds the op;
  * every (product row, op) pair of the table is run by tests/_mx_cases.CASES -- a form cannot ship without its scale-range and footprint cases;
  * a planned split's workspace is splits x M x N x 4 bytes;
  * the debug entry is not part of the public header.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _mx_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("variant", "family", "tm", "tn", "wm", "wn", "depth", "ops", "product")
F4, F8, F8_E5M2, ADA = 1, 2, 4, 8                       # MxOp
OPS = {F4: ("mxf4", False), F8: ("mxf8", False), F8_E5M2: ("mxf8", True), ADA: ("ada", False)}
HEADER = open(os.path.join(ROOT, "qutlass_amd", "csrc", "gemm_mx_forms.hip.h")).read()
FAMILY = [n.strip() for n in re.search(r"enum MxFamily : int \{([^}]*)\}", HEADER).group(1).split(",")]    # names in the enum's order: a family's value is its index
RING, DECODE = FAMILY.index("MXF_RING"), FAMILY.index("MXF_DECODE")
PRODUCT = {24, 25, 27, 28, 29, 58, 60, 70, 71, 72, 73, 90, 98, 561, 562} | set(range(568, 576))

MS = list(range(1, 18)) + [24, 32, 33, 64, 65, 96, 128, 129, 192, 256, 384, 512, 1024, 2048, 4096, 8192]


@pytest.fixture(scope="module")
def lib():
    from qutlass_amd import _lib, build

    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def forms(lib):
    f = lib.qutlass_amd_debug_mx_forms
    f.restype, f.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    n = f(None, 0)
    out = (ctypes.c_int * (9 * n))()
    assert f(out, 9 * n) == n
    return [dict(zip(FIELDS, out[9 * i:9 * i + 9])) for i in range(n)]


def shapes(ebits, count=3000):
    """seeded: M from the batch sizes where a rule switches, N a multiple of 8 up to 65536 (a few beyond 2^22: the ldd rule), K a multiple of the op's alignment up to 32768"""
    rng = np.random.default_rng(20261020 + ebits)
    kal = 128 if ebits == 4 else 32
    for i in range(count):
        n = int(rng.integers(1, 8193)) * 8 if i % 50 else (1 << 22) + int(rng.integers(0, 64)) * 8
        k = int(rng.integers(1, 32768 // kal + 1)) * kal if i % 50 else kal * int(rng.integers(1, 5))
        yield MS[int(rng.integers(0, len(MS)))], n, k


def test_table_is_well_formed(forms):
    v = [f["variant"] for f in forms]
    assert len(set(v)) == len(v) and all(x > 0 for x in v)
    for f in forms:
        assert f["tm"] > 0 and f["tn"] > 0 and f["wm"] > 0 and f["wn"] > 0 and f["depth"] >= 0, f
        assert 0 <= f["family"] < len(FAMILY) and 0 < f["ops"] <= 15 and f["product"] in (0, 1), f
    assert {f["variant"] for f in forms if f["product"]} == PRODUCT
    tn = [f["tn"] for f in forms if f["family"] == DECODE]
    assert tn == sorted(tn) == [16, 32, 48, 56, 64]          # the plans take the first decode row that leaves one workgroup per CU
    assert not any(f["ops"] & ADA and f["ops"] & F4 == 0 for f in forms)   # the row-major-scale op is an MXFP4 op


def test_every_planned_variant_is_a_product_row_of_its_op(lib, forms):
    row = {f["variant"]: f for f in forms}
    plan = lib.qutlass_amd_debug_gemm_plan
    plan.restype = ctypes.c_int
    plan.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    ada = lib.qutlass_amd_debug_ada_plan
    ada.restype = ctypes.c_int
    ada.argtypes = [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    ws = lib.qutlass_amd_gemm_splitk_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_int64, [ctypes.c_int] + [ctypes.c_int64] * 3
    out = (ctypes.c_int * 24)()
    seen = {F4: set(), F8: set(), ADA: set()}
    splits = 0

    def check(op, need, cnt, shape):
        assert cnt >= 1, shape
        for i in range(min(cnt, 8)):
            f = row.get(out[3 * i])
            assert f is not None and f["product"] and f["ops"] & need == need, (op, shape, out[3 * i])
            seen[op].add(out[3 * i])

    for ebits, op, need in ((4, F4, F4), (8, F8, F8 | F8_E5M2)):    # (the MXFP8 plan does not look at A's format: both must have the kernel)
        for m, n, k in shapes(ebits):
            need_ws = ws(ebits, m, n, k)
            for avail in (0, need_ws, 1 << 40):
                cnt = plan(ebits, m, n, k, avail, out, 8)
                check(op, need, cnt, (ebits, m, n, k, avail))
                if cnt == 1 and out[2] > 1:
                    splits += 1
                    assert avail >= need_ws == out[2] * m * n * 4, (ebits, m, n, k, avail, out[2], need_ws)
                    assert row[out[0]]["family"] == RING              # the only forms a plan splits
            if ebits == 4:
                check(ADA, ADA, ada(m, n, k, out, 8), ("ada", m, n, k))
    assert splits >= 50 and all(len(s) >= 6 for s in seen.values()), (splits, seen)


def test_every_product_row_of_every_op_is_run_on_the_gpu(forms):
    for f in forms:
        for bit, (op, a5) in OPS.items():
            if f["product"] and f["ops"] & bit:
                covered = {c.variant for c in mc.CASES if c.op == op and c.a5 == a5}
                assert f["variant"] in covered, f"form {f['variant']} of {op}{' (e5m2 A)' if a5 else ''} has no case in tests/_mx_cases.py"


def test_debug_entry_is_not_in_the_public_header():
    assert "qutlass_amd_debug_mx_forms" not in open(os.path.join(ROOT, "include", "qutlass_amd.h")).read()
