"""The rotate + quantize family without a GPU: the eight C entries qutlass_amd_fused_quantize_{mx,nv}[_blocked], qutlass_amd_fused_silu_mul_quantize_{mx,nv} and
qutlass_amd_fused_gather_quantize_{mx,nv} share their checks (capi.hip: QuantFormat, quant_check_*), but each keeps its own ORDER of them, and which message a call
that is wrong in two ways gets is part of the contract.  `expect()` below states every entry's chain independently of the library -- return code and the full
qutlass_amd_last_error() text -- and a grid over rotation x method x blocked x mask x one or two broken arguments must end exactly as it says.  Dummy addresses only:
a call is made only where the chain ends before the launch (a rejection, or a zero-row accept), so nothing here reaches HIP.  The same grid, with a few hundred
more shapes, is what tools/quantize_family_diff.py runs against two builds of the library.  Below that: the functional torch ops' shapes and the wrappers' errors."""
import itertools
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import qutlass_amd as q
from qutlass_amd import _lib
from qutlass_amd.utils import get_padded_shape_mx, get_padded_shape_nv

OK, INVALID = _lib.QAMD_OK, _lib.QAMD_ERR_INVALID
LAUNCH = "launch"   # expect(): every check passes -- the call would go on to HIP and is never made
X = 0x10000         # a 16-byte aligned dummy address: nothing below dereferences it
ROTS = (0, 8, 16, 32, 48, 64, 128, 256)
METHODS = (-1, 0, 1, 2)
P31 = 1 << 31

# entry -> (kind, nv, arguments in the C order); `stream` is always null
ENTRIES = {
    "qutlass_amd_fused_quantize_mx": ("flat", False, ("x", "h", "rot", "numel", "method", "out", "sf", "mask")),
    "qutlass_amd_fused_quantize_nv": ("flat", True, ("x", "h", "rot", "numel", "method", "gs", "out", "sf")),
    "qutlass_amd_fused_quantize_mx_blocked": ("blocked", False, ("x", "h", "rot", "rows", "k", "method", "out", "sf", "mask")),
    "qutlass_amd_fused_quantize_nv_blocked": ("blocked", True, ("x", "h", "rot", "rows", "k", "method", "gs", "out", "sf")),
    "qutlass_amd_fused_silu_mul_quantize_mx": ("gated", False, ("x", "h", "rot", "rows", "k", "method", "blocked", "out", "sf")),
    "qutlass_amd_fused_silu_mul_quantize_nv": ("gated", True, ("x", "h", "rot", "rows", "k", "method", "gs", "blocked", "out", "sf")),
    "qutlass_amd_fused_gather_quantize_mx": ("gather", False, ("x", "h", "rot", "t", "k", "src_row", "m", "method", "out", "sf")),
    "qutlass_amd_fused_gather_quantize_nv": ("gather", True, ("x", "h", "rot", "t", "k", "src_row", "m", "method", "gs", "out", "sf")),
}
NAMES = {"flat": "fusedQuantize%s", "blocked": "fusedQuantize%sBlocked", "gated": "fusedSiluMulQuantize%s", "gather": "fusedGatherQuantize%s"}
BASE = dict(x=X, h=X, out=X, sf=X, gs=X, mask=None, src_row=X, rot=32, method=0, blocked=0, numel=1024, rows=4, k=256, t=4, m=4)


def _i64(v):   # what the library's int64 arithmetic makes of a product
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def expect(entry, a):
    """(return code, message) the entry must give for the arguments a (a dict over BASE), or LAUNCH: the entry's checks in the entry's order."""
    kind, nv, _ = ENTRIES[entry]
    name = NAMES[kind] % ("Nv" if nv else "Mx") + ("Blocked" if kind == "gated" and a["blocked"] else "")
    rot, method, h, x = a["rot"], a["method"], a["h"] or 0, a["x"] or 0
    mask = a["mask"] if not nv and kind in ("flat", "blocked") else None
    rots = "16, 32, 64, or 128" if nv else "32, 64, or 128"
    rot_ok = rot in ((16, 32, 64, 128) if nv else (32, 64, 128))
    rp = max(rot, 32)
    bad = lambda text: (INVALID, f"{name}: {text}")
    null = bad("null pointer argument")
    bad_rot = bad(f"Unsupported rotation size {rot}; expected {'32' if mask else rots}.")
    bad_method = bad(f"invalid method {method}")
    bad_h = bad("the rotation matrix must be 16-byte aligned for rotation sizes >= 64")
    outs_null = not a["h"] or not a["out"] or not a["sf"] or (nv and not a["gs"])
    if kind in ("flat", "blocked"):
        rows, k = a["rows"], a["k"]
        if kind == "blocked" and (rows <= 0 or k <= 0 or rows >= P31 or k >= P31):
            return bad(f"bad shape ({rows}, {k})")
        numel = rows * k if kind == "blocked" else a["numel"]
        if not a["x"] or outs_null:
            return null
        if not rot_ok:
            return bad_rot
        if numel <= 0 or numel % rot:
            return bad(f"A must be divisible by {rot}")
        if numel * 2 >= 1 << 32:
            return bad("more than 2^31 elements is not supported")
        if method not in (0, 1):
            return bad_method
        if mask and method != 0:
            return bad("the clip mask is only defined for method quest")
        if kind == "blocked" and k % rp:
            return bad(f"the row length {k} must be a multiple of {'' if nv else 'the rotation size '}{rp} and divide numel")
        if rot >= 64 and h % 16:
            return bad_h
        return LAUNCH   # (a mask with rot 64 / 128 is refused after the launch set-up: not reachable without HIP)
    if not rot_ok:
        return bad_rot
    if method not in (0, 1):
        return bad_method
    if kind == "gated":
        rows, inter = a["rows"], a["k"]
        if rows < 0 or inter <= 0 or rows >= P31 or inter >= P31:
            return bad(f"bad shape ({rows}, 2 * {inter})")
        if inter % rp:
            return bad(f"the gate / up width {inter} must be a multiple of {rp}")
        if x % 16:
            return bad("x must be 16-byte aligned")
        if rows * inter >= 1 << 29:
            return bad(f"x (rows * 2 * inter * 2 = {_i64(rows * inter * 4)} bytes) must stay below 2 GiB")
        if rows == 0:
            return OK, None
        if not a["x"] or outs_null:
            return null
    else:
        t, k, m, src = a["t"], a["k"], a["m"], a["src_row"] or 0
        if t < 0 or m < 0 or k <= 0 or t >= P31 or m >= P31 or k >= P31:
            return bad(f"bad shape (x ({t}, {k}), {m} indices)")
        if k % rp:
            return bad(f"the row length {k} must be a multiple of {rp}")
        if x % 16 or src % 4:
            return bad("x must be 16-byte aligned (and src_row 4-byte aligned)")
        if t * k >= 1 << 30:
            return bad(f"x (rows * k * 2 = {t * k * 2} bytes) must stay below 2 GiB")
        if m * k >= P31:
            return bad("more than 2^31 elements is not supported")
        if m == 0:
            return OK, None
        if (not a["x"] and t > 0) or not a["src_row"] or outs_null:
            return null
    if rot >= 64 and h % 16:
        return bad_h
    return LAUNCH


def call(lib, entry, a):
    """(return code, message or None when accepted) of one call"""
    rc = getattr(lib, entry)(*[a[n] for n in ENTRIES[entry][2]], None)
    return rc, (lib.qutlass_amd_last_error().decode() if rc != OK else None)


# one broken argument each; the grid applies every one, and every pointer fault together with every shape fault
POINTERS = [dict(), dict(x=None), dict(h=None), dict(out=None), dict(sf=None), dict(gs=None), dict(src_row=None), dict(h=X + 2), dict(h=X + 8), dict(x=X + 4),
            dict(src_row=X + 2), dict(x=X + 4, src_row=X + 2)]
SHAPES = {
    "flat": [dict(numel=n) for n in (1024, 0, -32, 1000, 48, 16, P31 - 128, P31, P31 + 128, 1 << 33)],
    "blocked": [dict(rows=r, k=k) for r, k in ((4, 256), (0, 256), (4, 0), (-1, 256), (4, -256), (P31, 256), (4, P31), (P31 - 1, 128), (4, 48), (4, 96), (4, 32),
                                                 (4, 160), (3, 256), (1, 16), (1 << 20, 1 << 11), (1 << 19, 1 << 11))],
    "gated": [dict(rows=r, k=k) for r, k in ((4, 256), (0, 256), (0, 0), (0, 48), (-1, 256), (4, 0), (4, -256), (P31, 256), (4, P31), (4, 48), (4, 32), (4, 160),
                                               (1 << 15, 1 << 14), (1 << 21, 256), ((1 << 21) - 1, 256), (0, P31 - 128))],
    "gather": [dict(t=t, k=k, m=m) for t, k, m in ((4, 256, 4), (4, 256, 0), (0, 256, 0), (0, 256, 4), (-1, 256, 4), (4, 0, 4), (4, -256, 4), (4, 256, -1),
                                                     (P31, 256, 4), (4, P31, 4), (4, 256, P31), (4, 48, 4), (4, 32, 4), (4, 160, 0), (1 << 15, 1 << 15, 4),
                                                     ((1 << 22) - 1, 256, 4), (4, 1 << 20, 1 << 11), (4, 1 << 20, (1 << 11) - 1), (0, 1 << 20, 1 << 11))],
}


CHECKS = {"flat": 6, "blocked": 8, "gated": 9, "gather": 10}   # distinct endings of each kind's chain


def cases(entry, shapes=None, pointers=POINTERS):
    """every argument set of the grid for one entry, as dicts over BASE"""
    kind, nv, args = ENTRIES[entry]
    blocked = (0, 1) if "blocked" in args else (0,)
    masks = (None, X) if "mask" in args else (None,)
    for rot, method, b, mask, shape, ptr in itertools.product(ROTS, METHODS, blocked, masks, shapes or SHAPES[kind], pointers):
        if any(key not in args for key in ptr):
            continue
        yield {**BASE, **shape, **ptr, "rot": rot, "method": method, "blocked": b, "mask": mask}


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_check_of_the_entry_in_its_order(entry):
    lib = _lib.load()
    made = ends = 0
    seen = set()
    for a in cases(entry):
        want = expect(entry, a)
        if want == LAUNCH:
            continue
        got = call(lib, entry, a)
        assert got == want, (entry, a)
        made += 1
        ends += want[0] == OK
        seen.add(re.sub(r"-?\d+", "#", (want[1] or "accepted").split(": ", 1)[-1]))
    kind, nv, _ = ENTRIES[entry]
    # every way the chain can end did end some call: the checks of the kind (the gated and the gathering entries count their zero-row accept), and for MX the
    # two more that come with the clip mask (the "expected 32" wording of the rotation check, and mask-needs-quest)
    assert made >= 2000 and len(seen) == CHECKS[kind] + (0 if nv or kind in ("gated", "gather") else 2), (made, sorted(seen))
    assert (ends > 0) == (kind in ("gated", "gather"))


def _one(entry, **kw):
    return call(_lib.load(), entry, {**BASE, **kw})


def test_which_message_wins_when_two_things_are_wrong():
    """literal pins, one or more per entry: the orders differ between the entries on purpose"""
    mx, nv = "qutlass_amd_fused_quantize_mx", "qutlass_amd_fused_quantize_nv"
    # plain: null pointer before rotation before size before method before mask-needs-quest before the alignment of h
    assert _one(mx, x=None, rot=48) == (INVALID, "fusedQuantizeMx: null pointer argument")
    assert _one(mx, rot=16, numel=1000) == (INVALID, "fusedQuantizeMx: Unsupported rotation size 16; expected 32, 64, or 128.")
    assert _one(mx, rot=16, mask=X, method=1) == (INVALID, "fusedQuantizeMx: Unsupported rotation size 16; expected 32.")
    assert _one(mx, rot=64, numel=1000, method=2) == (INVALID, "fusedQuantizeMx: A must be divisible by 64")
    assert _one(mx, numel=P31, method=2) == (INVALID, "fusedQuantizeMx: more than 2^31 elements is not supported")
    assert _one(mx, method=1, mask=X, h=X + 2) == (INVALID, "fusedQuantizeMx: the clip mask is only defined for method quest")
    assert _one(mx, rot=128, method=2, h=X + 2) == (INVALID, "fusedQuantizeMx: invalid method 2")
    assert _one(nv, gs=None, rot=8) == (INVALID, "fusedQuantizeNv: null pointer argument")
    assert _one(nv, rot=8, method=-1) == (INVALID, "fusedQuantizeNv: Unsupported rotation size 8; expected 16, 32, 64, or 128.")
    assert _one(nv, rot=64, h=X + 8) == (INVALID, "fusedQuantizeNv: the rotation matrix must be 16-byte aligned for rotation sizes >= 64")
    # blocked: the shape comes first of all, the row length after the method; the two formats word the row length differently (MX names its unit)
    mxb, nvb = mx + "_blocked", nv + "_blocked"
    assert _one(mxb, rows=0, x=None) == (INVALID, "fusedQuantizeMxBlocked: bad shape (0, 256)")
    assert _one(mxb, rot=64, k=96, rows=2, method=2) == (INVALID, "fusedQuantizeMxBlocked: invalid method 2")
    assert _one(mxb, rot=64, k=96, rows=2) == (INVALID, "fusedQuantizeMxBlocked: the row length 96 must be a multiple of the rotation size 64 and divide numel")
    assert _one(nvb, rot=16, k=48, rows=2, h=None) == (INVALID, "fusedQuantizeNvBlocked: null pointer argument")
    assert _one(nvb, rot=16, k=48, rows=2) == (INVALID, "fusedQuantizeNvBlocked: the row length 48 must be a multiple of 32 and divide numel")
    assert _one(nvb, rows=4, k=P31, rot=0) == (INVALID, f"fusedQuantizeNvBlocked: bad shape (4, {P31})")
    # gated: rotation and method before the shape; zero rows are accepted before the pointers are looked at, but after the 2 GiB limit
    gmx, gnv = "qutlass_amd_fused_silu_mul_quantize_mx", "qutlass_amd_fused_silu_mul_quantize_nv"
    assert _one(gmx, rot=16, rows=-1) == (INVALID, "fusedSiluMulQuantizeMx: Unsupported rotation size 16; expected 32, 64, or 128.")
    assert _one(gmx, blocked=1, method=2, rows=-1) == (INVALID, "fusedSiluMulQuantizeMxBlocked: invalid method 2")
    assert _one(gmx, rows=-1, k=48, x=X + 4) == (INVALID, "fusedSiluMulQuantizeMx: bad shape (-1, 2 * 48)")
    assert _one(gmx, k=48, x=X + 4) == (INVALID, "fusedSiluMulQuantizeMx: the gate / up width 48 must be a multiple of 32")
    assert _one(gnv, rot=16, k=16, x=None) == (INVALID, "fusedSiluMulQuantizeNv: the gate / up width 16 must be a multiple of 32")
    assert _one(gnv, x=X + 4, rows=1 << 21) == (INVALID, "fusedSiluMulQuantizeNv: x must be 16-byte aligned")
    assert _one(gnv, blocked=1, rows=1 << 15, k=1 << 14, h=None) == (INVALID, "fusedSiluMulQuantizeNvBlocked: x (rows * 2 * inter * 2 = 2147483648 bytes) must stay below 2 GiB")
    assert _one(gnv, rows=0, x=None, h=None, out=None, sf=None, gs=None) == (OK, None)
    assert _one(gnv, gs=None, rot=128, h=X + 2) == (INVALID, "fusedSiluMulQuantizeNv: null pointer argument")
    # gather: as gated, with its own shape, alignment and size messages; a null x is fine while it has no rows
    amx, anv = "qutlass_amd_fused_gather_quantize_mx", "qutlass_amd_fused_gather_quantize_nv"
    assert _one(amx, method=-1, t=-1) == (INVALID, "fusedGatherQuantizeMx: invalid method -1")
    assert _one(amx, t=-1, k=48) == (INVALID, "fusedGatherQuantizeMx: bad shape (x (-1, 48), 4 indices)")
    assert _one(amx, k=48, src_row=X + 2) == (INVALID, "fusedGatherQuantizeMx: the row length 48 must be a multiple of 32")
    assert _one(amx, src_row=X + 2, t=1 << 15, k=1 << 15) == (INVALID, "fusedGatherQuantizeMx: x must be 16-byte aligned (and src_row 4-byte aligned)")
    assert _one(anv, t=1 << 15, k=1 << 15, m=1 << 16) == (INVALID, "fusedGatherQuantizeNv: x (rows * k * 2 = 2147483648 bytes) must stay below 2 GiB")
    assert _one(anv, k=1 << 20, m=1 << 11, h=None) == (INVALID, "fusedGatherQuantizeNv: more than 2^31 elements is not supported")
    assert _one(anv, m=0, h=None, src_row=None, out=None, sf=None, gs=None) == (OK, None)
    assert _one(anv, t=0, x=None, gs=None) == (INVALID, "fusedGatherQuantizeNv: null pointer argument")
    assert _one(anv, t=0, x=None, rot=64, h=X + 8) == (INVALID, "fusedGatherQuantizeNv: the rotation matrix must be 16-byte aligned for rotation sizes >= 64")


# ---- the torch and Python layers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 768), (2, 35, 768)])
def test_the_eight_functional_ops_give_the_padded_shapes(shape):
    """result shapes and dtypes of every functional op against get_padded_shape_* of the operand it quantizes: the tensor itself, its (.., I) activation, its gathered rows"""
    q.ops.register_torch_ops()
    amd = torch.ops.qutlass_amd
    with FakeTensorMode():
        x = torch.empty(*shape, dtype=torch.bfloat16, device="cuda")
        x2 = x.view(-1, shape[-1])
        h = torch.empty(32, 32, dtype=torch.bfloat16, device="cuda")
        gs = torch.empty(1, device="cuda")
        src = torch.empty(45, dtype=torch.int32, device="cuda")
        act = torch.empty(*shape[:-1], shape[-1] // 2, dtype=torch.bfloat16, device="cuda")
        gathered = torch.empty(45, shape[-1], dtype=torch.bfloat16, device="cuda")
        runs = [("quantize_mx", (x, h, 0), x, False, False), ("quantize_nv", (x, h, gs, 1), x, True, False),
                ("quantize_mx_blocked", (x, h, 0), x, False, True), ("quantize_nv_blocked", (x, h, gs, 1), x, True, True),
                ("silu_mul_quantize_mx", (x, h, 0, False), act, False, False), ("silu_mul_quantize_mx", (x, h, 1, True), act, False, True),
                ("silu_mul_quantize_nv", (x, h, gs, 0, False), act, True, False), ("silu_mul_quantize_nv", (x, h, gs, 1, True), act, True, True),
                ("gather_quantize_mx", (x2, h, src, 0), gathered, False, False), ("gather_quantize_nv", (x2, h, src, gs, 1), gathered, True, False)]
        assert {r[0] for r in runs} == {f"{kind}_{fmt}{tail}" for kind, tail in (("quantize", ""), ("quantize", "_blocked"), ("silu_mul_quantize", ""), ("gather_quantize", ""))
                                        for fmt in ("mx", "nv")}
        for op, args, operand, nv, blocked in runs:
            codes, sf = getattr(amd, op)(*args)
            pr, pc = (get_padded_shape_nv if nv else get_padded_shape_mx)(operand)
            assert codes.shape == (*operand.shape[:-1], operand.size(-1) // 2) and codes.dtype == torch.uint8 and codes.device.type == "cuda", op
            assert sf.shape == ((pr * pc,) if blocked else (pr, pc)) and sf.dtype == (torch.float8_e4m3fn if nv else torch.float8_e8m0fnu), op
    assert get_padded_shape_mx(torch.empty(70, 768)) == (128, 24) and get_padded_shape_nv(torch.empty(2, 35, 384)) == (128, 24)


def test_every_wrapper_refuses_a_bad_method_in_the_same_words():
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    h = torch.zeros(32, 32, dtype=torch.bfloat16)
    gs = torch.ones(1)
    src = torch.zeros(4, dtype=torch.int32)
    wrappers = [(q.fusedQuantizeMx, (x, h)), (q.fusedQuantizeNv, (x, h, gs)), (q.fusedQuantizeMxBlocked, (x, h)), (q.fusedQuantizeNvBlocked, (x, h, gs)),
                (q.fusedSiluMulQuantizeMx, (x, h)), (q.fusedSiluMulQuantizeMxBlocked, (x, h)), (q.fusedSiluMulQuantizeNv, (x, h, gs)),
                (q.fusedSiluMulQuantizeNvBlocked, (x, h, gs)), (q.fusedGatherQuantizeMx, (x, h, src)), (q.fusedGatherQuantizeNv, (x, h, gs, src)),
                (q.fused_quantize_matmul_mxf4_bf16_tn, (x, h, x, x, gs))]
    for fn, args in wrappers:
        with pytest.raises(ValueError) as e:
            fn(*args, method="nope")
        assert str(e.value) == "invalid method 'nope', must be 'quest' or 'abs_max'", fn.__name__
    with pytest.raises(ValueError) as e:
        q.fusedQuantizeMx(x, h, method="abs_max", return_mask=True)
    assert str(e.value) == "return_mask is only supported for method 'quest'"
