"""What the extension layer (qutlass_amd/csrc/torch_ext.cpp) rejects, op by op and check by check, with the message as it is.

The ops are registered for the CUDA dispatch key only, so their checks fire for GPU tensors alone: every case below is ONE call of one op of `_qutlass_C` or
`qutlass_amd` on the smallest tensors that reach one check, and asserts the text of the error (`torch_ext.cpp` stands for the `file:line` part).  A rejected call
launches nothing.  Every case starts from arguments the op accepts (so that a check which did not fire would meet a well-formed call, not an out-of-bounds one)
and changes what the case names.

The three generic checks (include/bindings_utils.h of the reference) are pinned with their numbering: per op the LAST tensor of the contiguity list is made
non-contiguous (`argument #k 'name'`), one CPU tensor stands among GPU ones, and -- on a machine with a second GPU -- one tensor lives on cuda:1.  Where an op's
device list is longer than its contiguity list (alpha of the non-FP8 GEMMs and of fusedQuantizeMatmulMxf4, the global scale of the NVFP4 quantizers, alpha of
backward_qt_bf16) a non-contiguous tensor of the difference goes THROUGH the contiguity pass and meets a later check; the four QAT-backward ops make no
same-device check, and a tensor on cuda:1 goes through to a later check likewise.

Checks no caller can reach (an earlier check shadows them), by op and message:
  matmul_* (all five)             "B K-dim must be >= <kmin>"   the inner dimensions match and "A K-dim must be >=" has passed: B's K is A's
  swigluOaiAndMul_, fusedSwigluOaiQuantizeMx[f8]_, moeCombineBias_
                                  "the number of experts must be in [1, 1024]" for E < 1: a bias of no rows is empty, which means "no bias" (E > 1024 is below)
  fusedSiluMulQuantizeMxf8_, fusedGatherQuantizeMxf8_
                                  "method must be 0 (quest) or 1 (abs_max)": the schema has no method, the op passes abs_max
  to_blocked                      "to_blocked: expected a GPU tensor (no CPU path in qutlass_amd)": a CPU tensor never reaches the CUDA kernel (NotImplementedError
                                  of the dispatcher, tests/test_gpu_parity.py)
  every op                        the "another DeviceType" wording of the device check: there is no third device type on the machine
What the C ABI rejects behind these checks (alignment, size limits, the method of the blocked quantizers) comes back through the same STD_TORCH_CHECK with the
library's own message; one case (matmul_mxf4_bf16_tn, K = 96) pins that path, the messages themselves are pinned where the C ABI is tested.
"""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, U8, I8, I32, I64, F32, F64 = torch.bfloat16, torch.uint8, torch.int8, torch.int32, torch.int64, torch.float32, torch.float64
E8, E4, E5 = torch.float8_e8m0fnu, torch.float8_e4m3fn, torch.float8_e5m2

CASES = []   # (id, qualified op, base: () -> {argument: value} in schema order, change: base -> {argument: value}, message, needs a second GPU)


def z(*shape, dtype=BF):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def nc(t):
    """t's shape and dtype, not contiguous (the last dimension needs two elements)"""
    v = torch.zeros((*t.shape[:-1], 2 * t.shape[-1]), dtype=t.dtype, device=t.device)[..., ::2]
    assert not v.is_contiguous() and v.shape == t.shape
    return v


def case(tag, qual, base, change, msg, second_gpu=False):
    CASES.append((f"{qual.split('::')[1]}-{tag}", qual, base, change, msg, second_gpu))


def generic(qual, op, base, contig, device_only=(), same=True, through=None, fall=None):
    """The three generic checks of one op.  contig: [(argument, name in the message)], the contiguity list in order; device_only: what joins the device passes
    behind it.  through: (change, message) -- a non-contiguous tensor of device_only meets that later check.  same=False: the op makes no same-device check, and
    with fall = (change, message) a tensor on cuda:1 meets that later check."""
    last, name = contig[-1]
    case("contiguous", qual, base, lambda a: {last: nc(a[last])},
         f"Expected contiguous tensor, but got non-contiguous tensor for argument #{len(contig) - 1} '{name}' (while checking arguments for {op})")
    devs = list(contig) + list(device_only)
    key, name = devs[-1]
    case("device", qual, base, lambda a: {key: a[key].cpu()},
         f"Expected tensor to have cuda DeviceType, but got tensor with cpu DeviceType (while checking arguments for {op})")
    if through:
        case("contiguity-list-is-shorter", qual, base, through[0], through[1])
    if same:
        case("same-device", qual, base, lambda a: {key: a[key].to("cuda:1")},
             f"Expected tensor for argument #0 '{devs[0][1]}' to have the same device as tensor for argument #{len(devs) - 1} '{name}'; but device 0 does not equal 1 "
             f"(while checking arguments for {op})", second_gpu=True)
    elif fall:
        case("no-same-device-check", qual, base, lambda a: {key: a[key].to("cuda:1"), **fall[0](a)}, fall[1], second_gpu=True)


def checks(qual, base, *pairs):
    for i, (change, msg) in enumerate(pairs):
        case(f"{i:02d}", qual, base, change, msg)


# ---- block-scaled GEMMs: M = N = 16, K = 128 -----------------------------------------------------------------------------------------
def _matmul(op, fp8, nn, nv, ada):
    qual = f"_qutlass_C::{op}"
    kmin, sfd, sfn = (16, E4, "float8_e4m3fn") if nv else (32, E8, "float8_e8m0fnu")
    data, other, dn = (E4, U8, "float8_e4m3fn") if fp8 else (U8, I8, "uint8")
    kb = 128 // (16 if nv else 32)
    need = 16 * kb if ada else 128 * ((kb + 3) // 4 * 4)
    layout = "row-major" if ada else "blocked"

    def base():
        kd = 128 if fp8 else 64
        return dict(A=z(128, 16, dtype=data) if nn else z(16, kd, dtype=data), B=z(16, kd, dtype=data), A_sf=z(need, dtype=sfd), B_sf=z(need, dtype=sfd),
                    alpha=torch.ones(1, device=DEV))

    four = [("A", "A"), ("B", "B"), ("A_sf", "A_sf"), ("B_sf", "B_sf")]
    if fp8:
        generic(qual, op, lambda: {**base(), "alpha": torch.ones(2, device=DEV)}, four + [("alpha", "alpha")])
    else:   # alpha is not in the contiguity list: a strided alpha reaches the dtype checks
        generic(qual, op, base, four, [("alpha", "alpha")],
                through=(lambda a: {"alpha": nc(torch.ones(2, device=DEV)), "A": a["A"].view(other)}, f"A must be {dn}"))
    small = (lambda a: {"A": z(8, 16, dtype=data), "B": z(16, 8, dtype=data)}) if nn else (lambda a: {"A": z(16, 8, dtype=data), "B": z(16, 8, dtype=data)})
    checks(qual, base,
           (lambda a: {"A": a["A"].view(other)}, f"A must be {dn}" + (" (or float8_e5m2)" if fp8 else "")),
           (lambda a: {"B": a["B"].view(other)}, f"B must be {dn}"),
           (lambda a: {"A_sf": a["A_sf"].view(U8)}, f"A_sf must be {sfn}"),
           (lambda a: {"B_sf": a["B_sf"].view(U8)}, f"B_sf must be {sfn}"),
           (lambda a: {"A": a["A"][None]}, "A and B must be 2D"),
           (lambda a: {"B": z(16, 32, dtype=data)}, "Inner dimensions must match for A.T @ B.T" if nn else "Inner dimensions must match for A @ B.T"),
           (small, f"A K-dim must be >= {kmin}"),
           (lambda a: {"alpha": a["alpha"].to(F64)}, "alpha must be a float32 tensor with at least one element"),
           (lambda a: {"alpha": a["alpha"][:0]}, "alpha must be a float32 tensor with at least one element"),
           (lambda a: {"A_sf": a["A_sf"][:4]}, f"A_sf has 4 elements, the {layout} scale layout of A needs {need}"),
           (lambda a: {"B_sf": a["B_sf"][:4]}, f"B_sf has 4 elements, the {layout} scale layout of B needs {need}"))


_matmul("matmul_mxf4_bf16_tn", False, False, False, False)
_matmul("matmul_nvf4_bf16_tn", False, False, True, False)
_matmul("matmul_ada_mxf4_bf16_tn", False, False, False, True)
_matmul("matmul_mxf8_bf16_tn", True, False, False, False)
_matmul("matmul_mxf8_bf16_nn", True, True, False, False)
# what the C ABI rejects comes back through the same check, with the library's message (K = 96: no multiple of 128)
case("c-abi-message", "_qutlass_C::matmul_mxf4_bf16_tn",
     lambda: dict(A=z(16, 48, dtype=U8), B=z(16, 48, dtype=U8), A_sf=z(512, dtype=E8), B_sf=z(512, dtype=E8), alpha=torch.ones(1, device=DEV)), lambda a: {},
     "multiple of 128")


# ---- grouped GEMMs: M = 4, E = 2, N = 8, K = 128 -------------------------------------------------------------------------------------
def _grouped(op, fp8, nv, w4a8):
    qual = f"qutlass_amd::{op}"
    sfd, sfn, kb = (E4, "float8_e4m3fn", 8) if nv else (E8, "float8_e8m0fnu", 4)
    ad, bd = (E4 if fp8 or w4a8 else U8), (E4 if fp8 else U8)

    def base():
        return dict(A=z(4, 128 if fp8 or w4a8 else 64, dtype=ad), B=z(2, 8, 128 if fp8 else 64, dtype=bd), A_sf=z(4 * kb, dtype=sfd), B_sf=z(16 * kb, dtype=sfd),
                    alpha=torch.ones(1, device=DEV), offs=torch.tensor([2, 4], dtype=I32, device=DEV))

    generic(qual, op, base, [(n, n) for n in ("A", "B", "A_sf", "B_sf", "alpha", "offs")])
    if w4a8:
        dtypes = [(lambda a: {"A": a["A"].view(E5)}, f"{op}: A must be float8_e4m3fn, float8_e5m2 tokens are not supported"),
                  (lambda a: {"A": a["A"].view(U8)}, f"{op}: A must be float8_e4m3fn"),
                  (lambda a: {"B": a["B"].view(I8)}, f"{op}: B must be uint8 or float4_e2m1fn_x2")]
        dims = "A must be 2D (M, K) and B 3D (E, N, K/2)"
    elif fp8:
        dtypes = [(lambda a: {"A": a["A"].view(U8)}, "A must be float8_e4m3fn or float8_e5m2"), (lambda a: {"B": a["B"].view(E5)}, "B must be float8_e4m3fn")]
        dims = "A must be 2D (M, K) and B 3D (E, N, K)"
    else:
        dtypes = [(lambda a: {"A": a["A"].view(I8)}, "A must be uint8 or float4_e2m1fn_x2"), (lambda a: {"B": a["B"].view(I8)}, "B must be uint8 or float4_e2m1fn_x2")]
        dims = "A must be 2D (M, K/2) and B 3D (E, N, K/2)"
    checks(qual, base, *dtypes,
           (lambda a: {"A_sf": a["A_sf"].view(U8)}, f"A_sf must be {sfn}"),
           (lambda a: {"B_sf": a["B_sf"].view(U8)}, f"B_sf must be {sfn}"),
           (lambda a: {"B": a["B"][0]}, dims),
           (lambda a: {"B": z(2, 8, 32, dtype=bd)}, "Inner dimensions must match for A @ B[g].T"),
           (lambda a: {"B": a["B"][:0]}, "the number of experts must be in [1, 1024] (got 0)"),
           (lambda a: {"offs": a["offs"].to(I64)}, "offs must be an int32 tensor of E = 2 elements"),
           (lambda a: {"offs": a["offs"][:1]}, "offs must be an int32 tensor of E = 2 elements"),
           (lambda a: {"alpha": z(3, dtype=F32)}, "alpha must be a float32 tensor of 1 or E = 2 elements"),
           (lambda a: {"alpha": a["alpha"].to(F64)}, "alpha must be a float32 tensor of 1 or E = 2 elements"),
           (lambda a: {"A_sf": a["A_sf"][:1]}, f"A_sf has 1 elements, the row-major scale layout of A needs {4 * kb}"),
           (lambda a: {"B_sf": a["B_sf"][:1]}, f"B_sf has 1 elements, the row-major scale layout of B needs {16 * kb}"))


_grouped("grouped_matmul_mxf4", False, False, False)
_grouped("grouped_matmul_nvf4", False, True, False)
_grouped("grouped_matmul_mxf8", True, False, False)
_grouped("grouped_matmul_mxf8_mxf4", False, False, True)


# ---- the rotate + quantize family ----------------------------------------------------------------------------------------------------
# operand (2, 64) bf16 (the gated ops: X (2, 128)), rotation 32 x 32; OUT / OUT_sf as the plain quantizers allocate them: (2, 32) packed or (2, 64) codes, (128, 4) scales
METHOD = "method must be 0 (quest) or 1 (abs_max)"
R32 = lambda: z(32, 32)


def _outs(nv=False, fp8=False):
    return dict(OUT=z(2, 64, dtype=E4) if fp8 else z(2, 32, dtype=U8), OUT_sf=z(128, 4, dtype=E4 if nv else E8))


def _prelude(qual, op, base, lead, gs=None, grouped=False, method=False, first=()):
    """The checks of quant_prelude for one op: lead -- the contiguity list in front of the global scale(s); first -- checks the op makes before it."""
    if grouped:   # global_scales (E,) is contiguous like everything else, and behind offs
        generic(qual, op, base, lead + [("global_scales", "global_scales")])
    elif gs:      # one element, device passes only: a strided (2,) one is met by the shape check
        generic(qual, op, base, lead, [(gs, "global_scale")], through=(lambda a: {gs: nc(z(2, dtype=F32))}, "global_scale must be a scalar"))
    else:
        generic(qual, op, base, lead)
    pairs = list(first) + [(lambda a: {"A": a["A"].to(F32)}, "A must be bf16"), (lambda a: {"R": a["R"].to(F32)}, "B must be bf16")]
    if grouped:
        pairs += [(lambda a: {"offs": a["offs"].to(I64)}, "offs must be a 1D int32 tensor"),
                  (lambda a: {"offs": a["offs"][None]}, "offs must be a 1D int32 tensor"),
                  (lambda a: {"global_scales": a["global_scales"].to(F64)}, "global_scales must be float"),
                  (lambda a: {"global_scales": a["global_scales"][:1]}, "global_scales must have one entry per entry of offs"),
                  (lambda a: {"global_scales": a["global_scales"][None]}, "global_scales must have one entry per entry of offs")]
    elif gs:
        pairs += [(lambda a: {gs: a[gs].to(F64)}, "global_scale must be float"),
                  (lambda a: {gs: z(2, dtype=F32)}, "global_scale must be a scalar"),
                  (lambda a: {gs: a[gs][None]}, "global_scale must be a scalar")]
    if method:
        pairs += [(lambda a: {"method": 2}, METHOD)]
    pairs += [(lambda a: {"R": z(32, 16)}, "Rotation matrix must be square"), (lambda a: {"R": z(1024)}, "Rotation matrix must be square")]
    checks(qual, base, *pairs)


def _plain(qual, op, nv=False, mask=False, fp8=False, method=None):
    def base():
        a = dict(A=z(2, 64), R=R32(), **_outs(nv, fp8))
        if mask:
            a["OUT_mask"] = z(2, 8, dtype=U8)
        if nv:
            a["global_scale"] = torch.ones(1, device=DEV)
        if method is not None:
            a["method"] = method
        return a

    lead = [("A", "A"), ("R", "B"), ("OUT", "OUT"), ("OUT_sf", "OUT_sf")] + ([("OUT_mask", "OUT_mask")] if mask else [])
    first = [(lambda a: {"method": 2}, METHOD)] if method is not None else []   # the twins check the method before anything else
    if fp8:
        first = [(lambda a: {"OUT": a["OUT"].view(U8)}, "OUT must be float8_e4m3fn or float8_e5m2"),
                 (lambda a: {"OUT_sf": a["OUT_sf"].view(I8)}, "OUT_sf must be float8_e8m0fnu or uint8")]
    _prelude(qual, op, base, lead, "global_scale" if nv else None, first=first)
    rots = "32" if mask else "16, 32, 64, or 128" if nv else "32, 64, or 128"
    pairs = [(lambda a: {"A": z(48)}, "A must be divisible by32"),
             (lambda a: {"R": z(64, 64) if mask else z(8, 8)}, f"Unsupported rotation size {64 if mask else 8}; expected {rots}."),
             (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"),
             (lambda a: {"OUT_sf": a["OUT_sf"].reshape(-1)[:3 if not nv else 7]}, "OUT_sf is too small")]
    if mask:
        pairs += [(lambda a: {"OUT_mask": a["OUT_mask"][:1]}, "OUT_mask is too small")]
    checks(qual + "/own", base, *pairs)


_plain("_qutlass_C::fusedQuantizeMxQuest", "fusedQuantizeMxQuest")
_plain("_qutlass_C::fusedQuantizeMxAbsMax", "fusedQuantizeMxAbsMax")
_plain("_qutlass_C::fusedQuantizeNvQuest", "fusedQuantizeNvQuest", nv=True)
_plain("_qutlass_C::fusedQuantizeNvAbsMax", "fusedQuantizeNvAbsMax", nv=True)
_plain("_qutlass_C::fusedQuantizeMxQuestWithMask", "fusedQuantizeMxQuestWithMask", mask=True)
_plain("qutlass_amd::fusedQuantizeMx_", "fusedQuantizeMxQuest", method=0)       # the twins name the reference's op of the method
_plain("qutlass_amd::fusedQuantizeNv_", "fusedQuantizeNvAbsMax", nv=True, method=1)
_plain("qutlass_amd::fusedQuantizeMxMask_", "fusedQuantizeMxQuestWithMask", mask=True)
_plain("qutlass_amd::fusedQuantizeMxf8_", "fusedQuantizeMxf8", fp8=True)


def _blocked(qual, op, nv=False, fp8=False):
    def base():
        a = dict(A=z(2, 64), R=R32(), **_outs(nv, fp8))
        a["OUT_sf"] = a["OUT_sf"].reshape(-1)
        if nv:
            a["global_scale"] = torch.ones(1, device=DEV)
        if not fp8:
            a["method"] = 1
        return a

    first = [(lambda a: {"OUT": a["OUT"].view(U8)}, "OUT must be float8_e4m3fn or float8_e5m2"),
             (lambda a: {"OUT_sf": a["OUT_sf"].view(I8)}, "OUT_sf must be float8_e8m0fnu or uint8")] if fp8 else []
    _prelude(qual, op, base, [("A", "A"), ("R", "B"), ("OUT", "OUT"), ("OUT_sf", "OUT_sf")], "global_scale" if nv else None, first=first)
    checks(qual + "/own", base,
           (lambda a: {"A": z(0, 64)}, "A must be a non-empty tensor"),
           (lambda a: {"R": z(8, 8)}, f"Unsupported rotation size 8; expected {'16, 32, 64, or 128' if nv else '32, 64, or 128'}."),
           (lambda a: {"A": z(2, 48)}, "the last dimension of A must be divisible by32"),
           (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"),
           (lambda a: {"OUT_sf": a["OUT_sf"][:511]}, "OUT_sf is too small for the blocked scale layout"))


_blocked("qutlass_amd::fusedQuantizeMxBlocked", "fusedQuantizeMxBlocked")
_blocked("qutlass_amd::fusedQuantizeNvBlocked", "fusedQuantizeNvBlocked", nv=True)
_blocked("qutlass_amd::fusedQuantizeMxf8Blocked_", "fusedQuantizeMxf8Blocked", fp8=True)

E4M3_ONLY = [(lambda a: {"OUT": a["OUT"].view(E5)}, "OUT must be float8_e4m3fn"), (lambda a: {"OUT_sf": a["OUT_sf"].view(I8)}, "OUT_sf must be float8_e8m0fnu or uint8")]


def _gated(qual, op, nv=False, grouped=False, fp8=False, blocked=None):
    """blocked None: the op has no such argument (flat scales)"""
    def base():
        a = dict(A=z(2, 128), R=R32(), **_outs(nv, fp8))
        if blocked:
            a["OUT_sf"] = a["OUT_sf"].reshape(-1)
        if grouped:
            a.update(global_scales=torch.ones(2, device=DEV), offs=torch.tensor([1, 2], dtype=I32, device=DEV))
        elif nv:
            a["global_scale"] = torch.ones(1, device=DEV)
        if not fp8:
            a["method"] = 1
        if blocked is not None:
            a["blocked"] = blocked
        return a

    qual += "/blocked" if blocked else ""
    lead = [("A", "A"), ("R", "B"), ("OUT", "OUT"), ("OUT_sf", "OUT_sf")] + ([("offs", "offs")] if grouped else [])
    _prelude(qual, op, base, lead, "global_scale" if nv and not grouped else None, grouped, method=not fp8, first=E4M3_ONLY if fp8 else [])
    checks(qual + "/own", base,
           (lambda a: {"A": z(2, 127)}, "the last dimension of A must be 2 * I"),
           (lambda a: {"A": z(2, 0)}, "the last dimension of A must be 2 * I"),
           (lambda a: {"R": z(8, 8)}, f"Unsupported rotation size 8; expected {'16, 32, 64, or 128' if nv else '32, 64, or 128'}."),
           (lambda a: {"A": z(2, 96)}, "the gate / up width must be divisible by32"),
           (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"),
           (lambda a: {"OUT_sf": a["OUT_sf"].reshape(-1)[:511 if blocked else 7 if nv else 3]},
            "OUT_sf is too small for the blocked scale layout" if blocked else "OUT_sf is too small"))


_gated("qutlass_amd::fusedSiluMulQuantizeMx_", "fusedSiluMulQuantizeMx", blocked=False)
_gated("qutlass_amd::fusedSiluMulQuantizeMx_", "fusedSiluMulQuantizeMxBlocked", blocked=True)     # the blocked form checks under its own name
_gated("qutlass_amd::fusedSiluMulQuantizeNv_", "fusedSiluMulQuantizeNv", nv=True, blocked=False)
_gated("qutlass_amd::fusedSiluMulQuantizeNv_", "fusedSiluMulQuantizeNvBlocked", nv=True, blocked=True)
_gated("qutlass_amd::fusedSiluMulQuantizeNvGrouped_", "fusedSiluMulQuantizeNvGrouped", nv=True, grouped=True)
_gated("qutlass_amd::fusedSiluMulQuantizeMxf8_", "fusedSiluMulQuantizeMxf8", fp8=True, blocked=False)
_gated("qutlass_amd::fusedSiluMulQuantizeMxf8_", "fusedSiluMulQuantizeMxf8Blocked", fp8=True, blocked=True)


def _gather(qual, op, nv=False, grouped=False, fp8=False):
    def base():   # T = 3 tokens, M = 2 rows
        a = dict(A=z(3, 64), R=R32(), src_row=z(2, dtype=I32), **_outs(nv, fp8))
        if grouped:
            a.update(global_scales=torch.ones(2, device=DEV), offs=torch.tensor([1, 2], dtype=I32, device=DEV))
        elif nv:
            a["global_scale"] = torch.ones(1, device=DEV)
        if not fp8:
            a["method"] = 1
        return a

    lead = [("A", "A"), ("R", "B"), ("src_row", "src_row"), ("OUT", "OUT"), ("OUT_sf", "OUT_sf")] + ([("offs", "offs")] if grouped else [])
    first = [(lambda a: {"OUT": a["OUT"].view(U8)}, "OUT must be float8_e4m3fn or float8_e5m2"),
             (lambda a: {"OUT_sf": a["OUT_sf"].view(I8)}, "OUT_sf must be float8_e8m0fnu or uint8")] if fp8 else []
    _prelude(qual, op, base, lead, "global_scale" if nv and not grouped else None, grouped, method=not fp8, first=first)
    checks(qual + "/own", base,
           (lambda a: {"A": z(192)}, "A must be 2D (T, K)"),
           (lambda a: {"A": z(3, 0)}, "A must be 2D (T, K)"),
           (lambda a: {"src_row": a["src_row"].to(I64)}, "src_row must be a 1D int32 tensor"),
           (lambda a: {"src_row": a["src_row"][None]}, "src_row must be a 1D int32 tensor"),
           (lambda a: {"R": z(8, 8)}, f"Unsupported rotation size 8; expected {'16, 32, 64, or 128' if nv else '32, 64, or 128'}."),
           (lambda a: {"A": z(3, 48)}, "the last dimension of A must be divisible by32"),
           (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"),
           (lambda a: {"OUT_sf": a["OUT_sf"].reshape(-1)[:7 if nv else 3]}, "OUT_sf is too small"))


_gather("qutlass_amd::fusedGatherQuantizeMx_", "fusedGatherQuantizeMx")
_gather("qutlass_amd::fusedGatherQuantizeNv_", "fusedGatherQuantizeNv", nv=True)
_gather("qutlass_amd::fusedGatherQuantizeNvGrouped_", "fusedGatherQuantizeNvGrouped", nv=True, grouped=True)
_gather("qutlass_amd::fusedGatherQuantizeMxf8_", "fusedGatherQuantizeMxf8", fp8=True)


# ---- the gated activations and the per-expert bias (gpt-oss) -------------------------------------------------------------------------
def _bias(qual, op, base, width, empty="offs without a bias"):
    """oai_bias: the checks on an optional (E, width) bias with its offs; base() has a bias of E = 2 with offs.  Its same-device checks compare with the op's first
    tensor, named 'X' whatever the op calls it.  empty: what an empty bias with offs meets.  (E = 1025: the one case that needs a tensor of more than a few KiB.)"""
    one = lambda t: {"bias": z(1, width), "offs": t}   # E = 1 needs no offs
    checks(qual + "/bias", base,
           (lambda a: {"bias": z(0)}, empty),
           (lambda a: {"bias": nc(a["bias"])}, f"Expected contiguous tensor, but got non-contiguous tensor for argument #0 'bias' (while checking arguments for {op})"),
           (lambda a: {"bias": a["bias"].cpu()}, f"Expected tensor to have cuda DeviceType, but got tensor with cpu DeviceType (while checking arguments for {op})"),
           (lambda a: {"bias": a["bias"].to(F32)}, "bias must be bf16"),
           (lambda a: {"bias": z(2, width + 8)}, f"bias must be (E, {width})"),
           (lambda a: {"bias": z(2 * width)}, f"bias must be (E, {width})"),
           (lambda a: {"bias": z(1025, width)}, "the number of experts must be in [1, 1024] (got 1025)"),
           (lambda a: {"offs": z(0, dtype=I32)}, "a bias of E = 2 experts needs offs"),
           (lambda a: {"offs": nc(a["offs"])}, f"Expected contiguous tensor, but got non-contiguous tensor for argument #0 'offs' (while checking arguments for {op})"),
           (lambda a: {"offs": a["offs"].cpu()}, f"Expected tensor to have cuda DeviceType, but got tensor with cpu DeviceType (while checking arguments for {op})"),
           (lambda a: {"offs": a["offs"].to(I64)}, "offs must be an int32 tensor of E = 2 elements"),
           (lambda a: {"offs": a["offs"][None]}, "offs must be an int32 tensor of E = 2 elements"),
           (lambda a: one(z(2, dtype=I32)), "offs must be an int32 tensor of E = 1 elements"))
    same = "Expected tensor for argument #0 'X' to have the same device as tensor for argument #1 '{}'; but device 0 does not equal 1 (while checking arguments for {})"
    case("bias-same-device", qual, base, lambda a: {"bias": a["bias"].to("cuda:1")}, same.format("bias", op), second_gpu=True)
    case("offs-same-device", qual, base, lambda a: {"offs": a["offs"].to("cuda:1")}, same.format("offs", op), second_gpu=True)


def _activation(qual, oai):
    op = qual.split("::")[1]

    def base():
        a = dict(X=z(2, 32), OUT=z(2, 16))
        if oai:
            a.update(alpha=1.702, limit=7.0, bias=z(2, 32), offs=torch.tensor([1, 2], dtype=I32, device=DEV))
        return a

    generic(qual, op, base, [("X", "X"), ("OUT", "OUT")])
    checks(qual, base,
           (lambda a: {"X": a["X"].to(F32)}, "X and OUT must be bf16"),
           (lambda a: {"OUT": a["OUT"].to(F32)}, "X and OUT must be bf16"),
           (lambda a: {"X": z(2, 31)}, "the last dimension of X must be 2 * I"),
           (lambda a: {"X": z(2, 0)}, "the last dimension of X must be 2 * I"),
           (lambda a: {"X": z(2, 24)}, "the gate / up width must be divisible by8"),
           (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"))
    if oai:
        _bias(qual, op, base, 32)


_activation("qutlass_amd::siluAndMul_", False)
_activation("qutlass_amd::swigluOaiAndMul_", True)


def _swiglu_oai_quantize(qual, op, plain, fp8):
    def base():
        a = dict(A=z(2, 128), R=R32(), **_outs(False, fp8), alpha=1.702, limit=7.0, bias=z(2, 128), offs=torch.tensor([1, 2], dtype=I32, device=DEV))
        if not fp8:
            a["method"] = 1
        return a

    _prelude(qual, op, base, [("A", "A"), ("R", "B"), ("OUT", "OUT"), ("OUT_sf", "OUT_sf")], method=not fp8, first=E4M3_ONLY if fp8 else [])
    checks(qual + "/own", base,
           (lambda a: {"A": z(2, 127)}, "the last dimension of A must be 2 * I"),
           (lambda a: {"R": z(128, 128)}, f"rotation size 128 is not supported; expected 32 or 64 (use swiglu_oai_and_mul followed by {plain})"),
           (lambda a: {"R": z(16, 16)}, "Unsupported rotation size 16; expected 32 or 64."),
           (lambda a: {"A": z(2, 96)}, "the gate / up width must be divisible by32"),
           (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"),
           (lambda a: {"OUT_sf": a["OUT_sf"].reshape(-1)[:3]}, "OUT_sf is too small"))
    _bias(qual, op, base, 128)


_swiglu_oai_quantize("qutlass_amd::fusedSwigluOaiQuantizeMx_", "fusedSwigluOaiQuantizeMx", "fusedQuantizeMx", False)
_swiglu_oai_quantize("qutlass_amd::fusedSwigluOaiQuantizeMxf8_", "fusedSwigluOaiQuantizeMxf8", "fusedQuantizeMxf8", True)


# ---- MoE combine and routing ---------------------------------------------------------------------------------------------------------
def _combine(qual, bias):
    op = qual.split("::")[1]

    def base():   # M = 4 rows of H = 8, T = 2 tokens, topk = 2
        a = dict(Y=z(4, 8), pos=z(2, 2, dtype=I32), weights=z(2, 2, dtype=F32))
        if bias:
            a.update(bias=z(2, 8), offs=torch.tensor([2, 4], dtype=I32, device=DEV))
        a["OUT"] = z(2, 8)
        return a

    generic(qual, op, base, [("Y", "Y"), ("pos", "pos"), ("weights", "weights"), ("OUT", "OUT")])
    checks(qual, base,
           (lambda a: {"Y": a["Y"].to(F32)}, "Y and OUT must be bf16"),
           (lambda a: {"OUT": a["OUT"].to(F32)}, "Y and OUT must be bf16"),
           (lambda a: {"pos": a["pos"].to(I64)}, "pos must be int32"),
           (lambda a: {"weights": a["weights"].to(BF)}, "weights must be float32"),
           (lambda a: {"Y": z(32)}, "Y must be 2D (M, H)"),
           (lambda a: {"Y": z(4, 0)}, "Y must be 2D (M, H)"),
           (lambda a: {"pos": z(4, dtype=I32)}, "pos and weights must both be (T, topk)"),
           (lambda a: {"weights": z(2, 3, dtype=F32)}, "pos and weights must both be (T, topk)"),
           (lambda a: {"Y": z(4, 12)}, "the row length of Y must be divisible by8"),
           (lambda a: {"pos": z(2, 33, dtype=I32), "weights": z(2, 33, dtype=F32)}, "topk must be in [1, 32] (got 33)"),
           (lambda a: {"pos": z(2, 0, dtype=I32), "weights": z(2, 0, dtype=F32)}, "topk must be in [1, 32] (got 0)"),
           (lambda a: {"OUT": a["OUT"][:1]}, "OUT is too small"))
    if bias:
        checks(qual + "/empty", base, (lambda a: {"bias": z(0), "offs": z(0, dtype=I32)}, "bias must be (E, 8)"))
        _bias(qual, op, base, 8, empty="bias must be (E, 8)")   # the op's own check of an empty bias comes first


_combine("qutlass_amd::moeCombine_", False)
_combine("qutlass_amd::moeCombineBias_", True)


def _topk(qual, grouped):
    op = qual.split("::")[1]

    def base():   # T = 2 tokens, E = 8 experts, topk = 2
        a = dict(logits=z(2, 8))
        if grouped:
            a["bias"] = z(8, dtype=F32)
        a.update(weights=z(2, 2, dtype=F32), ids=z(2, 2, dtype=I32))
        if grouped:
            a.update(scores=z(2, 8, dtype=F32), n_group=1, topk_group=1, scoring=0, renormalize=True, routed_scaling_factor=1.0)
        else:
            a["renormalize"] = True
        return a

    names = ["logits"] + (["bias"] if grouped else []) + ["weights", "ids"] + (["scores"] if grouped else [])
    generic(qual, op, base, [(n, n) for n in names])
    checks(qual, base,
           (lambda a: {"logits": a["logits"].to(torch.float16)}, "logits must be bf16 or float32"),
           (lambda a: {"weights": a["weights"].to(BF)}, "weights must be float32"),
           (lambda a: {"ids": a["ids"].to(I64)}, "ids must be int32"),
           (lambda a: {"logits": z(16)}, "logits must be 2D (T, E)"),
           (lambda a: {"weights": z(4, dtype=F32)}, "weights and ids must both be (T, topk)"),
           (lambda a: {"ids": z(3, 2, dtype=I32)}, "weights and ids must both be (T, topk)"),
           (lambda a: {"ids": z(2, 3, dtype=I32)}, "weights and ids must both be (T, topk)"))
    if grouped:
        checks(qual + "/own", base,
               (lambda a: {"bias": a["bias"].to(BF)}, "bias must be a float32 tensor of (E,)"),
               (lambda a: {"bias": z(7, dtype=F32)}, "bias must be a float32 tensor of (E,)"),
               (lambda a: {"bias": z(1, 8, dtype=F32)}, "bias must be a float32 tensor of (E,)"),
               (lambda a: {"scores": a["scores"].to(BF)}, "scores must be a float32 tensor of (T, E)"),
               (lambda a: {"scores": z(16, dtype=F32)}, "scores must be a float32 tensor of (T, E)"),
               (lambda a: {"scores": z(2, 7, dtype=F32)}, "scores must be a float32 tensor of (T, E)"))


_topk("qutlass_amd::moeTopkSoftmax_", False)
_topk("qutlass_amd::moeTopkGrouped_", True)


def _sort():
    qual, op = "qutlass_amd::moeSort_", "moeSort_"

    def base():   # T = 2, topk = 2, 4 experts, a map of 4 entries; the workspace may be empty below the one-launch bound, here it has two elements
        return dict(topk_ids=z(2, 2, dtype=I32), expert_map=z(4, dtype=I32), num_experts=4, src_row=z(4, dtype=I32), offs=z(4, dtype=I32), pos=z(2, 2, dtype=I32),
                    workspace=z(2, dtype=I32))

    generic(qual, op, base, [(n, n) for n in ("topk_ids", "src_row", "offs", "pos", "workspace")])
    same = "Expected tensor for argument #0 'topk_ids' to have the same device as tensor for argument #1 'expert_map'; but device 0 does not equal 1"
    checks(qual, base,
           (lambda a: {"topk_ids": a["topk_ids"].to(torch.int16)}, "topk_ids must be int32 or int64"),
           (lambda a: {"topk_ids": z(4, dtype=I32)}, "topk_ids must be 2D (T, topk)"),
           (lambda a: {"src_row": a["src_row"].to(I64)}, "src_row, offs and pos must be int32"),
           (lambda a: {"offs": a["offs"].to(I64)}, "src_row, offs and pos must be int32"),
           (lambda a: {"pos": a["pos"].to(I64)}, "src_row, offs and pos must be int32"),
           (lambda a: {"src_row": a["src_row"][:3]}, "src_row, offs or pos is too small"),
           (lambda a: {"offs": a["offs"][:3]}, "src_row, offs or pos is too small"),
           (lambda a: {"pos": a["pos"][:1]}, "src_row, offs or pos is too small"),
           (lambda a: {"expert_map": nc(a["expert_map"])},
            f"Expected contiguous tensor, but got non-contiguous tensor for argument #0 'expert_map' (while checking arguments for {op})"),
           (lambda a: {"expert_map": a["expert_map"].cpu()}, f"Expected tensor to have cuda DeviceType, but got tensor with cpu DeviceType (while checking arguments for {op})"),
           (lambda a: {"expert_map": a["expert_map"].to(I64)}, "expert_map must be a 1D int32 tensor"),
           (lambda a: {"expert_map": a["expert_map"][None]}, "expert_map must be a 1D int32 tensor"))
    case("map-same-device", qual, base, lambda a: {"expert_map": a["expert_map"].to("cuda:1")}, f"{same} (while checking arguments for {op})", second_gpu=True)


_sort()


# ---- rotate + quantize + GEMM in one launch: X (2, 128), N = 8 ------------------------------------------------------------------------
def _fused_matmul():
    qual, op = "qutlass_amd::fusedQuantizeMatmulMxf4", "fusedQuantizeMatmulMxf4"

    def base():
        return dict(X=z(2, 128), R=R32(), B=z(8, 64, dtype=U8), B_sf=z(512, dtype=E8), alpha=torch.ones(1, device=DEV), method=1)

    generic(qual, op, base, [("X", "X"), ("R", "R"), ("B", "B"), ("B_sf", "B_sf")], [("alpha", "alpha")],
            through=(lambda a: {"alpha": nc(torch.ones(2, device=DEV)), "B": a["B"].view(I8)}, "B must be uint8"))
    checks(qual, base,
           (lambda a: {"X": a["X"].to(F32)}, "X and R must be bf16"),
           (lambda a: {"R": a["R"].to(F32)}, "X and R must be bf16"),
           (lambda a: {"B": a["B"].view(I8)}, "B must be uint8"),
           (lambda a: {"B_sf": a["B_sf"].view(U8)}, "B_sf must be float8_e8m0fnu"),
           (lambda a: {"alpha": a["alpha"].to(F64)}, "alpha must be a float32 tensor with at least one element"),
           (lambda a: {"alpha": a["alpha"][:0]}, "alpha must be a float32 tensor with at least one element"),
           (lambda a: {"X": z()}, "X must be at least 1-D and B 2-D"),
           (lambda a: {"B": a["B"][None]}, "X must be at least 1-D and B 2-D"),
           (lambda a: {"R": z(32, 16)}, "Rotation matrix must be square"),
           (lambda a: {"B": z(8, 32, dtype=U8)}, "Inner dimensions must match for Q(X) @ B.T"),
           (lambda a: {"B_sf": a["B_sf"][:511]}, "B_sf is too small for the blocked scale layout of B"))


_fused_matmul()


# ---- QAT-backward data preparation: the reference's ops and their twins are one function each -----------------------------------------
SMALL = "output tensors are too small"


def _backward(names):
    def backward_t():   # x (64, 32): N = 64, M = 32
        return dict(x=z(64, 32), h=z(32, 32), xh_e2m1=z(32, 32, dtype=U8), xh_e8m0=z(32, 2, dtype=E8))

    def backward_qt():
        return dict(x_e2m1=z(64, 16, dtype=U8), x_e8m0=z(64, 1, dtype=E8), h=z(32, 32), alpha=torch.ones(1, device=DEV), xh_e2m1=z(32, 32, dtype=U8),
                    xh_e8m0=z(32, 2, dtype=E8))

    def square_double():   # m = 2 rows, padded to 128
        return dict(x_bf16=z(2, 32), x_fp8=z(128, 32, dtype=E4), row_scales=z(128, 1, dtype=E8), column_scales=z(32, 4, dtype=E8))

    def transpose():       # m = 2 rows of n = 32
        return dict(x_fp4=z(2, 16, dtype=U8), scales=z(2, 1, dtype=E8), x_fp8=z(32, 128, dtype=E4), shared_exps=z(32, 4, dtype=E8))

    qual = names[0]
    generic(qual, "backward_t_bf16", backward_t, [(n, n) for n in ("x", "h", "xh_e2m1", "xh_e8m0")], same=False, fall=(lambda a: {"xh_e2m1": a["xh_e2m1"][:1]}, SMALL))
    checks(qual, backward_t,
           (lambda a: {"x": a["x"].to(F32)}, "x and h must be bf16"),
           (lambda a: {"h": a["h"].to(F32)}, "x and h must be bf16"),
           (lambda a: {"x": z(2048)}, "x must be at least 2-D and h 32 x 32"),
           (lambda a: {"h": z(32, 16)}, "x must be at least 2-D and h 32 x 32"),
           (lambda a: {"xh_e2m1": a["xh_e2m1"][:1]}, SMALL),
           (lambda a: {"xh_e8m0": a["xh_e8m0"][:1]}, SMALL))
    qual = names[1]   # its device list has alpha in the middle (x_e2m1, x_e8m0, h, alpha, xh_e2m1, xh_e8m0), its contiguity list has no alpha
    case("contiguity-list-is-shorter", qual, backward_qt, lambda a: {"alpha": nc(torch.ones(2, device=DEV)), "xh_e2m1": a["xh_e2m1"][:1]}, SMALL)
    case("no-same-device-check", qual, backward_qt, lambda a: {"xh_e8m0": a["xh_e8m0"].to("cuda:1"), "xh_e2m1": a["xh_e2m1"][:1]}, SMALL, second_gpu=True)
    checks(qual, backward_qt,
           (lambda a: {"xh_e8m0": nc(a["xh_e8m0"])},
            "Expected contiguous tensor, but got non-contiguous tensor for argument #4 'xh_e8m0' (while checking arguments for backward_qt_bf16)"),
           (lambda a: {"alpha": a["alpha"].cpu()}, "Expected tensor to have cuda DeviceType, but got tensor with cpu DeviceType (while checking arguments for backward_qt_bf16)"),
           (lambda a: {"h": a["h"].to(F32)}, "h must be bf16 and alpha float"),
           (lambda a: {"alpha": a["alpha"].to(F64)}, "h must be bf16 and alpha float"),
           (lambda a: {"x_e2m1": z(1024, dtype=U8)}, "x_e2m1 / x_e8m0 must be 1-byte tensors of at least 2 dimensions and h 32 x 32"),
           (lambda a: {"x_e2m1": z(64, 8, dtype=torch.int16)}, "x_e2m1 / x_e8m0 must be 1-byte tensors of at least 2 dimensions and h 32 x 32"),
           (lambda a: {"x_e8m0": z(64, 1, dtype=torch.int16)}, "x_e2m1 / x_e8m0 must be 1-byte tensors of at least 2 dimensions and h 32 x 32"),
           (lambda a: {"h": z(32, 16)}, "x_e2m1 / x_e8m0 must be 1-byte tensors of at least 2 dimensions and h 32 x 32"),
           (lambda a: {"x_e8m0": z(63, 1, dtype=E8)}, "x_e8m0 must hold one scale per 32 elements of x_e2m1"),
           (lambda a: {"xh_e2m1": a["xh_e2m1"][:1]}, SMALL),
           (lambda a: {"xh_e8m0": a["xh_e8m0"][:1]}, SMALL))
    qual = names[2]
    generic(qual, "backward_bf16_square_double_mxfp8", square_double, [(n, n) for n in ("x_bf16", "x_fp8", "row_scales", "column_scales")], same=False,
            fall=(lambda a: {"row_scales": a["row_scales"][:1]}, SMALL))
    checks(qual, square_double,
           (lambda a: {"x_bf16": a["x_bf16"].to(F32)}, "x_bf16 must be a 2-D bf16 tensor"),
           (lambda a: {"x_bf16": z(64)}, "x_bf16 must be a 2-D bf16 tensor"),
           (lambda a: {"x_fp8": z(4096, dtype=E4)}, "x_fp8 must be (m_pad, n)"),
           (lambda a: {"x_fp8": z(128, 64, dtype=E4)}, "x_fp8 must be (m_pad, n)"),
           (lambda a: {"x_fp8": z(1, 32, dtype=E4)}, "x_fp8 must have a multiple of 128 rows, at least as many as x_bf16"),
           (lambda a: {"x_fp8": z(64, 32, dtype=E4)}, "x_fp8 must have a multiple of 128 rows, at least as many as x_bf16"),
           (lambda a: {"row_scales": a["row_scales"][:1]}, SMALL),
           (lambda a: {"column_scales": a["column_scales"][:1]}, SMALL))
    qual = names[3]
    generic(qual, "mxfp4_transpose_mxfp8", transpose, [(n, n) for n in ("x_fp4", "scales", "x_fp8", "shared_exps")], same=False,
            fall=(lambda a: {"shared_exps": a["shared_exps"][:1]}, SMALL))
    checks(qual, transpose,
           (lambda a: {"x_fp4": z(32, dtype=U8)}, "x_fp4 must be a 2-D 1-byte tensor, scales 1-byte"),
           (lambda a: {"x_fp4": z(2, 16, dtype=torch.int16)}, "x_fp4 must be a 2-D 1-byte tensor, scales 1-byte"),
           (lambda a: {"scales": z(2, 1, dtype=torch.int16)}, "x_fp4 must be a 2-D 1-byte tensor, scales 1-byte"),
           (lambda a: {"x_fp8": z(4096, dtype=E4)}, "x_fp8 must be (n, m_pad)"),
           (lambda a: {"x_fp8": z(16, 128, dtype=E4)}, "x_fp8 must be (n, m_pad)"),
           (lambda a: {"x_fp8": z(32, 1, dtype=E4)}, "x_fp8 must have a multiple of 128 columns, at least as many as x_fp4 has rows"),
           (lambda a: {"x_fp8": z(32, 64, dtype=E4)}, "x_fp8 must have a multiple of 128 columns, at least as many as x_fp4 has rows"),
           (lambda a: {"scales": z(1, 1, dtype=E8)}, "scales must hold one e8m0 per 32 elements"),
           (lambda a: {"shared_exps": a["shared_exps"][:1]}, SMALL))


_BACKWARD = ("backward_t_bf16", "backward_qt_bf16", "backward_bf16_square_double_mxfp8", "mxfp4_transpose_mxfp8")
_backward([f"_qutlass_C::{n}" for n in _BACKWARD])
_backward([f"qutlass_amd::{n}_" for n in _BACKWARD])

# ---- the block-scale swizzle ---------------------------------------------------------------------------------------------------------
checks("qutlass_amd::to_blocked", lambda: dict(input_matrix=z(2, 4, dtype=U8)),
       (lambda a: {"input_matrix": z(8, dtype=U8)}, "to_blocked expects a 2-D matrix"),
       (lambda a: {"input_matrix": z(2, 4)}, "Expected element size to be 1 byte (8 bits)"),
       (lambda a: {"input_matrix": nc(a["input_matrix"])}, "Input tensor must be contiguous"))


def test_every_op_of_the_extension_has_cases():
    """both namespaces: every op with a CUDA kernel is one the extension registered (the functional ops of ops.py are Python, registered for no device)"""
    import qutlass_amd  # noqa: F401  (loads the extension)

    covered = {c[1].split("/")[0] for c in CASES}
    ops = {n.split(".")[0] for n in torch._C._dispatch_get_registrations_for_dispatch_key("CUDA") if n.startswith(("_qutlass_C::", "qutlass_amd::"))}
    assert len(ops) >= 48 and ops <= covered, sorted(ops - covered)


@pytest.mark.parametrize("qual,base,change,msg,second_gpu", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_rejected_with_its_message(qual, base, change, msg, second_gpu):
    if second_gpu and torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    import qutlass_amd  # noqa: F401  (registers the ops)

    ns, name = qual.split("/")[0].split("::")
    args = base()
    args.update(change(args))
    with pytest.raises(RuntimeError, match=re.escape(msg)) as e:
        getattr(getattr(torch.ops, ns), name)(*args.values())
    assert "torch_ext.cpp" in str(e.value)
