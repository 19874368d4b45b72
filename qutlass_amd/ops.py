"""Operator registration: ``torch.ops._qutlass_C.*`` (the ops of the reference's binding file ``qutlass/csrc/bindings.cpp``)
and ``torch.ops.qutlass_amd.to_blocked``.

The ops live in the in-tree C++ extension ``qutlass/_CUDA.abi3.so`` (``csrc/torch_ext.cpp``, LibTorch stable ABI, no device
code) -- the same module name the reference's op library has (bindings.cpp:537-540): argument validation with the
reference's order and messages, output allocation, current-stream lookup, then ONE call into the C ABI of
``libqutlass_amd.so`` (``include/qutlass_amd.h``), where the hand-written HIP kernels are.  No Python-side compute and no
fallback: if the extension is not built, loading it raises.
"""
from __future__ import annotations

import math
import os
from typing import Callable, NamedTuple

import torch

from . import _lib
from .utils import padded_scale_shape

_HERE = os.path.dirname(os.path.abspath(__file__))
# QUTLASS_AMD_OP_LIBRARY: another build of the op library, e.g. the trimmed one (qutlass_amd.build.build_extension(minimal=True), the reference's QUTLASS_MINIMAL_BUILD)
EXT_PATH = os.environ.get("QUTLASS_AMD_OP_LIBRARY") or os.path.join(os.path.dirname(_HERE), "qutlass", "_CUDA.abi3.so")

_registered = False
_AMD = torch.ops.qutlass_amd   # (the namespace object: the runners below look the in-place twins up on it once per call)


def register_torch_ops() -> None:
    """Load the C++ extension, which registers ``_qutlass_C::*`` and ``qutlass_amd::to_blocked`` with the dispatcher
    (reference: bindings.cpp:498-535 + registration.h).  The file is the Python extension module ``qutlass._CUDA``; it is
    loaded by path here so that ``import qutlass_amd`` does not depend on the alias package, and ``import qutlass._CUDA``
    afterwards finds the same, already initialised library."""
    global _registered
    if _registered:
        return
    _lib.load()  # libqutlass_amd.so first (the extension links against it)
    if not os.path.exists(EXT_PATH):
        raise ImportError(
            f"{EXT_PATH} is missing: build the extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or python qutlass_amd/build.py). "
            "qutlass_amd has no CPU / eager fallback."
        )
    torch.ops.load_library(EXT_PATH)
    _register_fakes()
    _define_functional_ops()
    _registered = True   # only once the fake kernels are in place: a failed registration is retried (and raises again) on the next call


def _register_fakes() -> None:
    """Shape-only ("fake" / meta) kernels for every op of the extension, so that callers can be traced: `torch.compile(fullgraph=True)`, `make_fx`,
    `torch.export` under FakeTensorMode.  The reference's default `to_blocked` is plain torch written to be compiled through
    (qutlass/utils.py:160-193); here it is a custom op, and without a fake kernel a compiled caller graph-breaks or fails.  The 14 `_qutlass_C` ops get
    one where the schema tells the truth (the five GEMMs: they allocate (M, N) bf16); the ops that fill caller tensors are traced through their
    mutation-declaring twins in the `qutlass_amd` namespace (csrc/torch_ext.cpp), which return nothing."""
    def rf(qualname):   # (a trimmed op library -- QUTLASS_MINIMAL_BUILD -- does not define the training-only ops: nothing to register for them)
        ns, op = qualname.split("::")
        if hasattr(getattr(torch.ops, ns), op):
            return torch.library.register_fake(qualname)
        return lambda fn: fn

    def gemm_tn(A, B, A_sf, B_sf, alpha):
        return A.new_empty((A.size(0), B.size(0)), dtype=torch.bfloat16)

    for name in ("matmul_mxf4_bf16_tn", "matmul_nvf4_bf16_tn", "matmul_ada_mxf4_bf16_tn", "matmul_mxf8_bf16_tn"):
        rf(f"_qutlass_C::{name}")(gemm_tn)

    @rf("_qutlass_C::matmul_mxf8_bf16_nn")
    def _(A, B, A_sf, B_sf, alpha):   # A is (K, M) (bindings.cpp:185-214)
        return A.new_empty((A.size(1), B.size(0)), dtype=torch.bfloat16)

    # The reference's output-filling ops -- the five quantizers and the four QAT-backward data-prep ops of `_qutlass_C` -- get NO fake kernel: their
    # schemas (bindings.cpp:504-513, kept verbatim) declare neither the writes nor the aliasing returns, so a traced graph would treat the call as
    # dead code (AOTAutograd drops a `-> ()` op without declared mutation; inductor reuses OUT's storage while the returned alias is live).  Tracing
    # them fails loudly instead; the Python wrappers call the `qutlass_amd::*_` twins below, whose schemas declare `Tensor(a!)` and return nothing.
    def fills(*args):
        return None

    for row in (*QUANT_OPS.values(), *OUTPUT_OPS.values()):   # every in-place op is the twin of one row: none is called directly
        rf(f"qutlass_amd::{row.twin}")(fills)
    for row in QUANT_OPS_MXF6.values():   # (their twins live in a namespace of their own: csrc/torch_ext.cpp)
        rf(f"qutlass_amd_mxf6::{row.twin}")(fills)

    @rf("qutlass_amd::to_blocked")
    def _(input_matrix):
        rows, cols = input_matrix.shape
        return input_matrix.new_empty(((rows + 127) // 128 * 128) * ((cols + 3) // 4 * 4))

    @rf("qutlass_amd::fusedQuantizeMatmulMxf4")
    def _(X, R, B, B_sf, alpha, method):
        k = X.size(-1)
        return X.new_empty((X.numel() // k if k else 0, B.size(0)), dtype=torch.bfloat16)

    def grouped_tn(A, B, A_sf, B_sf, alpha, offs):   # A (M, K/2, 3K/4 or K), B (E, N, K/2 or K)
        return A.new_empty((A.size(0), B.size(1)), dtype=torch.bfloat16)

    for name in ("grouped_matmul_mxf4", "grouped_matmul_mxf8", "grouped_matmul_nvf4", "grouped_matmul_mxf8_mxf4", "grouped_matmul_mxf6_mxf4"):
        rf(f"qutlass_amd::{name}")(grouped_tn)

    @rf("qutlass_amd::grouped_matmul_bf16_mxf4_bf16_tn")
    def _(A, B, B_sf, alpha, offs, src_row):   # A (M, K) bf16, or with src_row (M,) the unsorted (T, K) tokens; B (E, N, K/2)
        return A.new_empty(((A if src_row is None else src_row).size(0), B.size(1)), dtype=torch.bfloat16)

    def routed(logits, topk, num_experts):   # the one-launch routing ops allocate their five results, like the grouped GEMMs: weights, ids, src_row, offs, pos
        T, i32 = logits.size(0), torch.int32
        return (logits.new_empty((T, topk), dtype=torch.float32), logits.new_empty((T, topk), dtype=i32), logits.new_empty((T * topk,), dtype=i32),
                logits.new_empty((num_experts,), dtype=i32), logits.new_empty((T, topk), dtype=i32))

    @rf("qutlass_amd::moe_route_fused")
    def _(logits, expert_map, topk, num_experts, renormalize):
        return routed(logits, topk, num_experts)

    @rf("qutlass_amd::moe_route_grouped_fused")
    def _(logits, bias, expert_map, topk, num_experts, n_group, topk_group, scoring, renormalize, routed_scaling_factor):
        return routed(logits, topk, num_experts)


def _define_functional_ops() -> None:
    """FUNCTIONAL forms of the output-filling ops (`qutlass_amd::quantize_mx` ...: allocate, call the in-place twin, return fresh tensors), defined in Python with
    `torch.library.custom_op`.  The wrappers of qutlass_amd/__init__.py call them only while a graph is being compiled (`torch.compiler.is_compiling()`): inductor (torch
    2.10) refuses every node that touches a `float8_e8m0fnu` tensor except views / cat / clone / `_scaled_mm` (torch/_inductor/lowering.py `unsupported_input_tensor`), so
    the `auto_functionalized` wrapper of a mutating op with an e8m0 argument is never decomposed and compilation dies ("auto_functionalized_v2 was not removed") -- while a
    functional op with e8m0 results is simply called as an extern kernel.  Eager callers keep the direct C++ path (a Python custom op costs ~10 us per call)."""
    if hasattr(torch.ops.qutlass_amd, "quantize_mx"):
        return
    from torch.library import custom_op

    for table, run, alloc in ((QUANT_OPS, run_quant, alloc_quant), (QUANT_OPS_MXF6, run_quant, alloc_quant), (OUTPUT_OPS, run_output, lambda row, *args: row.alloc(*args))):
        for name, row in table.items():
            if not hasattr(torch.ops.qutlass_amd_mxf6 if table is QUANT_OPS_MXF6 else torch.ops.qutlass_amd, row.twin):   # QUTLASS_MINIMAL_BUILD: inference ops only
                continue
            op = custom_op(f"qutlass_amd::{name}", mutates_args=(), schema=row.schema)(lambda *args, _row=row, _run=run: _run(_row, *args))
            op.register_fake(lambda *args, _row=row, _alloc=alloc: _alloc(_row, *args))   # the fake IS the row's allocator


# ---- the rotate + quantize family: the functional ops `qutlass_amd::<name>`, their fake kernels and the eager wrappers of __init__.py come from this table ----------
# schema:  of the functional op -- the leading tensors, [global_scale | global_scales, offs,] method[, blocked]
# twin:    the in-place op of csrc/torch_ext.cpp: the same arguments with OUT, OUT_sf inserted after the `lead` leading tensors
# operand: the shape of the tensor that is rotated and quantized, from the leading tensors -- the results are the plain quantizers' for a tensor of that shape
# fmt:     a key of QUANT_FORMATS;  blocked: scales flat in the to_blocked() layout -- fixed by the op, or None where it is the op's last argument
# The "mxf8" ops have no method: the argument behind the leading tensors is the code dtype (float8_e4m3fn / float8_e5m2).  It decides what is allocated and is not
# passed on to the twin, which reads the format off OUT's dtype.
# dtype:    ("mxf8") the code dtype where the op fixes it and has no such argument -- like blocked: fixed by the op, or None where it is an argument
# optional: (argument index, dtype or None for A's) of the `Tensor?` arguments; the twin takes an empty tensor for None
class QuantOp(NamedTuple):
    schema: str
    twin: str
    lead: int
    operand: Callable
    fmt: str
    blocked: bool | None
    dtype: torch.dtype | None = None
    optional: tuple = ()


def _same(A, R=None):
    return tuple(A.shape)


def _act(X, R=None):   # gated MLP: X is (.., 2 I) [gate | up], the operand (.., I)
    return (*X.shape[:-1], X.size(-1) // 2)


def _gathered(A, R, src_row):   # MoE dispatch: the operand is A[src_row], (M, K) for M indices
    return (src_row.size(0), A.size(-1))


_OAI_OPTIONAL = ((4, None), (5, torch.int32))   # bias in A's dtype, offs
QUANT_FORMATS = {"mx": (32, torch.float8_e8m0fnu), "nv": (16, torch.float8_e4m3fn), "mxf8": (32, torch.float8_e8m0fnu),
                 "mxf6": (32, torch.float8_e8m0fnu)}   # elements per scale, scale dtype
MXF8_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)   # code dtypes of the "mxf8" ops; "mx" and "nv" pack two e2m1 codes per uint8
QUANT_OPS = {
    "quantize_mx": QuantOp("(Tensor A, Tensor R, int method) -> (Tensor, Tensor)", "fusedQuantizeMx_", 2, _same, "mx", False),
    "quantize_nv": QuantOp("(Tensor A, Tensor R, Tensor global_scale, int method) -> (Tensor, Tensor)", "fusedQuantizeNv_", 2, _same, "nv", False),
    "quantize_mx_blocked": QuantOp("(Tensor A, Tensor R, int method) -> (Tensor, Tensor)", "fusedQuantizeMxBlocked", 2, _same, "mx", True),
    "quantize_nv_blocked": QuantOp("(Tensor A, Tensor R, Tensor global_scale, int method) -> (Tensor, Tensor)", "fusedQuantizeNvBlocked", 2, _same, "nv", True),
    "silu_mul_quantize_mx": QuantOp("(Tensor A, Tensor R, int method, bool blocked) -> (Tensor, Tensor)", "fusedSiluMulQuantizeMx_", 2, _act, "mx", None),
    "silu_mul_quantize_nv": QuantOp("(Tensor A, Tensor R, Tensor global_scale, int method, bool blocked) -> (Tensor, Tensor)", "fusedSiluMulQuantizeNv_", 2, _act, "nv", None),
    # gpt-oss: the clamped SwiGLU in place of silu * up, with the gate/up bias of the row's expert (None: no bias; offs None: one expert); flat scales
    "swiglu_oai_quantize_mx": QuantOp("(Tensor A, Tensor R, float alpha, float limit, Tensor? bias, Tensor? offs, int method) -> (Tensor, Tensor)",
                                      "fusedSwigluOaiQuantizeMx_", 2, _act, "mx", False, None, _OAI_OPTIONAL),
    "gather_quantize_mx": QuantOp("(Tensor A, Tensor R, Tensor src_row, int method) -> (Tensor, Tensor)", "fusedGatherQuantizeMx_", 3, _gathered, "mx", False),
    "gather_quantize_nv": QuantOp("(Tensor A, Tensor R, Tensor src_row, Tensor global_scale, int method) -> (Tensor, Tensor)", "fusedGatherQuantizeNv_", 3, _gathered, "nv", False),
    # one global scale per expert: global_scales (E,) with the grouped GEMMs' offs (E,)
    "gather_quantize_nv_grouped": QuantOp("(Tensor A, Tensor R, Tensor src_row, Tensor global_scales, Tensor offs, int method) -> (Tensor, Tensor)",
                                          "fusedGatherQuantizeNvGrouped_", 3, _gathered, "nv", False),
    "silu_mul_quantize_nv_grouped": QuantOp("(Tensor A, Tensor R, Tensor global_scales, Tensor offs, int method) -> (Tensor, Tensor)", "fusedSiluMulQuantizeNvGrouped_", 2,
                                            _act, "nv", False),
    # MXFP8: e4m3 / e5m2 codes, one e8m0 scale per 32 elements, abs-max (the gated op: e4m3 only)
    "quantize_mxf8": QuantOp("(Tensor A, Tensor R, ScalarType dtype) -> (Tensor, Tensor)", "fusedQuantizeMxf8_", 2, _same, "mxf8", False),
    "quantize_mxf8_blocked": QuantOp("(Tensor A, Tensor R, ScalarType dtype) -> (Tensor, Tensor)", "fusedQuantizeMxf8Blocked_", 2, _same, "mxf8", True),
    "silu_mul_quantize_mxf8": QuantOp("(Tensor A, Tensor R, ScalarType dtype, bool blocked) -> (Tensor, Tensor)", "fusedSiluMulQuantizeMxf8_", 2, _act, "mxf8", None),
    "gather_quantize_mxf8": QuantOp("(Tensor A, Tensor R, Tensor src_row, ScalarType dtype) -> (Tensor, Tensor)", "fusedGatherQuantizeMxf8_", 3, _gathered, "mxf8", False),
    # the clamped SwiGLU into e4m3 -- the A operand of the W4A8 grouped GEMM: e4m3 only (a forward activation; no dtype argument), abs-max only (no method), R = 32 / 64
    "swiglu_oai_quantize_mxf8": QuantOp("(Tensor A, Tensor R, float alpha, float limit, Tensor? bias, Tensor? offs) -> (Tensor, Tensor)", "fusedSwigluOaiQuantizeMxf8_", 2,
                                        _act, "mxf8", False, torch.float8_e4m3fn, _OAI_OPTIONAL),
}
# MXFP6: e2m3 codes, four in three bytes of a uint8 tensor (torch has no fp6 dtype), one e8m0 scale per 32 elements, abs-max, flat scales.  Rows of the same kind in
# a table of their own: the family's table above is enumerated, row for row, by the tests of the 4- and 8-bit ops.
QUANT_OPS_MXF6 = {
    "quantize_mxf6": QuantOp("(Tensor A, Tensor R) -> (Tensor, Tensor)", "fusedQuantizeMxf6_", 2, _same, "mxf6", False),
    "gather_quantize_mxf6": QuantOp("(Tensor A, Tensor R, Tensor src_row) -> (Tensor, Tensor)", "fusedGatherQuantizeMxf6_", 3, _gathered, "mxf6", False),
}


def mxf8_dtype(dtype) -> torch.dtype:
    if dtype not in MXF8_DTYPES:
        raise ValueError(f"invalid dtype {dtype!r}, must be torch.float8_e4m3fn or torch.float8_e5m2")
    return dtype


def alloc_quant(row: QuantOp, *args):
    """The results of one family op, uninitialised: packed e2m1 (.., K / 2) uint8 -- "mxf8": (.., K) codes in the dtype asked for; "mxf6": packed e2m3
    (.., 3 K / 4) uint8 -- and the scales -- (padded_rows,
    padded_cols), or their product flat when blocked -- of the operand (.., K); args as the functional op takes them.  The one allocator of the fake kernels, the
    functional ops and the eager wrappers."""
    shape = row.operand(*args[:row.lead])
    group, sf_dtype = QUANT_FORMATS[row.fmt]
    pr, pc = padded_scale_shape(math.prod(shape) // shape[-1], shape[-1], group)
    blocked = args[-1] if row.blocked is None else row.blocked
    if row.fmt == "mxf8":
        codes = args[0].new_empty(shape, dtype=row.dtype or mxf8_dtype(args[row.lead]))
    else:
        codes = args[0].new_empty((*shape[:-1], shape[-1] * 3 // 4 if row.fmt == "mxf6" else shape[-1] // 2), dtype=torch.uint8)
    return codes, args[0].new_empty((pr * pc,) if blocked else (pr, pc), dtype=sf_dtype)


def _optional(x: torch.Tensor, t: torch.Tensor | None, dtype: torch.dtype) -> torch.Tensor:
    """The in-place ops' "no tensor": an empty one."""
    return x.new_empty((0,), dtype=dtype) if t is None else t


def _no_none(args, optional):
    """args with the `Tensor?` ones of a row -- (index, dtype) pairs, dtype None: the first argument's -- as the in-place twin takes them"""
    args = list(args)
    for i, dtype in optional:
        args[i] = _optional(args[0], args[i], dtype or args[0].dtype)
    return args


def run_quant(row: QuantOp, *args):
    """Allocate, then the in-place twin."""
    o = alloc_quant(row, *args)
    if row.optional:
        args = _no_none(args, row.optional)
    lead = row.lead
    getattr(torch.ops.qutlass_amd_mxf6 if row.fmt == "mxf6" else _AMD, row.twin)(*args[:lead], o[0], o[1], *args[lead + (row.fmt == "mxf8" and row.dtype is None):])
    return o


# ---- every other op that fills caller-allocated results: functional op, fake kernel and eager wrapper come from this table as well --------------------------------
# schema:   of the functional op `qutlass_amd::<name>`
# twin:     the in-place op of csrc/torch_ext.cpp (a trimmed op library has no training-only twins: their rows are not registered)
# alloc:    the uninitialised results, from the functional op's arguments -- the one allocator of the fake kernel, the functional op and the eager wrapper
# call:     (twin, results, *arguments): the twin's argument order
# optional: as QuantOp's
class OutputOp(NamedTuple):
    schema: str
    twin: str
    alloc: Callable
    call: Callable
    optional: tuple = ()


def _alloc_act(X, *rest):   # gated MLP: X is (.., 2 I) [gate | up]
    return X.new_empty((*X.shape[:-1], X.size(-1) // 2))


def _alloc_combined(Y, pos, *rest):   # (M, H) sorted rows, (T, topk) -> (T, H)
    return Y.new_empty((pos.size(0), Y.size(-1)))


def _alloc_topk(logits, topk, *rest):   # (T, E) logits -> (T, topk) weights and ids
    return logits.new_empty((logits.size(0), topk), dtype=torch.float32), logits.new_empty((logits.size(0), topk), dtype=torch.int32)


def _alloc_topk_grouped(logits, bias, topk, *rest):   # the third result is the (T, E) scores, or an empty tensor when they are not asked for (rest[-1]: return_scores)
    return _alloc_topk(logits, topk) + (logits.new_empty(tuple(logits.shape) if rest[-1] else (0,), dtype=torch.float32),)


def _call_topk_grouped(twin, o, logits, bias, topk, n_group, topk_group, scoring, renormalize, routed_scaling_factor, return_scores):
    """(an empty bias is the in-place op's "no bias")"""
    if bias is not None and bias.numel() == 0:
        raise ValueError("bias must have E entries")
    twin(logits, logits.new_empty((0,), dtype=torch.float32) if bias is None else bias, o[0], o[1], o[2], n_group, topk_group, scoring, renormalize, routed_scaling_factor)


def _alloc_sort(topk_ids, expert_map, num_experts):
    """src_row, offs, pos; the kernels write every element, except that an empty sort launches nothing: offs is allocated as zeros always (one tiny fill), so no
    branch on the number of slots is traced"""
    return (topk_ids.new_empty((topk_ids.numel(),), dtype=torch.int32), topk_ids.new_zeros((num_experts,), dtype=torch.int32),
            topk_ids.new_empty(tuple(topk_ids.shape), dtype=torch.int32))


def _call_sort(twin, o, topk_ids, expert_map, num_experts):
    """with the scratch of the three-launch form (none up to the one-launch bound); an empty expert_map is the in-place op's "no map"."""
    if expert_map is not None and expert_map.numel() == 0:
        raise ValueError("expert_map must have at least one entry")
    ws = topk_ids.new_empty((_lib.load().qutlass_amd_moe_sort_workspace_bytes(topk_ids.numel(), num_experts) // 4,), dtype=torch.int32)
    twin(topk_ids, topk_ids.new_empty((0,), dtype=torch.int32) if expert_map is None else expert_map, num_experts, o[0], o[1], o[2], ws)


def _alloc_mask(A, R):   # fusedQuantizeMx's results and the clip mask, one bit per element
    return alloc_quant(QUANT_OPS["quantize_mx"], A) + (A.new_empty((*A.shape[:-1], A.size(-1) // 8), dtype=torch.uint8),)


# The two QAT-backward transposes allocate on h's device, as the reference's wrappers do (for every valid call that is x's device).
def _alloc_backward_t(x, h):   # (.., N, M) -> (.., M, N/2) e2m1x2, (.., M, N/32) e8m0
    return (h.new_empty((*x.shape[:-2], x.size(-1), x.size(-2) // 2), dtype=torch.float4_e2m1fn_x2),
            h.new_empty((*x.shape[:-2], x.size(-1), x.size(-2) // 32), dtype=torch.float8_e8m0fnu))


def _alloc_backward_qt(c, s, h, alpha):   # the same from x_e2m1 (.., N, M/2) and x_e8m0 (.., N, M/32)
    return (h.new_empty((*c.shape[:-2], c.size(-1) * 2, c.size(-2) // 2), dtype=torch.float4_e2m1fn_x2),
            h.new_empty((*s.shape[:-2], s.size(-1) * 32, s.size(-2) // 32), dtype=torch.float8_e8m0fnu))


def _alloc_square_double(x):   # (m, n) -> e4m3 (m_pad, n), row scales (m_pad, n/32), column scales (n, m_pad/32); m_pad: m rounded up to 128
    mp, n = (x.size(0) + 127) // 128 * 128, x.size(1)
    return (x.new_empty((mp, n), dtype=torch.float8_e4m3fn), x.new_empty((mp, n // 32), dtype=torch.float8_e8m0fnu),
            x.new_empty((n, mp // 32), dtype=torch.float8_e8m0fnu))


def _alloc_transpose(x, s):   # packed (m, n/2) -> e4m3 (n, m_pad), scales (n, m_pad/32); m_pad: m rounded up to 256, as in the reference
    mp, n = (x.size(0) + 255) // 256 * 256, x.size(1) * 2
    return x.new_empty((n, mp), dtype=torch.float8_e4m3fn), x.new_empty((n, mp // 32), dtype=torch.float8_e8m0fnu)


OUTPUT_OPS = {
    "silu_and_mul": OutputOp("(Tensor X) -> Tensor", "siluAndMul_", _alloc_act, lambda twin, o, X: twin(X, o)),
    "moe_combine": OutputOp("(Tensor Y, Tensor pos, Tensor weights) -> Tensor", "moeCombine_", _alloc_combined, lambda twin, o, Y, pos, weights: twin(Y, pos, weights, o)),
    # gpt-oss: the clamped SwiGLU with an optional per-expert bias (E, 2 I) and the grouped GEMMs' offs (E,); moe_combine with the down bias (E, H)
    "swiglu_oai_and_mul": OutputOp("(Tensor X, float alpha, float limit, Tensor? bias, Tensor? offs) -> Tensor", "swigluOaiAndMul_", _alloc_act,
                                   lambda twin, o, X, alpha, limit, bias, offs: twin(X, o, alpha, limit, bias, offs), ((3, None), (4, torch.int32))),
    "moe_combine_bias": OutputOp("(Tensor Y, Tensor pos, Tensor weights, Tensor bias, Tensor? offs) -> Tensor", "moeCombineBias_", _alloc_combined,
                                 lambda twin, o, Y, pos, weights, bias, offs: twin(Y, pos, weights, bias, offs, o), ((4, torch.int32),)),
    # MoE routing: (T, E) logits -> (T, topk) weights and ids; (T, topk) ids -> src_row (T * topk), offs (num_experts), pos (T, topk)
    "moe_topk_softmax": OutputOp("(Tensor logits, int topk, bool renormalize) -> (Tensor, Tensor)", "moeTopkSoftmax_", _alloc_topk,
                                 lambda twin, o, logits, topk, renormalize: twin(logits, o[0], o[1], renormalize)),
    "moe_topk_grouped": OutputOp("(Tensor logits, Tensor? bias, int topk, int n_group, int topk_group, int scoring, bool renormalize, float routed_scaling_factor, "
                                 "bool return_scores) -> (Tensor, Tensor, Tensor)", "moeTopkGrouped_", _alloc_topk_grouped, _call_topk_grouped),
    "moe_sort_fused": OutputOp("(Tensor topk_ids, Tensor? expert_map, int num_experts) -> (Tensor, Tensor, Tensor)", "moeSort_", _alloc_sort, _call_sort),
    # training only: the clip-mask quantizer and the QAT-backward data preparation
    "quantize_mx_mask": OutputOp("(Tensor A, Tensor R) -> (Tensor, Tensor, Tensor)", "fusedQuantizeMxMask_", _alloc_mask, lambda twin, o, A, R: twin(A, R, *o)),
    "backward_t": OutputOp("(Tensor x, Tensor h) -> (Tensor, Tensor)", "backward_t_bf16_", _alloc_backward_t, lambda twin, o, x, h: twin(x, h, *o)),
    "backward_qt": OutputOp("(Tensor x_e2m1, Tensor x_e8m0, Tensor h, Tensor alpha) -> (Tensor, Tensor)", "backward_qt_bf16_", _alloc_backward_qt,
                            lambda twin, o, x_e2m1, x_e8m0, h, alpha: twin(x_e2m1, x_e8m0, h, alpha, *o)),
    "square_double_mxfp8": OutputOp("(Tensor x_bf16) -> (Tensor, Tensor, Tensor)", "backward_bf16_square_double_mxfp8_", _alloc_square_double,
                                    lambda twin, o, x_bf16: twin(x_bf16, *o)),
    "transpose_mxfp8": OutputOp("(Tensor x_fp4, Tensor scales) -> (Tensor, Tensor)", "mxfp4_transpose_mxfp8_", _alloc_transpose,
                                lambda twin, o, x_fp4, scales: twin(x_fp4, scales, *o)),
}


def run_output(row: OutputOp, *args):
    """Allocate, then the in-place twin."""
    _, twin, alloc, call, optional = row
    o = alloc(*args)
    if optional:
        args = _no_none(args, optional)
    call(getattr(_AMD, twin), o, *args)
    return o


def to_blocked(input_matrix: torch.Tensor) -> torch.Tensor:
    """qutlass/utils.py:160-193 as a HIP kernel (csrc/to_blocked.hip.h) -> flat blocked byte vector, input dtype."""
    register_torch_ops()
    return torch.ops.qutlass_amd.to_blocked(input_matrix)
