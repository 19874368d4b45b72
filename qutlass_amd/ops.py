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

    for name in ("fusedQuantizeMx_", "fusedQuantizeNv_", "fusedQuantizeMxMask_", "fusedQuantizeMxBlocked", "fusedQuantizeNvBlocked",
                 "siluAndMul_", "fusedSiluMulQuantizeMx_", "fusedSiluMulQuantizeNv_",
                 "fusedGatherQuantizeMx_", "fusedGatherQuantizeNv_", "fusedGatherQuantizeNvGrouped_", "fusedSiluMulQuantizeNvGrouped_",
                 "fusedQuantizeMxf8_", "fusedQuantizeMxf8Blocked_", "fusedSiluMulQuantizeMxf8_", "fusedGatherQuantizeMxf8_", "moeCombine_",
                 "swigluOaiAndMul_", "fusedSwigluOaiQuantizeMx_", "fusedSwigluOaiQuantizeMxf8_", "moeCombineBias_", "moeTopkSoftmax_", "moeTopkGrouped_", "moeSort_", "backward_t_bf16_", "backward_qt_bf16_", "backward_bf16_square_double_mxfp8_", "mxfp4_transpose_mxfp8_"):
        rf(f"qutlass_amd::{name}")(fills)

    @rf("qutlass_amd::to_blocked")
    def _(input_matrix):
        rows, cols = input_matrix.shape
        return input_matrix.new_empty(((rows + 127) // 128 * 128) * ((cols + 3) // 4 * 4))

    @rf("qutlass_amd::fusedQuantizeMatmulMxf4")
    def _(X, R, B, B_sf, alpha, method):
        k = X.size(-1)
        return X.new_empty((X.numel() // k if k else 0, B.size(0)), dtype=torch.bfloat16)

    def grouped_tn(A, B, A_sf, B_sf, alpha, offs):   # A (M, K/2 or K), B (E, N, K/2 or K)
        return A.new_empty((A.size(0), B.size(1)), dtype=torch.bfloat16)

    for name in ("grouped_matmul_mxf4", "grouped_matmul_mxf8", "grouped_matmul_nvf4", "grouped_matmul_mxf8_mxf4"):
        rf(f"qutlass_amd::{name}")(grouped_tn)


def _define_functional_ops() -> None:
    """FUNCTIONAL forms of the output-filling ops (`qutlass_amd::quantize_mx` ...: allocate, call the in-place twin, return fresh tensors), defined in Python with
    `torch.library.custom_op`.  The wrappers of qutlass_amd/__init__.py call them only while a graph is being compiled (`torch.compiler.is_compiling()`): inductor (torch
    2.10) refuses every node that touches a `float8_e8m0fnu` tensor except views / cat / clone / `_scaled_mm` (torch/_inductor/lowering.py `unsupported_input_tensor`), so
    the `auto_functionalized` wrapper of a mutating op with an e8m0 argument is never decomposed and compilation dies ("auto_functionalized_v2 was not removed") -- while a
    functional op with e8m0 results is simply called as an extern kernel.  Eager callers keep the direct C++ path (a Python custom op costs ~10 us per call)."""
    if hasattr(torch.ops.qutlass_amd, "quantize_mx"):
        return
    from torch.library import custom_op

    amd = torch.ops.qutlass_amd
    have_training_ops = hasattr(amd, "backward_t_bf16_")

    # the rotate + quantize family: one registration per row of QUANT_OPS
    for name, row in QUANT_OPS.items():
        op = custom_op(f"qutlass_amd::{name}", mutates_args=(), schema=row.schema)(lambda *args, _row=row: run_quant_op(_row, *args))
        op.register_fake(lambda *args, _row=row: alloc_quant(_row, *args))
    # the e4m3 form of the clamped-SwiGLU quantizer: its record stands next to the table (see SWIGLU_OAI_MXF8), not in it
    op = custom_op("qutlass_amd::swiglu_oai_quantize_mxf8", mutates_args=(), schema=SWIGLU_OAI_MXF8.schema)(lambda *args: run_swiglu_oai_quant(SWIGLU_OAI_MXF8, *args))
    op.register_fake(lambda A, R, *rest: alloc_swiglu_oai_quant(SWIGLU_OAI_MXF8, A, R))

    # gated MLP: X is (.., 2 I) [gate | up]
    @custom_op("qutlass_amd::silu_and_mul", mutates_args=(), schema="(Tensor X) -> Tensor")
    def silu_and_mul(X):
        o = X.new_empty(_act(X))
        amd.siluAndMul_(X, o)
        return o

    silu_and_mul.register_fake(lambda X: X.new_empty(_act(X)))

    def _combined(Y, pos):
        return Y.new_empty((pos.size(0), Y.size(-1)))

    @custom_op("qutlass_amd::moe_combine", mutates_args=(), schema="(Tensor Y, Tensor pos, Tensor weights) -> Tensor")
    def moe_combine(Y, pos, weights):
        o = _combined(Y, pos)
        amd.moeCombine_(Y, pos, weights, o)
        return o

    moe_combine.register_fake(lambda Y, pos, weights: _combined(Y, pos))

    # gpt-oss: the clamped SwiGLU with an optional per-expert bias (E, 2 I) and the grouped GEMMs' offs (E,); moe_combine with the down bias (E, H)
    @custom_op("qutlass_amd::swiglu_oai_and_mul", mutates_args=(), schema="(Tensor X, float alpha, float limit, Tensor? bias, Tensor? offs) -> Tensor")
    def swiglu_oai_and_mul(X, alpha, limit, bias, offs):
        return run_swiglu_oai(X, alpha, limit, bias, offs)

    swiglu_oai_and_mul.register_fake(lambda X, alpha, limit, bias, offs: X.new_empty(_act(X)))

    @custom_op("qutlass_amd::moe_combine_bias", mutates_args=(), schema="(Tensor Y, Tensor pos, Tensor weights, Tensor bias, Tensor? offs) -> Tensor")
    def moe_combine_bias(Y, pos, weights, bias, offs):
        return run_moe_combine_bias(Y, pos, weights, bias, offs)

    moe_combine_bias.register_fake(lambda Y, pos, weights, bias, offs: _combined(Y, pos))

    # MoE routing: (T, E) logits -> (T, topk) weights and ids; (T, topk) ids -> src_row (T * topk), offs (num_experts), pos (T, topk)
    @custom_op("qutlass_amd::moe_topk_softmax", mutates_args=(), schema="(Tensor logits, int topk, bool renormalize) -> (Tensor, Tensor)")
    def moe_topk_softmax(logits, topk, renormalize):
        o = _alloc_topk(logits, topk)
        amd.moeTopkSoftmax_(logits, o[0], o[1], renormalize)
        return o

    moe_topk_softmax.register_fake(lambda logits, topk, renormalize: _alloc_topk(logits, topk))

    # the grouped router: the third result is the (T, E) scores, or an empty tensor when they are not asked for
    @custom_op("qutlass_amd::moe_topk_grouped", mutates_args=(),
               schema="(Tensor logits, Tensor? bias, int topk, int n_group, int topk_group, int scoring, bool renormalize, float routed_scaling_factor, bool return_scores) -> (Tensor, Tensor, Tensor)")
    def moe_topk_grouped(logits, bias, topk, n_group, topk_group, scoring, renormalize, routed_scaling_factor, return_scores):
        return run_moe_topk_grouped(logits, bias, topk, n_group, topk_group, scoring, renormalize, routed_scaling_factor, return_scores)

    moe_topk_grouped.register_fake(lambda logits, bias, topk, n_group, topk_group, scoring, renormalize, routed_scaling_factor, return_scores:
                                   _alloc_topk(logits, topk) + (_alloc_scores(logits, return_scores),))

    @custom_op("qutlass_amd::moe_sort_fused", mutates_args=(), schema="(Tensor topk_ids, Tensor? expert_map, int num_experts) -> (Tensor, Tensor, Tensor)")
    def moe_sort_fused(topk_ids, expert_map, num_experts):
        return run_moe_sort(topk_ids, expert_map, num_experts)

    moe_sort_fused.register_fake(lambda topk_ids, expert_map, num_experts: _alloc_sort(topk_ids, num_experts))

    if not have_training_ops:   # QUTLASS_MINIMAL_BUILD: inference ops only
        return

    def _mask(a):
        return alloc_quant(QUANT_OPS["quantize_mx"], a) + (a.new_empty((*a.shape[:-1], a.size(-1) // 8), dtype=torch.uint8),)

    @custom_op("qutlass_amd::quantize_mx_mask", mutates_args=(), schema="(Tensor A, Tensor R) -> (Tensor, Tensor, Tensor)")
    def quantize_mx_mask(A, R):
        o = _mask(A)
        amd.fusedQuantizeMxMask_(A, R, o[0], o[1], o[2])
        return o

    quantize_mx_mask.register_fake(lambda A, R: _mask(A))

    def _bt(x):   # (.., N, M) -> (.., M, N/2) e2m1x2, (.., M, N/32) e8m0
        return (x.new_empty((*x.shape[:-2], x.size(-1), x.size(-2) // 2), dtype=torch.float4_e2m1fn_x2),
                x.new_empty((*x.shape[:-2], x.size(-1), x.size(-2) // 32), dtype=torch.float8_e8m0fnu))

    @custom_op("qutlass_amd::backward_t", mutates_args=(), schema="(Tensor x, Tensor h) -> (Tensor, Tensor)")
    def backward_t(x, h):
        o = _bt(x)
        amd.backward_t_bf16_(x, h, o[0], o[1])
        return o

    backward_t.register_fake(lambda x, h: _bt(x))

    def _bqt(c, s):
        return (c.new_empty((*c.shape[:-2], c.size(-1) * 2, c.size(-2) // 2), dtype=torch.float4_e2m1fn_x2),
                c.new_empty((*s.shape[:-2], s.size(-1) * 32, s.size(-2) // 32), dtype=torch.float8_e8m0fnu))

    @custom_op("qutlass_amd::backward_qt", mutates_args=(), schema="(Tensor x_e2m1, Tensor x_e8m0, Tensor h, Tensor alpha) -> (Tensor, Tensor)")
    def backward_qt(x_e2m1, x_e8m0, h, alpha):
        o = _bqt(x_e2m1, x_e8m0)
        amd.backward_qt_bf16_(x_e2m1, x_e8m0, h, alpha, o[0], o[1])
        return o

    backward_qt.register_fake(lambda x_e2m1, x_e8m0, h, alpha: _bqt(x_e2m1, x_e8m0))

    def _sq(x):
        m, n = x.shape
        mp = (m + 127) // 128 * 128
        return (x.new_empty((mp, n), dtype=torch.float8_e4m3fn), x.new_empty((mp, n // 32), dtype=torch.float8_e8m0fnu),
                x.new_empty((n, mp // 32), dtype=torch.float8_e8m0fnu))

    @custom_op("qutlass_amd::square_double_mxfp8", mutates_args=(), schema="(Tensor x_bf16) -> (Tensor, Tensor, Tensor)")
    def square_double_mxfp8(x_bf16):
        o = _sq(x_bf16)
        amd.backward_bf16_square_double_mxfp8_(x_bf16, o[0], o[1], o[2])
        return o

    square_double_mxfp8.register_fake(lambda x_bf16: _sq(x_bf16))

    def _tr(x, s):
        m, n = x.shape[0], x.shape[1] * 2
        mp = (m + 255) // 256 * 256
        return x.new_empty((n, mp), dtype=torch.float8_e4m3fn), x.new_empty((n, mp // 32), dtype=torch.float8_e8m0fnu)

    @custom_op("qutlass_amd::transpose_mxfp8", mutates_args=(), schema="(Tensor x_fp4, Tensor scales) -> (Tensor, Tensor)")
    def transpose_mxfp8(x_fp4, scales):
        o = _tr(x_fp4, scales)
        amd.mxfp4_transpose_mxfp8_(x_fp4, scales, o[0], o[1])
        return o

    transpose_mxfp8.register_fake(lambda x_fp4, scales: _tr(x_fp4, scales))


# ---- the rotate + quantize family: the functional ops `qutlass_amd::<name>`, their fake kernels and the eager wrappers of __init__.py come from this table ----------
# schema:  of the functional op -- the leading tensors, [global_scale | global_scales, offs,] method[, blocked]
# twin:    the in-place op of csrc/torch_ext.cpp: the same arguments with OUT, OUT_sf inserted after the `lead` leading tensors
# operand: the shape of the tensor that is rotated and quantized, from the leading tensors -- the results are the plain quantizers' for a tensor of that shape
# fmt:     a key of QUANT_FORMATS;  blocked: scales flat in the to_blocked() layout -- fixed by the op, or None where it is the op's last argument
# The "mxf8" ops have no method: the argument behind the leading tensors is the code dtype (float8_e4m3fn / float8_e5m2).  It decides what is allocated and is not
# passed on to the twin, which reads the format off OUT's dtype.
class QuantOp(NamedTuple):
    schema: str
    twin: str
    lead: int
    operand: Callable
    fmt: str
    blocked: bool | None


def _same(A, R=None):
    return tuple(A.shape)


def _act(X, R=None):   # gated MLP: X is (.., 2 I) [gate | up], the operand (.., I)
    return (*X.shape[:-1], X.size(-1) // 2)


def _gathered(A, R, src_row):   # MoE dispatch: the operand is A[src_row], (M, K) for M indices
    return (src_row.size(0), A.size(-1))


QUANT_FORMATS = {"mx": (32, torch.float8_e8m0fnu), "nv": (16, torch.float8_e4m3fn), "mxf8": (32, torch.float8_e8m0fnu)}   # elements per scale, scale dtype
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
                                      "fusedSwigluOaiQuantizeMx_", 2, _act, "mx", False),
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
}
# The clamped SwiGLU into e4m3 -- the A operand of the W4A8 grouped GEMM.  Outside the table on purpose: the table's "mxf8" rows take a code dtype and every rotation,
# this op is e4m3 only (no dtype argument), R = 32 / 64, and takes alpha / limit / bias / offs; it is registered beside the loop over QUANT_OPS.
SWIGLU_OAI_MXF8 = QuantOp("(Tensor A, Tensor R, float alpha, float limit, Tensor? bias, Tensor? offs) -> (Tensor, Tensor)", "fusedSwigluOaiQuantizeMxf8_", 2, _act, "mxf8",
                          False)


def mxf8_dtype(dtype) -> torch.dtype:
    if dtype not in MXF8_DTYPES:
        raise ValueError(f"invalid dtype {dtype!r}, must be torch.float8_e4m3fn or torch.float8_e5m2")
    return dtype


def alloc_quant(row: QuantOp, *args):
    """The results of one family op, uninitialised: packed e2m1 (.., K / 2) uint8 -- "mxf8": (.., K) codes in the dtype asked for -- and the scales -- (padded_rows,
    padded_cols), or their product flat when blocked -- of the operand (.., K); args as the functional op takes them.  The one allocator of the fake kernels, the
    functional ops and the eager wrappers."""
    shape = row.operand(*args[:row.lead])
    group, sf_dtype = QUANT_FORMATS[row.fmt]
    pr, pc = padded_scale_shape(math.prod(shape) // shape[-1], shape[-1], group)
    blocked = args[-1] if row.blocked is None else row.blocked
    codes = args[0].new_empty(shape, dtype=mxf8_dtype(args[row.lead])) if row.fmt == "mxf8" else args[0].new_empty((*shape[:-1], shape[-1] // 2), dtype=torch.uint8)
    return codes, args[0].new_empty((pr * pc,) if blocked else (pr, pc), dtype=sf_dtype)


def run_quant(row: QuantOp, *args):
    """Allocate, then the in-place twin."""
    o = alloc_quant(row, *args)
    getattr(torch.ops.qutlass_amd, row.twin)(*args[:row.lead], o[0], o[1], *args[row.lead + (row.fmt == "mxf8"):])
    return o


def run_quant_op(row: QuantOp, *args):
    """run_quant -- or, for the clamped-SwiGLU ops, which take optional tensors, their own runner (the in-place twins take no None)."""
    return (run_swiglu_oai_quant if row.twin.startswith("fusedSwigluOaiQuantize") else run_quant)(row, *args)


def _optional(x: torch.Tensor, t: torch.Tensor | None, dtype: torch.dtype) -> torch.Tensor:
    """The in-place ops' "no tensor": an empty one."""
    return x.new_empty((0,), dtype=dtype) if t is None else t


def alloc_swiglu_oai_quant(row: QuantOp, A, R):
    """alloc_quant for the clamped-SwiGLU ops: the e4m3 form has no dtype argument (a forward activation is e4m3 only)."""
    return alloc_quant(row, A, R, *((torch.float8_e4m3fn,) if row.fmt == "mxf8" else ()))


def run_swiglu_oai_quant(row: QuantOp, A, R, alpha, limit, bias, offs, *method):
    """run_quant for the ops with optional tensors: the MXFP4 row of the table (method: one int) and SWIGLU_OAI_MXF8 (abs-max only: no method)."""
    o = alloc_swiglu_oai_quant(row, A, R)
    getattr(torch.ops.qutlass_amd, row.twin)(A, R, o[0], o[1], alpha, limit, _optional(A, bias, A.dtype), _optional(A, offs, torch.int32), *method)
    return o


def run_swiglu_oai(X, alpha, limit, bias, offs):
    o = X.new_empty(_act(X))
    torch.ops.qutlass_amd.swigluOaiAndMul_(X, o, alpha, limit, _optional(X, bias, X.dtype), _optional(X, offs, torch.int32))
    return o


def run_moe_combine_bias(Y, pos, weights, bias, offs):
    o = Y.new_empty((pos.size(0), Y.size(-1)))
    torch.ops.qutlass_amd.moeCombineBias_(Y, pos, weights, bias, _optional(Y, offs, torch.int32), o)
    return o


def _alloc_topk(logits: torch.Tensor, topk: int):
    return logits.new_empty((logits.size(0), topk), dtype=torch.float32), logits.new_empty((logits.size(0), topk), dtype=torch.int32)


def _alloc_scores(logits: torch.Tensor, wanted: bool):
    return logits.new_empty(tuple(logits.shape) if wanted else (0,), dtype=torch.float32)


def run_moe_topk_grouped(logits: torch.Tensor, bias: torch.Tensor | None, topk: int, n_group: int, topk_group: int, scoring: int, renormalize: bool,
                         routed_scaling_factor: float, return_scores: bool):
    """Allocate weights, ids and scores (empty when not asked for), then the in-place op; an empty bias is its "no bias"."""
    if bias is not None and bias.numel() == 0:
        raise ValueError("bias must have E entries")
    weights, ids = _alloc_topk(logits, topk)
    scores = _alloc_scores(logits, return_scores)
    no_bias = logits.new_empty((0,), dtype=torch.float32)
    torch.ops.qutlass_amd.moeTopkGrouped_(logits, no_bias if bias is None else bias, weights, ids, scores, n_group, topk_group, scoring, renormalize,
                                          routed_scaling_factor)
    return weights, ids, scores


def _alloc_sort(topk_ids: torch.Tensor, num_experts: int):
    """src_row, offs, pos; the kernels write every element, except that an empty sort launches nothing: offs is allocated as zeros always (one tiny fill), so no
    branch on the number of slots is traced"""
    return (topk_ids.new_empty((topk_ids.numel(),), dtype=torch.int32), topk_ids.new_zeros((num_experts,), dtype=torch.int32),
            topk_ids.new_empty(tuple(topk_ids.shape), dtype=torch.int32))


def run_moe_sort(topk_ids: torch.Tensor, expert_map: torch.Tensor | None, num_experts: int):
    """Allocate the three results and the scratch of the three-launch form (none up to the one-launch bound), then the in-place op."""
    if expert_map is not None and expert_map.numel() == 0:
        raise ValueError("expert_map must have at least one entry")
    out = _alloc_sort(topk_ids, num_experts)
    ws = topk_ids.new_empty((_lib.load().qutlass_amd_moe_sort_workspace_bytes(topk_ids.numel(), num_experts) // 4,), dtype=torch.int32)
    no_map = topk_ids.new_empty((0,), dtype=torch.int32)   # the in-place op's "no map"
    torch.ops.qutlass_amd.moeSort_(topk_ids, no_map if expert_map is None else expert_map, num_experts, out[0], out[1], out[2], ws)
    return out


def to_blocked(input_matrix: torch.Tensor) -> torch.Tensor:
    """qutlass/utils.py:160-193 as a HIP kernel (csrc/to_blocked.hip.h) -> flat blocked byte vector, input dtype."""
    register_torch_ops()
    return torch.ops.qutlass_amd.to_blocked(input_matrix)
