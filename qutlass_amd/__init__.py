"""qutlass_amd -- MI355X-native (gfx950 / CDNA4) implementation of the qutlass operator surface.

Public API = the hot-path functions of the reference's ``qutlass/__init__.py`` (same names, argument
meaning, defaults and Python-level error behaviour):

    fusedQuantizeMx, fusedQuantizeNv, matmul_mxf4_bf16_tn, matmul_nvf4_bf16_tn,
    matmul_mxf8_bf16_tn, matmul_mxf8_bf16_nn         (+ qutlass_amd.utils.to_blocked & friends)
    matmul_ada_mxf4_bf16_tn, backward_t_bf16, backward_qt_bf16, backward_bf16_square_double_mxfp8, mxfp4_transpose_mxfp8
    grouped_matmul_mxf4_bf16_tn                      (extension: mixture-of-experts layers, one launch over all experts)
    grouped_matmul_mxf8_bf16_tn                      (extension: the same for MXFP8, e4m3 or e5m2 tokens)
    grouped_matmul_nvf4_bf16_tn                      (extension: the same for NVFP4, row-major e4m3 scales per 16 elements)
    grouped_matmul_mxf8_mxf4_bf16_tn, matmul_mxf8_mxf4_bf16_tn  (extension: W4A8 -- MXFP8 tokens against MXFP4 expert weights as stored; the dense form is E = 1)
    grouped_matmul_mxf6_mxf4_bf16_tn, matmul_mxf6_mxf4_bf16_tn  (extension: W4A6 -- MXFP6 (e2m3) tokens against the same weights: W4A8's accuracy class at 3/4 of its token bytes)
    fusedQuantizeMxf6, fusedGatherQuantizeMxf6            (extension: the MXFP6 quantizers -- the A operand of the W4A6 GEMM)
    grouped_matmul_bf16_mxf4_bf16_tn, matmul_bf16_mxf4_bf16_tn  (extension: W4A16 -- bf16 tokens against the same weights, optionally gathered by src_row in the GEMM)
    silu_and_mul, fusedSiluMulQuantizeMx / Nv [Blocked]  (extension: the gated-MLP activation, alone and fused into the quantizers)
    moe_sort, fusedGatherQuantizeMx / Nv, moe_combine     (extension: MoE dispatch and combine around the grouped GEMMs)
    fusedGatherQuantizeNvGrouped, fusedSiluMulQuantizeNvGrouped  (extension: the two NVFP4 quantizers of the MoE chain with one global scale per expert)
    fusedQuantizeMxf8 [Blocked], fusedGatherQuantizeMxf8, fusedSiluMulQuantizeMxf8 [Blocked]  (extension: the MXFP8 quantizers -- the operands of the three MXFP8 GEMMs)
    moe_topk_softmax, moe_sort_fused, moe_route           (extension: MoE routing in HIP -- router logits to ids, weights and the sorted-row metadata)
    moe_topk_grouped, moe_route_grouped                   (extension: the grouped router of DeepSeek-V2 / V3 and Kimi-K2 -- sigmoid / softmax scores, selection bias, group-limited top-k)
    moe_route_fused, moe_route_grouped_fused              (extension: both routings in ONE launch for decode batches -- router and sort in one workgroup, the same bits)
    swiglu_oai_and_mul, fusedSwigluOaiQuantizeMx, moe_combine(bias=, offs=)  (extension: gpt-oss -- the clamped SwiGLU and the per-expert biases of both projections,
                                                          applied by the ops that read the grouped GEMMs' outputs; utils.split_interleaved_gate_up for the checkpoint layout)
    fusedSwigluOaiQuantizeMxf8                            (extension: the same activation into e4m3 -- the A operand of the W4A8 grouped GEMM, one launch)

All compute is hand-written HIP behind the C ABI of ``include/qutlass_amd.h``
(``libqutlass_amd.so``); importing this package loads that library and registers
``torch.ops._qutlass_C.*``.  There is no CPU or eager-PyTorch fallback: if the library is not built
the import fails, and every op requires GPU tensors.
"""
from __future__ import annotations

from typing import Literal

import torch

from . import _lib, ops
from .utils import ceil_div, get_padded_shape_mx, get_padded_shape_nv, pad_to_block, to_blocked  # noqa: F401

__version__ = "0.2.0"

_lib.load()                 # fail loudly at import time if the HIP library is missing
ops.register_torch_ops()    # torch.ops._qutlass_C.<op>  (reference: bindings.cpp:498-535)

qutlass_CUDA = torch.ops._qutlass_C
_ops_amd = torch.ops.qutlass_amd   # extensions + the mutation-declaring twins of the reference's output-filling ops
_METHOD_CODE = {"quest": 0, "abs_max": 1}

_FLASHINFER_MSG = (
    "flashinfer backend requested but not installed. flashinfer/cuDNN is an NVIDIA-only backend and is "
    "not available in the MI355X build; use backend='cutlass' (the native gfx950 kernels)."
)


def matmul_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                        alpha: torch.Tensor,
                        backend: Literal["cutlass", "flashinfer"] = "cutlass") -> torch.Tensor:
    """qutlass/__init__.py:34-76.  ``backend="cutlass"`` selects the native kernel (name kept for
    drop-in compatibility); ``"flashinfer"`` raises ImportError exactly as the reference does when
    flashinfer is absent."""
    if backend == "cutlass":
        return qutlass_CUDA.matmul_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha)
    elif backend == "flashinfer":
        raise ImportError(_FLASHINFER_MSG)
    else:
        raise ValueError(f"invalid backend {backend!r}; use 'cutlass' or 'flashinfer'")


def matmul_ada_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                            alpha: torch.Tensor) -> torch.Tensor:
    """qutlass/__init__.py:79-86: small-batch MXFP4 GEMM taking the UN-swizzled (rows, K/32) scales."""
    return qutlass_CUDA.matmul_ada_mxf4_bf16_tn(a, b, a_sf, b_sf, alpha)


def grouped_matmul_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                                alpha: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): grouped MXFP4 GEMM for mixture-of-experts layers, one launch over all experts.

    a      (M, K/2) uint8 / float4_e2m1fn_x2 -- the tokens, sorted by expert
    b      (E, N, K/2) uint8 / float4_e2m1fn_x2 -- the stacked expert weights
    a_sf   float8_e8m0fnu, >= M*K/32 elements, read as row-major (M, K/32): fusedQuantizeMx's scale buffer as is (like matmul_ada_mxf4_bf16_tn)
    b_sf   float8_e8m0fnu, >= E*N*K/32 elements, read as row-major (E, N, K/32)
    alpha  float32, 1 element (shared) or E elements (per expert)
    offs   int32 (E,): the cumulative END rows of the groups (torch._grouped_mm's convention) -- group g is rows [offs[g-1], offs[g]), offs[-1] := 0

    Returns out (M, N) bf16 with out[r] = alpha[g] * (A_r . SFA) (B_g . SFB_g)^T for every row r of group g.  Empty groups are allowed; rows at or
    past offs[E-1] are not written (their contents are unspecified, as in torch._grouped_mm).  The offsets are read on the device, so the call
    needs no host sync and works under graph capture and torch.compile; each offset is clamped to [0, M] and a decreasing one is an empty group.
    K % 128 == 0, N % 8 == 0, 1 <= E <= 1024; one expert's weight below 2 GiB (the stack may exceed it).  M == 0 returns an empty output."""
    return _ops_amd.grouped_matmul_mxf4(a, b, a_sf, b_sf, alpha, offs)


def grouped_matmul_mxf8_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                                alpha: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): grouped MXFP8 GEMM for mixture-of-experts layers, one launch over all experts.

    a      (M, K) float8_e4m3fn or float8_e5m2 -- the tokens, sorted by expert (e5m2 selects the e5m2-A path, as in matmul_mxf8_bf16_tn: MoE dgrad)
    b      (E, N, K) float8_e4m3fn -- the stacked expert weights
    a_sf   float8_e8m0fnu, >= M*K/32 elements, read as row-major (M, K/32)
    b_sf   float8_e8m0fnu, >= E*N*K/32 elements, read as row-major (E, N, K/32)
    alpha  float32, 1 element (shared) or E elements (per expert)
    offs   int32 (E,): the cumulative END rows of the groups (torch._grouped_mm's convention) -- group g is rows [offs[g-1], offs[g]), offs[-1] := 0

    Returns out (M, N) bf16 with out[r] = alpha[g] * (A_r . SFA) (B_g . SFB_g)^T for every row r of group g.  Empty groups are allowed; rows at or
    past offs[E-1] are not written (their contents are unspecified, as in torch._grouped_mm).  The offsets are read on the device, so the call
    needs no host sync and works under graph capture and torch.compile; each offset is clamped to [0, M] and a decreasing one is an empty group.
    K % 128 == 0, N % 8 == 0, 1 <= E <= 1024; the token matrix and one expert's weight below 2 GiB (the stack may exceed it).  M == 0 returns an
    empty output."""
    return _ops_amd.grouped_matmul_mxf8(a, b, a_sf, b_sf, alpha, offs)


def _check_w4a8_operands(op: str, a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor, b_dim: int) -> None:
    """the rejections of the W4A8 ops that need no device: raised before the op is dispatched (shapes and dtypes only, so tracing goes through them)"""
    if a.dtype == torch.float8_e5m2:
        raise ValueError(f"{op}: a must be float8_e4m3fn, float8_e5m2 tokens are not supported (grouped_matmul_mxf8_bf16_tn takes them, against e4m3 weights)")
    if a.dtype != torch.float8_e4m3fn:
        raise ValueError(f"{op}: a must be float8_e4m3fn (got {a.dtype})")
    if b.dtype not in (torch.uint8, torch.float4_e2m1fn_x2):
        raise ValueError(f"{op}: b must be uint8 or float4_e2m1fn_x2 packed e2m1 (got {b.dtype})")
    if a.dim() != 2 or b.dim() != b_dim:
        raise ValueError(f"{op}: a must be 2D (M, K) and b {b_dim}D ({'E, ' if b_dim == 3 else ''}N, K/2)")
    if a.size(1) != 2 * b.size(-1):
        raise ValueError(f"{op}: inner dimensions must match, a is (M, K = {a.size(1)}) and b (.., K/2 = {b.size(-1)})")
    for name, sf, rows in (("a_sf", a_sf, a.size(0)), ("b_sf", b_sf, b.numel() // max(b.size(-1), 1))):
        if sf.dtype != torch.float8_e8m0fnu:
            raise ValueError(f"{op}: {name} must be float8_e8m0fnu (got {sf.dtype})")
        if sf.numel() < rows * (a.size(1) // 32):
            raise ValueError(f"{op}: {name} has {sf.numel()} elements, the row-major scale layout needs {rows * (a.size(1) // 32)}")


def grouped_matmul_mxf8_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                                     alpha: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): grouped W4A8 GEMM for mixture-of-experts layers -- MXFP8 tokens against MXFP4 expert weights as a checkpoint stores
    them (gpt-oss; every weight fusedQuantizeMx writes), one launch over all experts.

    a      (M, K) float8_e4m3fn -- the tokens, sorted by expert: what fusedQuantizeMxf8 / fusedGatherQuantizeMxf8 / fusedSiluMulQuantizeMxf8 write (e5m2 is rejected)
    b      (E, N, K/2) uint8 / float4_e2m1fn_x2 -- the stacked expert weights: what fusedQuantizeMx writes and grouped_matmul_mxf4_bf16_tn reads
    a_sf   float8_e8m0fnu, >= M*K/32 elements, read as row-major (M, K/32): the quantizer's flat scale buffer as it is (no to_blocked)
    b_sf   float8_e8m0fnu, >= E*N*K/32 elements, read as row-major (E, N, K/32)
    alpha  float32, 1 element (shared) or E elements (per expert)
    offs   int32 (E,): the cumulative END rows of the groups (torch._grouped_mm's convention) -- group g is rows [offs[g-1], offs[g]), offs[-1] := 0

    Returns out (M, N) bf16 with out[r] = alpha[g] * (A_r . SFA_r) (B_g . SFB_g)^T for every row r of group g: fp32 accumulation, one fp32 multiply by alpha, one
    rounding to bf16.  Empty groups are allowed; rows at or past offs[E-1] are not written.  The offsets are read on the device, so the call needs no host sync and
    works under graph capture and torch.compile; each offset is clamped to [0, M] and a decreasing one is an empty group.  Scale byte 255 and the e4m3 NaN code give
    NaN outputs as in grouped_matmul_mxf8_bf16_tn.  K % 128 == 0, N % 8 == 0, 1 <= E <= 1024; the token matrix and one expert's weight below 2 GiB (the stack may
    exceed it).  M == 0 returns an empty output.

    The op runs wave-owned 32x32 / 32x16 / 64x32 tiles only -- it has no 64x64 ring form, so prefill-sized groups run on the decode tiles (README, DESIGN.md
    section 8 for what that costs against grouped_matmul_mxf8_bf16_tn on weights upcast to e4m3)."""
    _check_w4a8_operands("grouped_matmul_mxf8_mxf4_bf16_tn", a, b, a_sf, b_sf, 3)
    return _ops_amd.grouped_matmul_mxf8_mxf4(a, b, a_sf, b_sf, alpha, offs)


def matmul_mxf8_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): the dense form of grouped_matmul_mxf8_mxf4_bf16_tn -- a (M, K) float8_e4m3fn against ONE MXFP4 weight b (N, K/2)
    uint8 / float4_e2m1fn_x2, flat row-major e8m0 scales (M, K/32) and (N, K/32) like matmul_ada_mxf4_bf16_tn's, alpha float32 with one element.  Returns (M, N)
    bf16.  The grouped op with E = 1: its offs is a one-element device tensor filled with M, so there is no host sync and no kernel of its own."""
    _check_w4a8_operands("matmul_mxf8_mxf4_bf16_tn", a, b, a_sf, b_sf, 2)
    offs = torch.full((1,), a.size(0), dtype=torch.int32, device=a.device)
    return _ops_amd.grouped_matmul_mxf8_mxf4(a, b.unsqueeze(0), a_sf, b_sf, alpha, offs)


def _check_w4a6_operands(op: str, a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor, b_dim: int) -> None:
    """the rejections of the W4A6 ops that need no device, in the manner of _check_w4a8_operands"""
    if a.dtype != torch.uint8:
        raise ValueError(f"{op}: a must be uint8, packed e2m3 codes as fusedQuantizeMxf6 writes them (got {a.dtype})")
    if b.dtype not in (torch.uint8, torch.float4_e2m1fn_x2):
        raise ValueError(f"{op}: b must be uint8 or float4_e2m1fn_x2 packed e2m1 (got {b.dtype})")
    if a.dim() != 2 or b.dim() != b_dim:
        raise ValueError(f"{op}: a must be 2D (M, 3K/4) and b {b_dim}D ({'E, ' if b_dim == 3 else ''}N, K/2)")
    if a.size(1) * 2 != 3 * b.size(-1):
        raise ValueError(f"{op}: inner dimensions must match, a is (M, 3K/4 = {a.size(1)}) and b (.., K/2 = {b.size(-1)})")
    k = 2 * b.size(-1)
    for name, sf, rows in (("a_sf", a_sf, a.size(0)), ("b_sf", b_sf, b.numel() // max(b.size(-1), 1))):
        if sf.dtype != torch.float8_e8m0fnu:
            raise ValueError(f"{op}: {name} must be float8_e8m0fnu (got {sf.dtype})")
        if sf.numel() < rows * (k // 32):
            raise ValueError(f"{op}: {name} has {sf.numel()} elements, the row-major scale layout needs {rows * (k // 32)}")


def grouped_matmul_mxf6_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                                     alpha: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): grouped W4A6 GEMM for mixture-of-experts layers -- MXFP6 (e2m3) tokens against MXFP4 expert weights as a checkpoint
    stores them, one launch over all experts.  e2m3 has e4m3's three mantissa bits and the block scale supplies the range it lacks: W4A8's accuracy class
    (README) at 3/4 of its token bytes.

    a      (M, 3K/4) uint8 -- the tokens, sorted by expert, as fusedQuantizeMxf6 / fusedGatherQuantizeMxf6 write them: element k of a row in bits 6k .. 6k+5 of the
           row read as one little-endian bit string (a 32-element scale block is 24 bytes); a code is sign, 2 exponent bits (bias 1), 3 mantissa bits
    b      (E, N, K/2) uint8 / float4_e2m1fn_x2 -- the stacked expert weights: what fusedQuantizeMx writes and grouped_matmul_mxf4_bf16_tn reads
    a_sf   float8_e8m0fnu, >= M*K/32 elements, read as row-major (M, K/32): the quantizer's flat scale buffer as it is
    b_sf   float8_e8m0fnu, >= E*N*K/32 elements, read as row-major (E, N, K/32)
    alpha  float32, 1 element (shared) or E elements (per expert)
    offs   int32 (E,): the cumulative END rows of the groups, as in grouped_matmul_mxf8_mxf4_bf16_tn

    Returns out (M, N) bf16 = bf16(alpha[g] * sum a b): exact products, fp32 sums, one rounding.  Rows at or past offs[E-1] are not written; each offset is clamped
    to [0, M] and a decreasing one is an empty group; the offsets are read on the device (graph capture, torch.compile).  Scale bytes 0 .. 254 mean 2^(b - 127);
    byte 255 on either side makes that row's or column's outputs NaN (the quantizers mark a group that held a NaN or an infinity that way).  K % 128 == 0,
    N % 8 == 0, 1 <= E <= 1024; the token matrix and one expert's weight below 2 GiB.  Wave-owned 32x32 / 32x16 / 64x32 tiles only, as for W4A8."""
    _check_w4a6_operands("grouped_matmul_mxf6_mxf4_bf16_tn", a, b, a_sf, b_sf, 3)
    return _ops_amd.grouped_matmul_mxf6_mxf4(a, b, a_sf, b_sf, alpha, offs)


def matmul_mxf6_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): the dense form of grouped_matmul_mxf6_mxf4_bf16_tn -- a (M, 3K/4) uint8 packed e2m3 against ONE MXFP4 weight b
    (N, K/2), flat row-major e8m0 scales, alpha float32 with one element.  The grouped op with E = 1, as matmul_mxf8_mxf4_bf16_tn is."""
    _check_w4a6_operands("matmul_mxf6_mxf4_bf16_tn", a, b, a_sf, b_sf, 2)
    offs = torch.full((1,), a.size(0), dtype=torch.int32, device=a.device)
    return _ops_amd.grouped_matmul_mxf6_mxf4(a, b.unsqueeze(0), a_sf, b_sf, alpha, offs)


def _check_w4a16_operands(op: str, a: torch.Tensor, b: torch.Tensor, b_sf: torch.Tensor, b_dim: int, src_row: torch.Tensor | None = None) -> None:
    """the rejections of the W4A16 ops that need no device: raised before the op is dispatched (shapes and dtypes only, so tracing goes through them)"""
    if a.dtype != torch.bfloat16:
        raise ValueError(f"{op}: a must be bfloat16 (got {a.dtype}; quantized tokens go to grouped_matmul_mxf8_mxf4_bf16_tn / grouped_matmul_mxf4_bf16_tn)")
    if b.dtype not in (torch.uint8, torch.float4_e2m1fn_x2):
        raise ValueError(f"{op}: b must be uint8 or float4_e2m1fn_x2 packed e2m1 (got {b.dtype})")
    if a.dim() != 2 or b.dim() != b_dim:
        raise ValueError(f"{op}: a must be 2D ({'T' if src_row is not None else 'M'}, K) and b {b_dim}D ({'E, ' if b_dim == 3 else ''}N, K/2)")
    if a.size(1) != 2 * b.size(-1):
        raise ValueError(f"{op}: inner dimensions must match, a is (.., K = {a.size(1)}) and b (.., K/2 = {b.size(-1)})")
    if b_sf.dtype != torch.float8_e8m0fnu:
        raise ValueError(f"{op}: b_sf must be float8_e8m0fnu (got {b_sf.dtype})")
    need = b.numel() // max(b.size(-1), 1) * (a.size(1) // 32)
    if b_sf.numel() < need:
        raise ValueError(f"{op}: b_sf has {b_sf.numel()} elements, the row-major scale layout needs {need}")
    if src_row is not None and (src_row.dtype != torch.int32 or src_row.dim() != 1):
        raise ValueError(f"{op}: src_row must be a 1D int32 tensor (got {src_row.dtype}, {src_row.dim()}D)")


def grouped_matmul_bf16_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, b_sf: torch.Tensor, alpha: torch.Tensor, offs: torch.Tensor, *,
                                     src_row: torch.Tensor | None = None) -> torch.Tensor:
    """EXTENSION (no reference counterpart): grouped W4A16 GEMM for mixture-of-experts layers -- bf16 tokens, unquantized, against MXFP4 expert weights as a
    checkpoint stores them (gpt-oss; every weight fusedQuantizeMx writes), one launch over all experts.  No quantizer runs in front of it.

    a        (M, K) bfloat16 -- the tokens, sorted by expert; with src_row: the UNSORTED (T, K) tokens
    b        (E, N, K/2) uint8 / float4_e2m1fn_x2 -- the stacked expert weights: what grouped_matmul_mxf4_bf16_tn reads
    b_sf     float8_e8m0fnu, >= E*N*K/32 elements, read as row-major (E, N, K/32)
    alpha    float32, 1 element (shared) or E elements (per expert)
    offs     int32 (E,): the cumulative END rows of the groups (torch._grouped_mm's convention) -- group g is rows [offs[g-1], offs[g]), offs[-1] := 0
    src_row  optional int32 (M,): sorted row r reads a[src_row[r]] (moe_sort's / moe_route's src_row as it is) -- the gather of the routed tokens happens in
             the GEMM's own loads; an index outside [0, T) reads an all-zero token; T * K * 2 bytes below 2 GiB

    Returns out (M, N) bf16 with out[r, n] = bf16(alpha[g] * sum_k x[r, k] * w[g, n, k]), w = e2m1(code) * 2^(b_sf - 127) held as bf16: exact products, fp32
    sums, one fp32 multiply by alpha, one rounding.  w is exact under scale bytes 2 ... 252; byte 255 gives NaN in every output of that weight row for the rows
    of that expert; bytes 0, 1, 253, 254 are outside the exact contract (underflow / overflow to inf).  NaN and inf in the tokens propagate.  Empty groups are
    allowed; rows at or past offs[E-1] are not written; the offsets are read on the device (graph capture, torch.compile), each clamped to [0, M], a decreasing
    one is an empty group.  K % 128 == 0, N % 8 == 0, 1 <= E <= 1024; the token matrix and one expert's weight below 2 GiB.  M == 0 returns an empty output.

    Wave-owned 32x32 / 32x16 / 64x32 tiles only, as grouped_matmul_mxf8_mxf4_bf16_tn (README, DESIGN.md section 8 for where it loses)."""
    _check_w4a16_operands("grouped_matmul_bf16_mxf4_bf16_tn", a, b, b_sf, 3, src_row)
    return _ops_amd.grouped_matmul_bf16_mxf4_bf16_tn(a, b, b_sf, alpha, offs, src_row)


def matmul_bf16_mxf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, b_sf: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): the dense form of grouped_matmul_bf16_mxf4_bf16_tn -- a (M, K) bfloat16 against ONE MXFP4 weight b (N, K/2)
    uint8 / float4_e2m1fn_x2 with flat row-major e8m0 scales (N, K/32), alpha float32 with one element.  Returns (M, N) bf16.  The grouped op with E = 1: its offs
    is a one-element device tensor filled with M, so there is no host sync and no kernel of its own."""
    _check_w4a16_operands("matmul_bf16_mxf4_bf16_tn", a, b, b_sf, 2)
    offs = torch.full((1,), a.size(0), dtype=torch.int32, device=a.device)
    return _ops_amd.grouped_matmul_bf16_mxf4_bf16_tn(a, b.unsqueeze(0), b_sf, alpha, offs, None)


def grouped_matmul_nvf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                                alpha: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): grouped NVFP4 GEMM for mixture-of-experts layers, one launch over all experts.

    a      (M, K/2) uint8 or float4_e2m1fn_x2 -- the tokens, sorted by expert
    b      (E, N, K/2) uint8 or float4_e2m1fn_x2 -- the stacked expert weights
    a_sf   float8_e4m3fn, >= M*K/16 elements, read as ROW-MAJOR (M, K/16): fusedQuantizeNv's scale buffer as it is (no to_blocked)
    b_sf   float8_e4m3fn, >= E*N*K/16 elements, read as row-major (E, N, K/16)
    alpha  float32, 1 element (shared) or E elements (per expert: alpha[g] = 1 / (global_scale_a * global_scale_b[g]))
    offs   int32 (E,): the cumulative END rows of the groups (torch._grouped_mm's convention) -- group g is rows [offs[g-1], offs[g]), offs[-1] := 0

    Returns out (M, N) bf16 with out[r] = alpha[g] * (A_r . SFA_r) (B_g . SFB_g)^T for every row r of group g, in matmul_nvf4_bf16_tn's arithmetic (e2m1 x e4m3
    exact in f16, fp32 sums).  Empty groups are allowed; rows at or past offs[E-1] are not written (their contents are unspecified, as in torch._grouped_mm).
    The offsets are read on the device, so the call needs no host sync and works under graph capture and torch.compile; each offset is clamped to [0, M]
    and a decreasing one is an empty group.  K % 128 == 0, N % 8 == 0, 1 <= E <= 1024; the token matrix and one expert's weight below 2 GiB (the stack may
    exceed it).  M == 0 returns an empty output."""
    return _ops_amd.grouped_matmul_nvf4(a, b, a_sf, b_sf, alpha, offs)


def matmul_nvf4_bf16_tn(a: torch.Tensor, b: torch.Tensor, a_sf: torch.Tensor, b_sf: torch.Tensor,
                        alpha: torch.Tensor,
                        backend: Literal["cutlass", "flashinfer"] = "cutlass") -> torch.Tensor:
    """qutlass/__init__.py:89-131."""
    if backend == "cutlass":
        return qutlass_CUDA.matmul_nvf4_bf16_tn(a, b, a_sf, b_sf, alpha)
    elif backend == "flashinfer":
        raise ImportError(_FLASHINFER_MSG)
    else:
        raise ValueError(f"invalid backend {backend!r}; use 'cutlass' or 'flashinfer'")


def matmul_mxf8_bf16_tn(a: torch.Tensor, b: torch.Tensor, block_scale_a: torch.Tensor,
                        block_scale_b: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """qutlass/__init__.py:134-139."""
    return qutlass_CUDA.matmul_mxf8_bf16_tn(a, b, block_scale_a, block_scale_b, alpha)


def matmul_mxf8_bf16_nn(a: torch.Tensor, b: torch.Tensor, block_scale_a: torch.Tensor,
                        block_scale_b: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """qutlass/__init__.py:141-146 (A stored (K, M))."""
    return qutlass_CUDA.matmul_mxf8_bf16_nn(a, b, block_scale_a, block_scale_b, alpha)


def _method_code(method) -> int:
    if method not in _METHOD_CODE:
        raise ValueError(f"invalid method {method!r}, must be 'quest' or 'abs_max'")
    return _METHOD_CODE[method]


def _quantize(op: str, *args):
    """One op of the rotate + quantize family (a row of ops.QUANT_OPS or ops.QUANT_OPS_MXF6), args as the functional op ``qutlass_amd::<op>`` takes them.  Eager: allocate, then the in-place
    twin; under torch.compile: the functional op (see ops.py)."""
    if torch.compiler.is_compiling():
        return getattr(_ops_amd, op)(*args)
    return ops.run_quant(ops.QUANT_OPS[op] if op in ops.QUANT_OPS else ops.QUANT_OPS_MXF6[op], *args)


def _output(op: str, *args):
    """The same for every other op that fills results allocated here (a row of ops.OUTPUT_OPS)."""
    if torch.compiler.is_compiling():
        return getattr(_ops_amd, op)(*args)
    return ops.run_output(ops.OUTPUT_OPS[op], *args)


def fusedQuantizeMx(a: torch.Tensor, b: torch.Tensor, *, method: Literal["quest", "abs_max"] = "quest",
                    return_mask: bool = False):
    """qutlass/__init__.py:149-180: allocate packed e2m1 + (padded_rows, padded_cols) e8m0 [+ clip mask]
    and run the fused rotate+quantize kernel.  As in the reference the scale buffer is written flat
    (first numel/32 bytes) and its padding is left uninitialised.
    (The op calls go through `qutlass_amd::` twins of `_qutlass_C.fusedQuantizeMx*` -- same kernels, same checks: the reference's schemas hide the writes from
    torch.compile.  Eager: the in-place twin on tensors allocated here; under torch.compile: the functional form, see ops.py.)"""
    code = _method_code(method)
    if not return_mask:
        return _quantize("quantize_mx", a, b, code)
    if method != "quest":
        raise ValueError("return_mask is only supported for method 'quest'")
    return _output("quantize_mx_mask", a, b)


def fusedQuantizeNv(a: torch.Tensor, b: torch.Tensor, global_scale: torch.Tensor, *,
                    method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """qutlass/__init__.py:183-203."""
    return _quantize("quantize_nv", a, b, global_scale, _method_code(method))


def fusedQuantizeMxBlocked(a: torch.Tensor, b: torch.Tensor, *, method: Literal["quest", "abs_max"] = "quest") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): ``fusedQuantizeMx`` whose scales come out GEMM-ready -- the second tensor is
    byte for byte ``to_blocked(fusedQuantizeMx(a, b, method=method)[1])`` (flat, zero padded), written by the quantizer itself:
    one launch instead of two on the activation path (qutlass/__init__.py:149-180 + qutlass/utils.py:160-193)."""
    return _quantize("quantize_mx_blocked", a, b, _method_code(method))


def fusedQuantizeNvBlocked(a: torch.Tensor, b: torch.Tensor, global_scale: torch.Tensor, *,
                           method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeNv`` with the e4m3 scales written directly in the ``to_blocked`` layout (see fusedQuantizeMxBlocked)."""
    return _quantize("quantize_nv_blocked", a, b, global_scale, _method_code(method))


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    """EXTENSION (no reference counterpart): the activation of a gated MLP as one streaming HIP kernel.  x is (.., 2 I) bf16, contiguous, with
    gate = x[..., :I] and up = x[..., I:] (what a GEMM against stacked [W1; W3] returns); the result is (.., I) bf16,

        s = bf16(g / (1 + exp(-g)))  (correctly rounded: fp32 arithmetic, fp64 near a bf16 tie),   act = bf16(float(s) * float(u))

    i.e. what ``torch.nn.functional.silu(gate) * up`` computes in bf16.  I % 8 == 0; no size limit below 2^31 rows / columns."""
    return _output("silu_and_mul", x)


def _silu_mul_quantize(op: str, x, *args):
    if not torch.compiler.is_compiling() and x.size(-1) % 2:   # (a traced call leaves this to the op's own check)
        raise ValueError(f"the last dimension of x must be 2 * I (got {x.size(-1)})")
    return _quantize(op, x, *args)


def fusedSiluMulQuantizeMx(x: torch.Tensor, h: torch.Tensor, *, method: Literal["quest", "abs_max"] = "quest") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): ``fusedQuantizeMx(silu_and_mul(x), h, method=method)`` in ONE launch, byte for byte -- the quantizer reads gate and up
    itself and applies the activation in registers, so the (.., I) bf16 activation never goes through memory (4.5 B instead of 8.5 B moved per element).
    x is (.., 2 I) bf16, contiguous; I % max(R, 32) == 0 for the R x R rotation h.  Returns e2m1 (.., I/2) and e8m0 (padded_rows, padded_cols) exactly as
    fusedQuantizeMx does for a (.., I) tensor (scales flat in the first rows * I / 32 bytes, padding untouched).  x must stay below 2 GiB (the kernel addresses
    it with 32-bit offsets; larger inputs raise -- split them by rows).  Non-finite gate / up values give unspecified bytes in their own groups only.
    Measured faster than the two calls for R <= 32 (1.15-1.45x); at R = 128 it is not: keep silu_and_mul + fusedQuantizeMx there."""
    return _silu_mul_quantize("silu_mul_quantize_mx", x, h, _method_code(method), False)


def fusedSiluMulQuantizeMxBlocked(x: torch.Tensor, h: torch.Tensor, *, method: Literal["quest", "abs_max"] = "quest") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxBlocked(silu_and_mul(x), h, method=method)`` in one launch (see fusedSiluMulQuantizeMx): the scales come out flat in the
    ``to_blocked`` layout, zero padded -- what the dense ``matmul_mxf4_bf16_tn`` takes.  x below 2 GiB."""
    return _silu_mul_quantize("silu_mul_quantize_mx", x, h, _method_code(method), True)


def fusedSiluMulQuantizeNv(x: torch.Tensor, h: torch.Tensor, global_scale: torch.Tensor, *,
                           method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeNv(silu_and_mul(x), h, global_scale, method=method)`` in one launch, byte for byte (see fusedSiluMulQuantizeMx); R may be 16.
    x below 2 GiB."""
    return _silu_mul_quantize("silu_mul_quantize_nv", x, h, global_scale, _method_code(method), False)


def fusedSiluMulQuantizeNvBlocked(x: torch.Tensor, h: torch.Tensor, global_scale: torch.Tensor, *,
                                  method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeNvBlocked(silu_and_mul(x), h, global_scale, method=method)`` in one launch (see fusedSiluMulQuantizeMxBlocked).  x below 2 GiB."""
    return _silu_mul_quantize("silu_mul_quantize_nv", x, h, global_scale, _method_code(method), True)


def moe_sort(topk_ids: torch.Tensor, num_experts: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): the routing metadata of a mixture-of-experts layer from the router's (T, topk) integer expert ids.

    src_row  (T * topk,) int32 -- the token of every sorted row: rows are ordered by expert, and within an expert by (token, slot) (a stable sort)
    offs     (num_experts,) int32 -- the cumulative END rows of the experts, the grouped GEMMs' convention; dropped rows are not counted
    pos      (T, topk) int32 -- the sorted row of every routed slot, or -1 where the id was dropped

    An id outside [0, num_experts) is DROPPED (an expert that lives on another rank): its row sorts behind every real expert, past offs[-1], where the grouped
    GEMMs write nothing, and moe_combine skips its -1.  Plain torch ops without a host sync or a data-dependent shape (stable argsort, searchsorted, scatter): it
    runs under graph capture and torch.compile, and on CPU tensors.  Feed src_row to fusedGatherQuantize*, offs to grouped_matmul_*, pos to moe_combine."""
    if topk_ids.dim() != 2:
        raise ValueError(f"topk_ids must be (T, topk) (got {tuple(topk_ids.shape)})")
    topk = topk_ids.size(1)
    ids = topk_ids.reshape(-1).to(torch.int64)
    key = torch.where((ids >= 0) & (ids < num_experts), ids, num_experts)
    order = torch.argsort(key, stable=True)
    rows = torch.arange(ids.numel(), device=ids.device)
    offs = torch.searchsorted(key[order], torch.arange(num_experts, device=ids.device), right=True)
    pos = torch.empty_like(order).scatter_(0, order, rows)
    pos = torch.where(key < num_experts, pos, -1).view_as(topk_ids)
    return torch.div(order, topk, rounding_mode="floor").to(torch.int32), offs.to(torch.int32), pos.to(torch.int32)


def moe_topk_softmax(logits: torch.Tensor, topk: int, *, renormalize: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): the router's (T, E) logits -> (weights (T, topk) float32, ids (T, topk) int32) in ONE HIP launch, one wave per token.

    Selection is exact and part of the contract: the first topk experts in the order (logit descending, expert index ascending), ids[t] in that order.  Logits
    compare as floating-point numbers (-0.0 and +0.0 tie; the lower index wins); the choice is made on the logits, never on the probabilities (exp can merge two
    logits).  -inf is a legal logit (a masked expert): probability 0, sorts last.  Weights in fp32: m = max_j x_j, e_j = exp(x_j - m), p_j = e_j / sum_j e_j, and
    with renormalize w_k = p_k / sum over the selected p (the order of the sums is the kernel's business).  A token whose row holds a NaN or +inf, or nothing but
    -inf, gets unspecified weights; its ids are still distinct and inside [0, E), and no other token is affected.

    logits bf16 or float32, contiguous; 1 <= E <= 1024 (the grouped GEMMs' limit), 1 <= topk <= min(E, 32) (moe_combine's limit); T == 0 returns empty tensors.  No
    host sync, no workspace: graph-capturable.  ids feed moe_sort / moe_sort_fused, weights and ids feed moe_combine, as they are."""
    if logits.dim() != 2:
        raise ValueError(f"logits must be (T, E) (got {tuple(logits.shape)})")
    if not 1 <= topk <= min(logits.size(1), 32):
        raise ValueError(f"topk must be in [1, min(E, 32)] (got topk = {topk} for E = {logits.size(1)})")
    return _output("moe_topk_softmax", logits, topk, renormalize)


def moe_sort_fused(topk_ids: torch.Tensor, num_experts: int, *, expert_map: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): ``moe_sort(topk_ids, num_experts)`` -- the same three int32 results, bit for bit -- as a counting sort in HIP: one launch
    of one workgroup up to the one-launch bound of T * topk slots, three launches (count, scan, scatter) over scratch allocated here beyond it.  No atomics and no
    workgroup waiting on another: the result does not depend on the launch geometry or on timing.  topk_ids (T, topk) int32 or int64 on the device; 1 <=
    num_experts <= 1024; T * topk < 2^31.

    expert_map (G,) int32, G >= 1, for expert parallelism: an id g in [0, G) is replaced by expert_map[g] before anything else; a value outside [0, num_experts)
    (conventionally -1, "not on this rank") drops the slot, and an id outside [0, G) is dropped without reading the map.  Dropped slots sort behind every real
    expert with pos = -1 and are not counted in offs, as in moe_sort.  No host sync: graph-capturable; traces under torch.compile."""
    if topk_ids.dim() != 2:
        raise ValueError(f"topk_ids must be (T, topk) (got {tuple(topk_ids.shape)})")
    return _output("moe_sort_fused", topk_ids, expert_map, num_experts)


def moe_route(logits: torch.Tensor, topk: int, num_experts: int | None = None, *, renormalize: bool = True,
              expert_map: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """EXTENSION: the whole routing of a mixture-of-experts layer from the router's logits: ``moe_topk_softmax`` then ``moe_sort_fused`` -- two launches for decode-sized
    inputs.  Returns (weights, ids, src_row, offs, pos).  num_experts defaults to E, the logits' second dimension; with expert_map pass the number of LOCAL experts."""
    weights, ids = moe_topk_softmax(logits, topk, renormalize=renormalize)
    return (weights, ids) + tuple(moe_sort_fused(ids, logits.size(1) if num_experts is None else num_experts, expert_map=expert_map))


def _check_grouped(logits, topk, n_group, topk_group, bias, scoring):
    if logits.dim() != 2:
        raise ValueError(f"logits must be (T, E) (got {tuple(logits.shape)})")
    E = logits.size(1)
    if scoring not in _lib.MOE_SCORING:
        raise ValueError(f"scoring must be 'sigmoid' or 'softmax' (got {scoring!r})")
    if not 1 <= E <= 1024:
        raise ValueError(f"the number of experts must be in [1, 1024] (got {E})")
    if not 1 <= n_group <= 64:
        raise ValueError(f"n_group must be in [1, 64] (got {n_group})")
    if E % n_group != 0:
        raise ValueError(f"n_group must divide E (got n_group = {n_group} for E = {E})")
    if not 1 <= topk_group <= n_group:
        raise ValueError(f"topk_group must be in [1, n_group] (got {topk_group} for n_group = {n_group})")
    if not 1 <= topk <= min(32, topk_group * (E // n_group)):
        raise ValueError(f"topk must be in [1, min(32, topk_group * E / n_group)] (got topk = {topk} for E = {E}, n_group = {n_group}, topk_group = {topk_group})")
    if bias is not None and (bias.dim() != 1 or bias.size(0) != E or bias.dtype != torch.float32):
        raise ValueError(f"bias must be a float32 tensor of (E,) = ({E},) (got {bias.dtype} {tuple(bias.shape)})")


def moe_topk_grouped(logits: torch.Tensor, topk: int, *, n_group: int = 1, topk_group: int = 1, bias: torch.Tensor | None = None, scoring: str = "sigmoid",
                     renormalize: bool = True, routed_scaling_factor: float = 1.0, return_scores: bool = False):
    """EXTENSION (no reference counterpart): the grouped router of DeepSeek-V3 / R1 (E 256, sigmoid, bias, top-8 of the top-4 of 8 groups, x 2.5), Kimi-K2 (E 384,
    one group, x 2.827) and DeepSeek-V2 (softmax, 8 groups of 20, no bias) in ONE HIP launch: (T, E) logits -> (weights (T, topk) float32, ids (T, topk) int32),
    and with return_scores a third result, scores (T, E) float32.  All arithmetic is fp32; G = n_group, S = E / G.

      scores     "sigmoid": s_j = 1 / (1 + exp(-x_j)) (-inf gives 0, +inf gives 1); "softmax": moe_topk_softmax's p_j.  The order of the sum is free.
      choice     c_j = s_j + bias_j (one fp32 add) with a bias -- (E,) float32, every entry finite or -inf --, else c_j = s_j.  c alone decides what is selected;
                 the bias never reaches a weight.
      groups     (G > 1) group g = experts [g S, (g + 1) S); its score is the sum of its two largest c with a bias (one fp32 add; one expert: that value), its
                 largest c without.  The first topk_group groups in (score descending, group index ascending) survive; experts of the other groups are not
                 candidates, whatever the sign of c (vLLM's -inf mask, not the zero fill of the Hugging Face model code).
      selection  the first topk candidates in (c descending, expert index ascending), ids[t] in that order; -0 ties with +0.
      weights    w_k = s_{id_k}, the UNBIASED score; renormalize: divided by their sum (a sum of 0 gives unspecified weights); last multiplied by
                 routed_scaling_factor (one fp32 multiply).
      scores     the s_j the kernel selected on, bit for bit (balance losses and the bias update of auxiliary-loss-free balancing need them; every choice can be
                 repeated exactly from them).  Asking for them changes no bit of ids or weights.

    Selection runs on c, NOT on the logits: this differs on purpose from moe_topk_softmax, where there is no bias and selecting on the logits is exact -- here a
    bias reorders the experts, and two logits that round to one score tie (the lower index wins).  A row holding a NaN (or a +inf + -inf in c or a group score) gets
    unspecified weights; its ids are still distinct and inside [0, E), and no other row is affected.

    logits bf16 or float32, contiguous; 1 <= E <= 1024, 1 <= n_group <= 64, E % n_group == 0, 1 <= topk_group <= n_group, 1 <= topk <= min(32, topk_group * S);
    T == 0 returns empty tensors.  No host sync, no workspace: graph-capturable; traces under torch.compile."""
    _check_grouped(logits, topk, n_group, topk_group, bias, scoring)
    weights, ids, scores = _output("moe_topk_grouped", logits, bias, topk, n_group, topk_group, _lib.MOE_SCORING[scoring], renormalize, float(routed_scaling_factor),
                                   return_scores)
    return (weights, ids, scores) if return_scores else (weights, ids)


def moe_route_grouped(logits: torch.Tensor, topk: int, num_experts: int | None = None, *, n_group: int = 1, topk_group: int = 1, bias: torch.Tensor | None = None,
                      scoring: str = "sigmoid", renormalize: bool = True, routed_scaling_factor: float = 1.0,
                      expert_map: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """EXTENSION: ``moe_route`` with the grouped router in front: ``moe_topk_grouped`` then ``moe_sort_fused`` -- two launches for decode-sized inputs.  Returns
    (weights, ids, src_row, offs, pos), what moe_route returns.  num_experts defaults to E; with expert_map pass the number of LOCAL experts."""
    weights, ids = moe_topk_grouped(logits, topk, n_group=n_group, topk_group=topk_group, bias=bias, scoring=scoring, renormalize=renormalize,
                                    routed_scaling_factor=routed_scaling_factor)
    return (weights, ids) + tuple(moe_sort_fused(ids, logits.size(1) if num_experts is None else num_experts, expert_map=expert_map))


def _check_expert_map(expert_map):
    if expert_map is not None and expert_map.numel() == 0:
        raise ValueError("expert_map must have at least one entry")


def moe_route_fused(logits: torch.Tensor, topk: int, num_experts: int | None = None, *, renormalize: bool = True,
                    expert_map: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """EXTENSION: ``moe_route(logits, topk, num_experts, renormalize=renormalize, expert_map=expert_map)`` -- the same five results (weights, ids, src_row, offs, pos),
    bit for bit -- in ONE launch for decode batches: up to ``qutlass_amd_moe_route_fused_max_tokens()`` tokens (a measured bound, at most 64) one workgroup routes its
    tokens, a wave per token, and sorts the T * topk slots it has just produced, their keys handed over in LDS; the kernel runs moe_topk_softmax's and moe_sort_fused's
    own device code.  Beyond the bound the op runs those two, so it takes every T.  The same limits and ValueErrors as moe_route; T == 0 returns empty tensors and an
    all-zero offs.  A functional op that allocates its results without a fill -- one graph node up to the bound -- (``torch.ops.qutlass_amd.moe_route_fused``): no host sync, graph-capturable, traces under
    torch.compile."""
    if logits.dim() != 2:
        raise ValueError(f"logits must be (T, E) (got {tuple(logits.shape)})")
    if not 1 <= topk <= min(logits.size(1), 32):
        raise ValueError(f"topk must be in [1, min(E, 32)] (got topk = {topk} for E = {logits.size(1)})")
    _check_expert_map(expert_map)
    return _ops_amd.moe_route_fused(logits, expert_map, topk, logits.size(1) if num_experts is None else num_experts, renormalize)


def moe_route_grouped_fused(logits: torch.Tensor, topk: int, num_experts: int | None = None, *, n_group: int = 1, topk_group: int = 1, bias: torch.Tensor | None = None,
                            scoring: str = "sigmoid", renormalize: bool = True, routed_scaling_factor: float = 1.0,
                            expert_map: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """EXTENSION: ``moe_route_grouped`` with the same arguments and the same five results, bit for bit, in ONE launch for decode batches -- moe_route_fused with the
    grouped router (moe_topk_grouped's device code) in front; the two-launch form beyond the same measured bound."""
    _check_grouped(logits, topk, n_group, topk_group, bias, scoring)
    _check_expert_map(expert_map)
    return _ops_amd.moe_route_grouped_fused(logits, bias, expert_map, topk, logits.size(1) if num_experts is None else num_experts, n_group, topk_group,
                                            _lib.MOE_SCORING[scoring], renormalize, float(routed_scaling_factor))


def fusedGatherQuantizeMx(x: torch.Tensor, h: torch.Tensor, src_row: torch.Tensor, *,
                          method: Literal["quest", "abs_max"] = "quest") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): ``fusedQuantizeMx(x.index_select(0, src_row), h, method=method)`` in ONE launch, byte for byte -- the MoE dispatch: the
    quantizer reads every routed row through the index, so the (M, K) bf16 copy of the tokens is never written (about 2.5 B moved per routed element instead of 6.5).
    x is (T, K) bf16, contiguous; src_row is (M,) int32 on the device (moe_sort's first result); K % max(R, 32) == 0 for the R x R rotation h.  Returns e2m1 (M, K/2)
    and e8m0 (padded_rows, padded_cols) exactly as fusedQuantizeMx does for an (M, K) tensor: scales flat in the first M * K / 32 bytes, padding untouched -- what
    grouped_matmul_mxf4_bf16_tn reads as it is.  The indices are read on the device (no host sync: graph-capturable); an index outside [0, T) -- -1 padding included --
    gives the bytes of an all-zero row and can neither fault nor read another row.  x must stay below 2 GiB (32-bit offsets; larger inputs raise).
    Speed against index_select + fusedQuantizeMx: not measured yet (benchmarks/bench_moe_dispatch_mi355x.py)."""
    return _quantize("gather_quantize_mx", x, h, src_row, _method_code(method))


def fusedGatherQuantizeNv(x: torch.Tensor, h: torch.Tensor, global_scale: torch.Tensor, src_row: torch.Tensor, *,
                          method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeNv(x.index_select(0, src_row), h, global_scale, method=method)`` in one launch, byte for byte (see fusedGatherQuantizeMx); R may be
    16; e4m3 scales flat in the first M * K / 16 bytes -- what grouped_matmul_nvf4_bf16_tn reads as it is.  x below 2 GiB."""
    return _quantize("gather_quantize_nv", x, h, src_row, global_scale, _method_code(method))


def fusedGatherQuantizeNvGrouped(x: torch.Tensor, h: torch.Tensor, global_scales: torch.Tensor, src_row: torch.Tensor, offs: torch.Tensor, *,
                                 method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): ``fusedGatherQuantizeNv`` with ONE GLOBAL SCALE PER EXPERT, in one launch -- the A operand that
    grouped_matmul_nvf4_bf16_tn's per-expert alpha (alpha[g] = 1 / (a_gs[g] * w_gs[g])) expects, for checkpoints that carry an activation scale per expert.

    global_scales  (E,) float32 on the device;  offs  (E,) int32 on the device: the grouped GEMMs' cumulative END rows (moe_sort's / moe_sort_fused's second result);
    1 <= E <= 1024.  The expert of sorted row m is g(m) = min(E - 1, #{g : offs[g] <= m}): the group the grouped GEMM puts the row in; rows at or past offs[-1] (the
    dropped slots, which the GEMM never reads) take expert E - 1's scale, so every byte is defined.

    The bytes of row m, codes and e4m3 scales, are those of ``fusedGatherQuantizeNv(x, h, global_scales[g(m):g(m)+1], src_row, method=method)``; everything else is that
    function's: flat scales in the first M * K / 16 bytes with the padding untouched, an all-zero row for an index outside [0, T), x below 2 GiB.  method "quest" reads
    no global scale: the result is fusedGatherQuantizeNv's.  offs is read on the device (no host sync, no workspace: graph-capturable; traces under torch.compile);
    malformed offs (negative, above M, decreasing) cannot fault -- every row is then quantized with the scale of SOME expert in [0, E), which one is unspecified.
    Cost against the single-scale op: DESIGN.md section 10."""
    return _quantize("gather_quantize_nv_grouped", x, h, src_row, global_scales, offs, _method_code(method))


def fusedSiluMulQuantizeNvGrouped(x: torch.Tensor, h: torch.Tensor, global_scales: torch.Tensor, offs: torch.Tensor, *,
                                  method: Literal["quest", "abs_max"] = "abs_max") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedSiluMulQuantizeNv`` with one global scale per expert (see fusedGatherQuantizeNvGrouped): row m of act = silu(gate) * up, x = (M, 2 I) the sorted
    rows a grouped gate/up GEMM returned, is quantized with global_scales[g(m)], g(m) from offs (E,) int32 -- the down projection's A operand.  The bytes of row m are
    those of ``fusedSiluMulQuantizeNv(x, h, global_scales[g(m):g(m)+1], method=method)``; flat scales only (what grouped_matmul_nvf4_bf16_tn reads as it is); x below 2 GiB."""
    return _silu_mul_quantize("silu_mul_quantize_nv_grouped", x, h, global_scales, offs, _method_code(method))


def fusedQuantizeMxf8(a: torch.Tensor, h: torch.Tensor, *, dtype: torch.dtype = torch.float8_e4m3fn) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION (no reference counterpart): rotate and quantize to MXFP8 -- the operand the three MXFP8 GEMMs take, made on the device.  a is (.., K) bf16, h a
    runtime R x R bf16 matrix, R in {32, 64, 128} (no 16: the scale group is 32); K % R == 0.  y = a_group @ h exactly as fusedQuantizeMx computes it (the
    identity matrix gives a plain quantizer); then for every 32 consecutive y

        amax = max |y| (NaNs ignored);  E = the biased exponent field of the fp32 amax;  SH = 7 for float8_e4m3fn, 14 for float8_e5m2
        scale byte  e8 = 127 if amax == 0 else clamp(E - SH, 0, 254)       (the scaled maximum lies in [128, 256) / [2^14, 2^15): no finite input saturates)
        code        q = RNE(y * 2^(127 - e8)) in dtype                      (the scaling is exact; -0 keeps its sign)

    -- the rule of the reference's e8m0_shift7 and of oracle.pseudoquant_mxfp8 (without the latter's bf16-log2 rounding of the exponent).  Abs-max only (Quest's
    constant is an FP4 constant); no clip mask, no global scale.  Returns codes, a's shape in dtype, and float8_e8m0fnu scales allocated (padded_rows, padded_cols) and
    written flat in the first numel / 32 bytes, padding untouched, exactly as fusedQuantizeMx's: what grouped_matmul_mxf8_bf16_tn reads as it is.  A NaN input
    gives NaN codes throughout its own rotation block, the bytes of a block that holds +-inf are unspecified; no other block is affected.  Fewer than 2^31 elements."""
    return _quantize("quantize_mxf8", a, h, ops.mxf8_dtype(dtype))


def fusedQuantizeMxf8Blocked(a: torch.Tensor, h: torch.Tensor, *, dtype: torch.dtype = torch.float8_e4m3fn) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxf8`` whose scales come out GEMM-ready -- the second tensor is byte for byte ``to_blocked(fusedQuantizeMxf8(a, h, dtype=dtype)[1])``
    (flat, zero padded), written by the quantizer itself: what the dense ``matmul_mxf8_bf16_tn`` takes.  K % R == 0 for the last dimension K."""
    return _quantize("quantize_mxf8_blocked", a, h, ops.mxf8_dtype(dtype))


def fusedGatherQuantizeMxf8(x: torch.Tensor, h: torch.Tensor, src_row: torch.Tensor, *, dtype: torch.dtype = torch.float8_e4m3fn) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxf8(x.index_select(0, src_row), h, dtype=dtype)`` in ONE launch, byte for byte -- the MXFP8 MoE dispatch (float8_e5m2: the dgrad token
    path of grouped_matmul_mxf8_bf16_tn).  x is (T, K) bf16, contiguous, src_row (M,) int32 on the device, K % R == 0; codes (M, K), flat scales.  An index outside
    [0, T) gives a zero row (codes 0, scale 127) and can neither fault nor read another row; the indices are read on the device (graph-capturable).  x below 2 GiB.
    Measured 1.2-2.4x faster than index_select + fusedQuantizeMxf8 at every shape taken."""
    return _quantize("gather_quantize_mxf8", x, h, src_row, ops.mxf8_dtype(dtype))


def fusedQuantizeMxf6(a: torch.Tensor, h: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: rotate + quantize to MXFP6 -- e2m3 codes, four in three bytes, with one e8m0 scale per 32 elements: the A operand of
    grouped_matmul_mxf6_mxf4_bf16_tn.  y = a_group @ h as in fusedQuantizeMxf8 (h: R x R bf16, R in {32, 64, 128}; the identity gives a plain quantizer), then per 32
    consecutive y: e8 = 255 if any is NaN or infinite (all 32 codes 0 -- the format has no NaN code, the scale byte carries it), 127 if amax == 0, else
    clamp(E - 2, 0, 254) with E the exponent field of the fp32 amax (the OCP MX rule: the scaled maximum lies in [4, 8)); q = min(RNE(|y| 2^(127 - e8)), 7.5) with
    the sign of y, ties to the even code, (7.5, 8) saturating on purpose, -0 keeping its sign.  Returns uint8 codes (.., 3K/4) -- element k in bits 6k .. 6k+5 of
    the row read little-endian -- and float8_e8m0fnu scales (padded_rows, padded_cols), written flat in the first numel / 32 bytes as fusedQuantizeMx's."""
    return _quantize("quantize_mxf6", a, h)


def fusedGatherQuantizeMxf6(x: torch.Tensor, h: torch.Tensor, src_row: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxf6(x.index_select(0, src_row), h)`` in ONE launch, byte for byte -- the MXFP6 MoE dispatch.  x is (T, K) bf16, contiguous and
    below 2 GiB, src_row (M,) int32 on the device, K % R == 0; codes (M, 3K/4), flat scales.  An index outside [0, T) gives a zero row: codes 0, scale byte 127."""
    return _quantize("gather_quantize_mxf6", x, h, src_row)


def fusedSiluMulQuantizeMxf8(x: torch.Tensor, h: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxf8(silu_and_mul(x), h)`` in ONE launch, byte for byte (see fusedSiluMulQuantizeMx): x is (.., 2 I) bf16 [gate | up], I % R == 0;
    float8_e4m3fn codes (.., I) and flat scales -- the down projection's A operand for grouped_matmul_mxf8_bf16_tn.  e4m3 only: a forward activation has no use for
    e5m2.  x below 2 GiB.  Measured faster than the two calls at R = 32 (1.17-1.46x); at R = 128 it is NOT -- 0.50-0.72x at decode shapes, 0.94-1.08x at prefill
    (as for fusedSiluMulQuantizeMx): keep silu_and_mul + fusedQuantizeMxf8 there."""
    return _silu_mul_quantize("silu_mul_quantize_mxf8", x, h, torch.float8_e4m3fn, False)


def fusedSiluMulQuantizeMxf8Blocked(x: torch.Tensor, h: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxf8Blocked(silu_and_mul(x), h)`` in one launch (see fusedSiluMulQuantizeMxf8): the scales come out flat in the ``to_blocked`` layout,
    zero padded -- what the dense ``matmul_mxf8_bf16_tn`` takes.  x below 2 GiB.  Slower than its two-launch composition at R = 128, like the flat form."""
    return _silu_mul_quantize("silu_mul_quantize_mxf8", x, h, torch.float8_e4m3fn, True)


def _bf16_exact(v: float) -> bool:
    import struct

    try:
        return struct.unpack("<I", struct.pack("<f", v))[0] & 0xffff == 0
    except OverflowError:
        return False


def _check_swiglu_oai(x, alpha, limit, bias, offs, rot=None, op="fusedSwigluOaiQuantizeMx", plain="fusedQuantizeMx"):
    """The Python-level checks of the clamped-SwiGLU ops (a traced call leaves the shapes to the op's own checks); op / plain: the fused op and the plain quantizer
    its R = 128 message names."""
    import math

    if torch.compiler.is_compiling():   # (the C entry repeats the value checks)
        return float(alpha), float(limit)
    alpha, limit = float(alpha), float(limit)
    if not (math.isfinite(alpha) and alpha > 0):
        raise ValueError(f"alpha must be finite and > 0 (got {alpha})")
    if not (math.isfinite(limit) and limit > 0 and _bf16_exact(limit)):
        raise ValueError(f"limit must be > 0, finite and exactly representable in bf16 (got {limit})")
    if rot == 128:
        raise ValueError(f"rotation size 128 is not supported by {op} (R = 32 or 64): use swiglu_oai_and_mul followed by {plain}")
    if x.size(-1) % 2:
        raise ValueError(f"the last dimension of x must be 2 * I (got {x.size(-1)})")
    if bias is None:
        if offs is not None:
            raise ValueError("offs without a bias")
    else:
        if bias.dim() != 2 or bias.size(1) != x.size(-1):
            raise ValueError(f"bias must be (E, 2 * I) = (E, {x.size(-1)}) (got {tuple(bias.shape)})")
        _check_bias_offs(bias, offs)
    return alpha, limit


def _check_bias_offs(bias, offs):
    E = bias.size(0)
    if not 1 <= E <= 1024:
        raise ValueError(f"the number of experts must be in [1, 1024] (got {E})")
    if offs is None:
        if E > 1:
            raise ValueError(f"a bias of E = {E} experts needs offs")
    elif offs.dim() != 1 or offs.size(0) != E or offs.dtype != torch.int32:
        raise ValueError(f"offs must be an int32 tensor of (E,) = ({E},) (got {offs.dtype} {tuple(offs.shape)})")


def swiglu_oai_and_mul(x: torch.Tensor, *, alpha: float = 1.702, limit: float = 7.0, bias: torch.Tensor | None = None,
                       offs: torch.Tensor | None = None) -> torch.Tensor:
    """EXTENSION (no reference counterpart): the activation of a gpt-oss expert, the clamped SwiGLU, as one streaming HIP kernel -- with the gate/up bias of the row's
    expert added on the way in.  x is (.., 2 I) bf16, contiguous, with gate = x[..., :I] and up = x[..., I:] (gpt-oss stores the columns interleaved:
    utils.split_interleaved_gate_up, once at load time); the result is (.., I) bf16.  Per element, g, u, bg, bu bf16:

        g1 = bf16(float(g) + float(bg)),  u1 = bf16(float(u) + float(bu))     with a bias (one fp32 add, then RNE: torch's bf16 add); else g1 = g, u1 = u
        gc = min(g1, limit);   uc = min(max(u1, -limit), limit)                (exact)
        s  = bf16 of the REAL number gc / (1 + exp(-alpha * gc)), CORRECTLY rounded (alpha the fp32 value, the product not rounded: fp32 arithmetic, fp64 near a
             bf16 tie and for |alpha * gc| > 16)
        act = bf16(float(s) * (float(uc) + 1.0f))                              (one fp32 add, one fp32 multiply, no fma, then RNE)

    Deliberately NOT bit-equal to the reference model's bf16 op chain (which rounds alpha * gate, the sigmoid, up + 1 and both products separately): fewer
    roundings, closer to the exact function.  For gates with |gc| < 2^-120 the true s lies within 2^-130 (relative) of a tie between bf16 subnormals; s is then
    within one bf16 step, and no more is promised.  NaN / +-inf in gate, up or bias give unspecified bytes for their own element.  A zero gate, up and bias give +0,
    so zero-padded columns are harmless: gpt-oss's H = I = 2880 is no multiple of 128 -- pad K to 2944 with zero weight rows and zero bias.

    bias (E, 2 I) bf16 in the same [gate | up] halves, 1 <= E <= 1024; offs (E,) int32 on the device, the grouped GEMMs' cumulative END rows -- required for E > 1,
    optional for E == 1.  With a bias x is read as (rows, 2 I) SORTED rows: row r takes bias[g(r)], g(r) = min(E - 1, #{g : offs[g] <= r}), the group the grouped GEMM
    put the row in; rows at or past offs[-1] take expert E - 1's bias.  Malformed offs select SOME expert in [0, E) and cannot address outside bias.  offs is read
    on the device (no host sync: graph-capturable).  I % 8 == 0; alpha finite and > 0; limit > 0, finite and a bf16 value -- ValueError otherwise.
    Measured 4.5-5.4x faster (with fusedQuantizeMx behind it) than the torch composition of bias add, clamp, sigmoid and multiply (README;
    profiles/bench_swiglu_oai_mi355x.txt)."""
    alpha, limit = _check_swiglu_oai(x, alpha, limit, bias, offs)
    return _output("swiglu_oai_and_mul", x, alpha, limit, bias, offs)


def fusedSwigluOaiQuantizeMx(x: torch.Tensor, h: torch.Tensor, *, alpha: float = 1.702, limit: float = 7.0, bias: torch.Tensor | None = None,
                             offs: torch.Tensor | None = None, method: Literal["quest", "abs_max"] = "quest") -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMx(swiglu_oai_and_mul(x, alpha=alpha, limit=limit, bias=bias, offs=offs), h, method=method)`` in ONE launch, byte for byte -- the
    down projection's A operand of a gpt-oss layer: the quantizer reads gate, up and the two bias chunks of the row's expert itself and applies the activation in
    registers (see swiglu_oai_and_mul for the arithmetic and fusedSiluMulQuantizeMx for the form).  Returns e2m1 (.., I/2) and e8m0 (padded_rows, padded_cols) as
    fusedQuantizeMx does for a (.., I) tensor: scales flat in the first rows * I / 32 bytes, padding untouched -- what grouped_matmul_mxf4_bf16_tn reads as it is.
    R in {32, 64} for the R x R rotation h (I = 2880 admits no 128, and the gated kernels at R = 128 are slower than their two launches: R = 128 raises -- use
    swiglu_oai_and_mul followed by fusedQuantizeMx); I % R == 0; both methods; no clip mask, no blocked form.  x, and bias, below 2 GiB.  Non-finite gate / up /
    bias values give unspecified bytes in their own rotation groups only.
    Measured against the two calls (gpt-oss shapes, I = 2944, with bias; profiles/bench_swiglu_oai_mi355x.txt): R = 32 wins from 128 tokens x top-4 on (1.14-1.23x)
    and is level to SLOWER at 16 tokens (0.95-1.01x); at R = 64 it is SLOWER up to 128 tokens (0.67-0.69x at 16, 0.94-0.96x at 128) and wins only at prefill sizes
    (1.12-1.13x at 4096 tokens): keep swiglu_oai_and_mul + fusedQuantizeMx for R = 64 at decode sizes.  4.6-6.6x (R = 32) faster than the torch composition."""
    code = _method_code(method)
    alpha, limit = _check_swiglu_oai(x, alpha, limit, bias, offs, h.size(0) if h.dim() == 2 else None)
    return _quantize("swiglu_oai_quantize_mx", x, h, alpha, limit, bias, offs, code)


def fusedSwigluOaiQuantizeMxf8(x: torch.Tensor, h: torch.Tensor, *, alpha: float = 1.702, limit: float = 7.0, bias: torch.Tensor | None = None,
                               offs: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION: ``fusedQuantizeMxf8(swiglu_oai_and_mul(x, alpha=alpha, limit=limit, bias=bias, offs=offs), h)`` in ONE launch, byte for byte -- the down
    projection's A operand of a gpt-oss W4A8 layer (grouped_matmul_mxf8_mxf4_bf16_tn: MXFP4 expert weights as stored against 8-bit tokens): fusedSwigluOaiQuantizeMx
    with the MXFP8 epilogue (see swiglu_oai_and_mul for the arithmetic, fusedQuantizeMxf8 for the scale rule).  The (.., I) bf16 activation never goes through memory:
    5 B moved per element instead of 8.5.  Returns float8_e4m3fn codes (.., I) and float8_e8m0fnu scales (padded_rows, padded_cols) as fusedQuantizeMxf8 does for a
    (.., I) tensor: scales flat in the first rows * I / 32 bytes, padding untouched.  e4m3 only (a forward activation has no use for e5m2); abs-max only.
    R in {32, 64} for the R x R rotation h (R = 128 raises -- use swiglu_oai_and_mul followed by fusedQuantizeMxf8); I % R == 0; no blocked form.  bias (E, 2 I) bf16
    and offs (E,) int32 as in swiglu_oai_and_mul; malformed offs select some expert in [0, E).  x, and bias, below 2 GiB.  Non-finite gate / up / bias values give
    unspecified bytes in their own rotation groups only.  No host sync: graph-capturable; traces under torch.compile.
    Measured against the two launches (gpt-oss shapes, I = 2944, with bias, tokens x top-4; profiles/bench_swiglu_oai_mxf8_mi355x.txt): R = 32 wins from 128 tokens
    on (1.08-1.17x; 1.26-1.28x at 4096 tokens, 78-80 against 100-102 us) and is level to SLOWER at 16 tokens (0.94-0.99x, 6.5-7.0 against 6.2-6.6 us); at R = 64 it is
    SLOWER up to 128 tokens (0.67-0.69x at 16, 10.0-10.5 against 6.7-7.1 us; 0.91-0.95x at 128, 9.8-11.1 against 9.3-10.3 us) and wins only at prefill sizes
    (1.15-1.17x at 4096 tokens): keep swiglu_oai_and_mul + fusedQuantizeMxf8 for R = 64 at decode sizes.  4.5-7.0x (R = 32) faster than the torch composition; as
    fast as fusedSwigluOaiQuantizeMx on the same input (0.99-1.02x: the kernel is bound by the activation's vector work, not by the code bytes)."""
    alpha, limit = _check_swiglu_oai(x, alpha, limit, bias, offs, h.size(0) if h.dim() == 2 else None, "fusedSwigluOaiQuantizeMxf8", "fusedQuantizeMxf8")
    return _quantize("swiglu_oai_quantize_mxf8", x, h, alpha, limit, bias, offs)


def moe_combine(y: torch.Tensor, pos: torch.Tensor, weights: torch.Tensor, *, bias: torch.Tensor | None = None, offs: torch.Tensor | None = None) -> torch.Tensor:
    """EXTENSION (no reference counterpart): the weighted sum that ends a mixture-of-experts layer, one streaming HIP kernel.  y is (M, H) bf16 (the down projection's
    sorted rows), pos (T, topk) int32 (moe_sort's third result), weights (T, topk) float32; the result is (T, H) bf16 with, for every column c,

        acc = +0.0f;  for k in 0 .. topk-1, in this order:  if 0 <= pos[t, k] < M:  acc = acc + weights[t, k] * float(y[pos[t, k], c]);   out[t, c] = bf16(acc)

    every product and every sum rounded to fp32 on its own (no fma: numpy.float32 reproduces it bit for bit), bf16 by round-to-nearest-even.  A slot with pos outside
    [0, M) is SKIPPED, not multiplied by zero: the unspecified rows a grouped GEMM leaves past offs[-1] (NaN, inf, garbage) never reach the result, and a token
    whose slots are all dropped gives +0.  A gather without atomics: deterministic.  H % 8 == 0, 1 <= topk <= 32; no size limit below 2^31 rows / columns.

    bias (E, H) bf16 with offs (E,) int32 (the grouped GEMMs' cumulative END rows; optional for E == 1): the down projection's per-expert bias of gpt-oss, added to
    every gathered row in bf16 as the reference model adds it to the GEMM result -- a kernel of its own; without a bias the call is the op above, unchanged:

        acc = +0.0f;  for k in slot order:  p = pos[t, k];  if 0 <= p < M:  v = bf16(float(y[p, c]) + float(bias[g(p), c]));  acc = acc + weights[t, k] * float(v)

    g(p) = min(E - 1, #{g : offs[g] <= p}) is the group the grouped GEMM computed row p in, so an expert_map needs no special case.  Skipped slots stay skipped:
    nothing of y or bias read for them reaches out.  1 <= E <= 1024; malformed offs select some expert in [0, E).  Measured 2.5-4.5x faster than torch's bias add
    followed by the op; the bias costs 1.4-4.1 us over the op without one (profiles/bench_swiglu_oai_mi355x.txt)."""
    if bias is not None:
        if not torch.compiler.is_compiling():
            if bias.dim() != 2 or bias.size(1) != y.size(-1):
                raise ValueError(f"bias must be (E, H) = (E, {y.size(-1)}) (got {tuple(bias.shape)})")
            _check_bias_offs(bias, offs)
        return _output("moe_combine_bias", y, pos, weights, bias, offs)
    if offs is not None:
        raise ValueError("offs without a bias")
    return _output("moe_combine", y, pos, weights)


def _decode_single_launch_wins(m: int, n: int, k: int, rot: int, device: torch.device | None = None) -> bool:
    """The measured one-launch / two-launch rule of the activation path.  [r4] It lives in the C library now
    (``qutlass_amd_activation_path_launches``, csrc/capi.hip: thresholds, measurements and the CU-count scaling are documented there), so
    that a caller of the C ABI gets the same rule; this is the Python face of it.  The rule scales with the CU count of HIP's CURRENT device, so it is asked
    with the operand's device current (a mixed or partitioned node would otherwise be judged by device 0)."""
    ask = lambda: _lib.load().qutlass_amd_activation_path_launches(int(m), int(n), int(k), int(rot)) == 1
    if device is not None and device.type == "cuda" and torch.cuda.is_available():
        with torch.cuda.device(device):
            return ask()
    return ask()


def fused_quantize_matmul_mxf4_bf16_tn(x: torch.Tensor, h: torch.Tensor, b: torch.Tensor, b_sf: torch.Tensor, alpha: torch.Tensor, *,
                                       method: Literal["quest", "abs_max"] = "quest", single_launch: bool | None = None) -> torch.Tensor:
    """EXTENSION: ``matmul_mxf4_bf16_tn(*fusedQuantizeMx(x, h, method=method) -> to_blocked, b, b_sf, alpha)`` -- the activation path of
    one linear layer (qutlass/__init__.py:149-180 -> qutlass/utils.py:160-193 -> qutlass/__init__.py:34-76) in fewer launches, same bits:
      * TWO launches: the quantizer writes GEMM-ready scales (``fusedQuantizeMxBlocked``), then the GEMM;
      * ONE launch for decode batches (csrc/gemm_mx_fusedq.hip.h: the small-batch GEMM rotates and quantises its own A operand),
        chosen where it measured faster (``qutlass_amd_activation_path_launches`` in the C library, calibrated on a 256-CU MI355X and scaled
        with the CU count); ``single_launch=True / False`` forces either.
    ``method`` defaults to ``"quest"`` like ``fusedQuantizeMx`` (qutlass/__init__.py:149): swapping the composed calls for this helper keeps the quantizer."""
    code = _method_code(method)
    k = x.size(-1)
    m = x.numel() // k if k else 0
    if single_launch is None:
        single_launch = _decode_single_launch_wins(m, b.size(0), k, h.size(0), x.device)
    if single_launch:
        out = torch.ops.qutlass_amd.fusedQuantizeMatmulMxf4(x, h, b, b_sf, alpha, code)
        return out.view(*x.shape[:-1], b.size(0))
    a_q, a_sf = fusedQuantizeMxBlocked(x, h, method=method)
    return qutlass_CUDA.matmul_mxf4_bf16_tn(a_q.view(-1, k // 2), b, a_sf, b_sf, alpha).view(*x.shape[:-1], b.size(0))


def backward_t_bf16(x: torch.Tensor, h: torch.Tensor, xh_e2m1: torch.Tensor = None,
                    xh_e8m0: torch.Tensor = None) -> tuple[torch.Tensor, torch.Tensor]:
    """qutlass/__init__.py:206-243: abs-max MXFP4 of x^T (last two dims swapped) rotated per 32 along the old
    second-to-last dim.  Outputs (.., M, N/2) float4_e2m1fn_x2 and (.., M, N/32) e8m0 for x of shape (.., N, M)."""
    assert x.dtype == h.dtype == torch.bfloat16 and x.is_contiguous() and h.is_contiguous()
    if xh_e2m1 is None and xh_e8m0 is None:
        return _output("backward_t", x, h)
    xh_e2m1, xh_e8m0 = _provided("backward_t", (x, h), xh_e2m1, xh_e8m0)
    assert xh_e2m1.dtype == torch.float4_e2m1fn_x2 and xh_e8m0.dtype == torch.float8_e8m0fnu
    assert xh_e2m1.is_contiguous() and xh_e8m0.is_contiguous()
    _ops_amd.backward_t_bf16_(x, h, xh_e2m1, xh_e8m0)
    return xh_e2m1, xh_e8m0


def _provided(op: str, args, xh_e2m1, xh_e8m0):
    """The results of backward_t_bf16 / backward_qt_bf16 where the caller provides some: the others from the op's row.  Its allocator puts them on h's device, as the
    reference's wrappers do (and the fake kernel with it); for every valid call that is x's device."""
    if xh_e2m1 is not None and xh_e8m0 is not None:
        return xh_e2m1, xh_e8m0
    fresh = ops.OUTPUT_OPS[op].alloc(*args)
    return fresh[0] if xh_e2m1 is None else xh_e2m1, fresh[1] if xh_e8m0 is None else xh_e8m0


def backward_qt_bf16(x_e2m1: torch.Tensor, x_e8m0: torch.Tensor, h: torch.Tensor, alpha: torch.Tensor,
                     xh_e2m1: torch.Tensor = None, xh_e8m0: torch.Tensor = None) -> tuple[torch.Tensor, torch.Tensor]:
    """qutlass/__init__.py:246-286: the same on an MXFP4 operand (x_e2m1 (.., N, M/2), x_e8m0 (.., N, M/32))."""
    assert x_e2m1.is_contiguous() and x_e8m0.is_contiguous() and h.is_contiguous()
    if xh_e2m1 is None and xh_e8m0 is None:
        return _output("backward_qt", x_e2m1, x_e8m0, h, alpha)
    xh_e2m1, xh_e8m0 = _provided("backward_qt", (x_e2m1, x_e8m0, h, alpha), xh_e2m1, xh_e8m0)
    assert xh_e2m1.is_contiguous() and xh_e8m0.is_contiguous()
    _ops_amd.backward_qt_bf16_(x_e2m1, x_e8m0, h, alpha, xh_e2m1, xh_e8m0)
    return xh_e2m1, xh_e8m0


def backward_bf16_square_double_mxfp8(x_bf16: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """qutlass/__init__.py:288-297: e4m3 with one e8m0 per 32 x 32 block, returned row-wise (m_pad, n/32) and column-wise
    (n, m_pad/32), m_pad = rows rounded up to 128.  The missing rows are zeros INSIDE the kernel: no padded copy of x."""
    return _output("square_double_mxfp8", x_bf16)


def mxfp4_transpose_mxfp8(x_fp4: torch.Tensor, scales: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """qutlass/__init__.py:299-315: MXFP4 (m, n/2) + e8m0 (m, n/32) -> transposed e4m3 (n, m_pad) + e8m0 (n, m_pad/32), m_pad = rows
    rounded up to 256 as in the reference.  The padding rows (zero codes, unit scales) exist only inside the kernel: x_fp4 is
    not copied and `scales` is not written (the reference's own "TODO: padding in kernel")."""
    return _output("transpose_mxfp8", x_fp4, scales)


_OUT_OF_SCOPE = ()


def __getattr__(name):
    if name in _OUT_OF_SCOPE:
        raise AttributeError(
            f"qutlass_amd does not provide {name!r} yet: it is outside the hot path this build covers "
            "(SURVEY.md section 8f lists it as 'next')."
        )
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
