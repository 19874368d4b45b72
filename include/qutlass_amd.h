/*
 * qutlass_amd.h -- C ABI of the MI355X (gfx950) microscaled low-bit GEMM library.
 *
 * This is the drop-in boundary for the qutlass hot path: every entry point replaces one host
 * launcher that the reference's torch op bindings (qutlass/csrc/bindings.cpp) call, with plain
 * device pointers, sizes and a HIP stream instead of torch::stable::Tensor.  A maintainer of the
 * reference binds these from bindings.cpp (or from Python via ctypes) -- see INTEGRATION.md.
 *
 * Conventions
 *   - all pointers are DEVICE pointers on the current HIP device; `stream` is a hipStream_t
 *     (NULL = the legacy default stream).  Calls are asynchronous and never synchronise.
 *   - return value: 0 = launched; QAMD_ERR_INVALID = argument rejected (nothing launched);
 *     QAMD_ERR_HIP = the HIP runtime refused the launch.  qutlass_amd_last_error() returns a
 *     thread-local message for the last non-zero return.
 *   - no global state besides the one verification switch at the end of this file; re-entrant; the library never allocates
 *     (the reference cudaMalloc's a CUTLASS workspace per call, gemm.cu:160-162); ops that use
 *     scratch (mxf8 NN pre-pass, split-K of the *_ws GEMMs) take it from the caller.
 */
#ifndef QUTLASS_AMD_H_
#define QUTLASS_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QAMD_OK 0
#define QAMD_ERR_INVALID 1
#define QAMD_ERR_HIP 2

#define QAMD_METHOD_QUEST 0
#define QAMD_METHOD_ABSMAX 1

/* ---- block-scaled GEMMs:  D[M,N] (bf16, row-major) = alpha[0] * (A.SFA) (B.SFB)^T ------------- */

/*
 * Input contract of the MX GEMMs below (MXFP4 / MXFP8, TN / NN, row-major-scale and grouped entries, every kernel form behind them;
 * pinned by tests/test_gpu_mx_scale_range.py and tests/test_gpu_gemm_footprint.py):
 *   * e8m0 scale bytes 0 ... 254 are the powers 2^-127 ... 2^127, each on its own: a block whose two scales are far apart
 *     (0 against 254) but whose product is ordinary contributes exactly that product.  Byte 255 is NaN: it makes NaN exactly the
 *     outputs of its A row / B column (every K group, the last one and the rows next to a tile or expert boundary included) and
 *     no other output.
 *   * fp8 operand codes follow IEEE / OCP propagation: the e4m3 NaN codes 0x7f / 0xff and the e5m2 NaN codes give NaN, e5m2 +-inf
 *     gives +-inf by the sign of the product, inf x 0 and inf - inf give NaN.
 *   * Nothing outside [D, D + M N) is written (grouped: rows past offs[E-1] are left alone), nor outside the workspace_bytes
 *     handed to an entry that takes a workspace.
 *   * Bytes outside the operands and outside the extents of the scale operands (row-major: rows x K/32; blocked: the padded
 *     to_blocked image) are never consumed.  The padding ROWS of a blocked image may hold anything; its scale COLUMNS past K
 *     (K % 128 != 0) meet masked-out operand bytes only, so any finite byte there contributes nothing.
 */

/*
 * MXFP4.  A: (M, K/2) bytes, B: (N, K/2) bytes, two e2m1 per byte (element 2j = low nibble), K % 128 == 0.
 * A_sf / B_sf: e8m0, one per 32 K-elements, in the to_blocked layout of a
 * (ceil(M/128)*128, ceil(K/128)*4) matrix (resp. N).  alpha: device fp32[1].  N % 8 == 0.
 * Replaces matmul_host_mxf4_bf16_tn (qutlass/csrc/gemm.cu:174-248; declared include/gemm.h:21-27;
 * called from bindings.cpp:32-66).
 */
int qutlass_amd_matmul_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                    void* stream);

/*
 * MXFP4, small-batch variant: same operands, but A_sf / B_sf are the UN-swizzled row-major (M, K/32) / (N, K/32) e8m0
 * matrices (what fusedQuantizeMx writes, without to_blocked).  Any M is accepted; built for small batches: an LDS-free
 * split-K kernel for M <= 32 against a small weight, the 64x64 ring kernel with row-major scale fetch for N >= 8192 or
 * M > 32 (both weight-bandwidth bound).  K % 128 == 0, N % 8 == 0.
 * Replaces matmul_host_ada_mxf4_bf16_tn (qutlass/csrc/gemm_ada.cu:30-135; bindings.cpp:104-138; scale addressing
 * cutlass_extensions/gemm/threadblock/mx_mma_multistage.h:418-448).
 */
int qutlass_amd_matmul_ada_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                        const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                        void* stream);

/*
 * EXTENSION (no counterpart in the reference): grouped MXFP4 GEMM for mixture-of-experts layers, one launch over E experts.
 * A: (M, K/2) tokens sorted by expert, A_sf: row-major (M, K/32) e8m0 (what fusedQuantizeMx writes).  B: (E, N, K/2) stacked
 * expert weights, B_sf: row-major (E, N, K/32).  alpha: device fp32[n_alpha], n_alpha = 1 (shared) or E (per expert).
 * offs: device int32[E], the cumulative END rows of the groups (torch._grouped_mm's convention): group g = rows
 * [offs[g-1], offs[g]), offs[-1] := 0.  D[r] = alpha[g] * (A_r . SFA) (B_g . SFB_g)^T for every row r of group g; rows at or past
 * offs[E-1] are not written.  The offsets are read on the device (graph capture works); each is clamped to [0, M] and a
 * decreasing one is an empty group, so malformed offsets never address outside the operands.
 * K % 128 == 0, N % 8 == 0, 1 <= E <= 1024, M * K/2 and N * K/2 (one expert) below 2 GiB; the stack may exceed 2 GiB.
 * M == 0 returns QAMD_OK without a launch.
 */
int qutlass_amd_grouped_matmul_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                            const float* alpha, int64_t n_alpha, const int32_t* offs, void* D,
                                            int64_t M, int64_t N, int64_t K, int64_t E, void* stream);

/*
 * NVFP4.  Same operand layout, scales are e4m3fn per 16 K-elements in the to_blocked layout of a
 * (ceil(M/128)*128, ceil(K/64)*4) matrix; K % 32 == 0.
 * Replaces matmul_host_nvf4_bf16_tn (gemm.cu:250-326; bindings.cpp:68-102).
 */
int qutlass_amd_matmul_nvf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                    void* stream);

/*
 * MXFP8 (e4m3fn data, e8m0 per 32).  TN: A (M,K), B (N,K) row-major.  K % 32 == 0.
 * Replaces matmul_host_mxf8_bf16_tn (gemm.cu:328-386; bindings.cpp:140-177).
 */
int qutlass_amd_matmul_mxf8_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                    void* stream);

/*
 * The same two GEMMs with caller-owned scratch, which unlocks split-K for small outputs with a long K (fewer than 256
 * tiles of 64x64 -- at most 128 of them -- and K >= 32 stages of 128 bytes: e.g. M = 64, N = 4096, K = 14336 runs 64
 * workgroups without it).
 * Each K split writes its fp32 partial to workspace[z][M][N]; a second kernel sums the splits in fixed order, applies
 * alpha and rounds to bf16 (deterministic; identical to the single-pass result whenever the fp32 partial sums are
 * exact, which is the regime the reference's equality tests run in).  qutlass_amd_gemm_splitk_workspace_bytes(ebits = 4
 * or 8, M, N, K) returns the bytes the split needs, 0 when the shape does not split; a NULL or smaller workspace
 * silently runs the single-pass kernel.  The workspace is used on `stream` for the duration of the call's kernels and must be
 * 16-byte aligned (the partials are written as 16-byte vectors; a misaligned pointer is rejected with QAMD_ERR_INVALID).
 * (The reference allocates and frees a CUTLASS workspace inside every call, gemm.cu:160-162.)
 *
 * Alignment.  A, B, both scale operands and D of the matmul_{mxf4,mxf8,nvf4}_bf16_* entries must be 16-byte aligned (QAMD_ERR_INVALID otherwise): operands are
 * fetched as 16-byte pieces, the output leaves as 16-byte stores.  Tensors that torch allocates, and row ranges of them, are.  (The reference's CUTLASS kernels
 * require 128-bit alignment through their TMA descriptors, gemm.cu:90-143.)
 *
 * Reproducibility.  Every entry point is deterministic: the same call on the same device returns the same bytes, run after run and
 * under HIP-graph replay.  It is NOT bit-stable ACROSS entry points or devices for general data: whether a shape splits K depends on
 * whether a workspace was passed and on the device's CU count (the plans scale with it), and a split sums the fp32 partials in a
 * different order than the single pass -- the bf16 output can differ in its last bit.  Exact-regime operands (every partial sum
 * exactly representable: the regime of the reference's own equality tests) give identical bytes on every path.  For one summation
 * order everywhere call the entries without `_ws`.
 */
int64_t qutlass_amd_gemm_splitk_workspace_bytes(int ebits, int64_t M, int64_t N, int64_t K);
int qutlass_amd_matmul_mxf4_bf16_tn_ws(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                       const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                       void* workspace, int64_t workspace_bytes, void* stream);
int qutlass_amd_matmul_mxf8_bf16_tn_ws(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                       const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                       void* workspace, int64_t workspace_bytes, void* stream);

/*
 * [r3] The NVFP4 GEMM with caller-owned scratch: split-K for outputs of a few dozen 128x128 tiles with a long K (e.g. M = 256, N = 4096,
 * K = 14336), where the single pass can only fill the chip with 64x64 tiles whose 32x32 wave tiles dequantise two operand fragments per MFMA.
 * Same contract as the MX entries above: fp32 partials in workspace[z][M][N], summed in fixed z order by a second kernel (alpha, bf16);
 * qutlass_amd_nvf4_splitk_workspace_bytes(M, N, K) returns the bytes the planned split needs, 0 when the shape does not split; a NULL or
 * smaller workspace silently runs the single-pass kernel (= qutlass_amd_matmul_nvf4_bf16_tn).
 */
int64_t qutlass_amd_nvf4_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K);
int qutlass_amd_matmul_nvf4_bf16_tn_ws(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                       const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                       void* workspace, int64_t workspace_bytes, void* stream);

/*
 * MXFP8 NN: A is stored (K, M) row-major (the reference's ColumnMajor A), B (N, K); A_sf is still the
 * to_blocked layout of the (M, K/32) scale matrix.  K % 32 == 0, M % 16 == 0 (the reference's
 * AlignmentA = 16 on the contiguous M axis, gemm.cu:400).
 * workspace: caller-owned device scratch, used on `stream` only for the duration of the call's kernels (the library
 * itself never allocates).  Small problems re-lay A as (M, K) with a byte-transpose pre-pass and then run the TN kernel:
 * they need M * K bytes.  Problems whose 256x256 tiles fill the chip read the (K, M) operand directly and need NONE.
 * qutlass_amd_mxf8_nn_workspace_bytes_for(M, N, K) returns what THIS shape needs (0 for the in-place path: workspace may be
 * NULL); qutlass_amd_mxf8_nn_workspace_bytes(M, K) is the shape-independent upper bound M * K.
 * Replaces matmul_host_mxf8_bf16_nn (gemm.cu:388-434; bindings.cpp:179-216).
 */
int64_t qutlass_amd_mxf8_nn_workspace_bytes(int64_t M, int64_t K);
int64_t qutlass_amd_mxf8_nn_workspace_bytes_for(int64_t M, int64_t N, int64_t K);
int qutlass_amd_matmul_mxf8_bf16_nn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                    void* workspace, int64_t workspace_bytes, void* stream);

/*
 * EXTENSION (no reference counterpart): MXFP8 with an e5m2 A operand -- the gradient x activation GEMMs of a QAT
 * backward pass (BASELINE.json configs[4]).  The reference's entry points reject every element type but e4m3
 * (bindings.cpp:157-160, 196-199; gemm.cu:339-345, 399-403); CDNA4's scaled MFMA takes the format per operand.
 * a_format / b_format: QAMD_FP8_E4M3 or QAMD_FP8_E5M2; b_format must be QAMD_FP8_E4M3.  Everything else (layouts, scales,
 * alignment, workspace rules, return codes) as the entry of the same name without `_fmt`: the TN entry takes the optional
 * split-K scratch of qutlass_amd_matmul_mxf8_bf16_tn_ws (NULL / 0 = never split), the NN entry the re-layout scratch reported by
 * qutlass_amd_mxf8_nn_workspace_bytes_for(M, N, K) (may be NULL when that returns 0: the in-place operand path).  With both
 * formats E4M3 they ARE those entries.
 */
#define QAMD_FP8_E4M3 0
#define QAMD_FP8_E5M2 1
int qutlass_amd_matmul_mxf8_bf16_tn_fmt(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                        const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                        int a_format, int b_format, void* workspace, int64_t workspace_bytes, void* stream);
int qutlass_amd_matmul_mxf8_bf16_nn_fmt(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                        const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                        int a_format, int b_format, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * EXTENSION (no counterpart in the reference): grouped MXFP8 GEMM for mixture-of-experts layers, one launch over E experts.
 * A: (M, K) fp8 tokens sorted by expert, e4m3 or e5m2 (a_format: QAMD_FP8_E4M3 / QAMD_FP8_E5M2), A_sf: row-major (M, K/32) e8m0.
 * B: (E, N, K) e4m3 stacked expert weights, B_sf: row-major (E, N, K/32).  alpha: device fp32[n_alpha], n_alpha = 1 (shared)
 * or E (per expert).  offs: device int32[E], the cumulative END rows of the groups (torch._grouped_mm's convention): group g =
 * rows [offs[g-1], offs[g]), offs[-1] := 0.  D[r] = alpha[g] * (A_r . SFA) (B_g . SFB_g)^T for every row r of group g; rows at
 * or past offs[E-1] are not written.  The offsets are read on the device (graph capture works); each is clamped to [0, M] and a
 * decreasing one is an empty group, so malformed offsets never address outside the operands.
 * K % 128 == 0, N % 8 == 0, 1 <= E <= 1024, M * K and N * K (one expert) below 2 GiB; the stack may exceed 2 GiB.
 * M == 0 returns QAMD_OK without a launch.
 */
int qutlass_amd_grouped_matmul_mxf8_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                            const float* alpha, int64_t n_alpha, const int32_t* offs, void* D,
                                            int64_t M, int64_t N, int64_t K, int64_t E, int a_format, void* stream);

/*
 * EXTENSION (no counterpart in the reference): grouped W4A8 GEMM for mixture-of-experts layers -- MXFP8 tokens against MXFP4
 * expert weights as they are stored (gpt-oss checkpoints, fusedQuantizeMx's output), one launch over E experts.
 * A: (M, K) e4m3 tokens sorted by expert, A_sf: row-major (M, K/32) e8m0 (fusedQuantizeMxf8 / fusedGatherQuantizeMxf8 write both).
 * B: (E, N, K/2) packed e2m1 stacked expert weights, B_sf: row-major (E, N, K/32) e8m0 (the operands of
 * qutlass_amd_grouped_matmul_mxf4_bf16_tn).  alpha, offs, D, the clamping of the offsets and the rows that are not written: as
 * qutlass_amd_grouped_matmul_mxf8_bf16_tn.  D[r] = alpha[g] * (A_r . SFA_r) (B_g . SFB_g)^T with fp32 accumulation, one fp32
 * multiply by alpha and one rounding to bf16.  Scale byte 255 and the e4m3 NaN code give NaN outputs as they do there.
 * K % 128 == 0, N % 8 == 0, 1 <= E <= 1024, M * K and N * K/2 (one expert) below 2 GiB; the stack may exceed 2 GiB.
 * M == 0 returns QAMD_OK without a launch.  Wave-owned 32x32 / 32x16 / 64x32 tiles only: there is no 64x64 ring form, so
 * prefill-sized groups run on the decode tiles.
 */
int qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                                 const float* alpha, int64_t n_alpha, const int32_t* offs, void* D,
                                                 int64_t M, int64_t N, int64_t K, int64_t E, void* stream);

/*
 * EXTENSION (no counterpart in the reference): grouped W4A6 GEMM for mixture-of-experts layers -- MXFP6 (e2m3) tokens against
 * MXFP4 expert weights as they are stored, one launch over E experts: W4A8's accuracy class at 3/4 of its token bytes.
 * A: (M, 3K/4) bytes of packed e2m3 codes, tokens sorted by expert (the MXFP6 operand format at the quantizers below), 16-byte
 * aligned; A_sf: row-major (M, K/32) e8m0 (fusedQuantizeMxf6 / fusedGatherQuantizeMxf6 write both).  B, B_sf, alpha, offs, D, the
 * clamping of the offsets and the rows that are not written: as qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn.
 * D[r] = bf16(alpha[g] * sum_k a[r, k] b[g, n, k]): exact products, fp32 sums, one fp32 multiply by alpha, one rounding.  Scale
 * bytes 0 ... 254 mean 2^(b - 127); byte 255 on either side makes that row's or column's outputs NaN (e2m3 has no NaN code: the
 * quantizers mark a group that held a NaN or an infinity with scale byte 255).
 * K % 128 == 0, N % 8 == 0, 1 <= E <= 1024, M * 3K/4 and N * K/2 (one expert) below 2 GiB; the stack may exceed 2 GiB.
 * M == 0 returns QAMD_OK without a launch.  Wave-owned 32x32 / 32x16 / 64x32 tiles only, as for W4A8.
 */
int qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                                 const float* alpha, int64_t n_alpha, const int32_t* offs, void* D,
                                                 int64_t M, int64_t N, int64_t K, int64_t E, void* stream);

/*
 * EXTENSION (no counterpart in the reference): grouped W4A16 GEMM for mixture-of-experts layers -- bf16 tokens, unquantised and
 * without scales, against MXFP4 expert weights as they are stored (gpt-oss checkpoints, fusedQuantizeMx's output), one launch over
 * E experts.  A: (M, K) bf16 tokens sorted by expert.  B, B_sf, alpha, offs, D, the clamping of the offsets and the rows that are
 * not written: as qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn.
 * D[r, n] = bf16(alpha[g] * sum_k A[r, k] * w[g, n, k]), w = e2m1(code) * 2^(B_sf - 127) held as bf16 (exact whenever it is 0 or
 * 2^-126 <= |w| <= bf16's largest finite value: every code under scale bytes 2 ... 252).  The products are exact in fp32, the
 * sums are fp32, one fp32 multiply by alpha, one rounding to bf16.  Scale byte 255 gives NaN in every output of that weight row
 * for the rows of that expert; bytes 0, 1, 253, 254 are outside the exact contract (byte 0 reads as w = 0, byte 1 gives bf16
 * subnormals, 253 / 254 may overflow to inf).  NaN and inf in A propagate as in fp64 arithmetic.
 * src_row (may be NULL): device int32[M].  With it A is the UNSORTED (T, K) tokens and row r of D reads A[src_row[r]] -- the
 * gather of the routed tokens in the GEMM; T * K * 2 must stay below 2 GiB, an index outside [0, T) reads an all-zero token and
 * never addresses outside A.  T is ignored when src_row is NULL.
 * K % 128 == 0, N % 8 == 0, 1 <= E <= 1024, M * 2K and N * K/2 (one expert) below 2 GiB; the stack may exceed 2 GiB.
 * M == 0 returns QAMD_OK without a launch.  Wave-owned 32x32 / 32x16 / 64x32 tiles only, as for W4A8.
 */
int qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn(const void* A, const void* B, const void* B_sf, const float* alpha, int64_t n_alpha,
                                                 const int32_t* offs, const int32_t* src_row, int64_t T, void* D,
                                                 int64_t M, int64_t N, int64_t K, int64_t E, void* stream);

/*
 * EXTENSION (no counterpart in the reference): grouped NVFP4 GEMM for mixture-of-experts layers, one launch over E experts.
 * A: (M, K/2) packed e2m1 tokens sorted by expert, A_sf: ROW-MAJOR (M, K/16) e4m3 (the quantizer's buffer as it is, no to_blocked).
 * B: (E, N, K/2) stacked expert weights, B_sf: row-major (E, N, K/16).  alpha: device fp32[n_alpha], n_alpha = 1 (shared)
 * or E (per expert).  offs: device int32[E], the cumulative END rows of the groups (torch._grouped_mm's convention): group g =
 * rows [offs[g-1], offs[g]), offs[-1] := 0.  D[r] = alpha[g] * (A_r . SFA_r) (B_g . SFB_g)^T for every row r of group g, in
 * qutlass_amd_matmul_nvf4_bf16_tn's arithmetic; rows at or past offs[E-1] are not written.  The offsets are read on the device
 * (graph capture works); each is clamped to [0, M] and a decreasing one is an empty group, so malformed offsets never address
 * outside the operands.
 * K % 128 == 0, N % 8 == 0, 1 <= E <= 1024, M * K/2 and N * K/2 (one expert) below 2 GiB; the stack may exceed 2 GiB.
 * M == 0 returns QAMD_OK without a launch.
 */
int qutlass_amd_grouped_matmul_nvf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                            const float* alpha, int64_t n_alpha, const int32_t* offs, void* D,
                                            int64_t M, int64_t N, int64_t K, int64_t E, void* stream);

/* ---- fused rotate + quantize ------------------------------------------------------------------ */

/*
 * x: bf16[numel] viewed as (numel/rot, rot); h: bf16[rot*rot] row-major (runtime matrix, y = x_g . h);
 * rot in {32, 64, 128}; numel % rot == 0.  method: QAMD_METHOD_QUEST / QAMD_METHOD_ABSMAX.
 * out_e2m1: numel/2 bytes; out_e8m0: numel/32 bytes written FLAT in group order (the caller's
 * (padded_rows, padded_cols) buffer keeps its padding untouched, as in the reference);
 * out_mask: NULL, or numel/8 bytes (one u32 per 32-group; quest + rot 32 only).
 * Alignment: h must be 16-byte aligned for rot >= 64 (QAMD_ERR_INVALID otherwise; the kernel stages it with 16-byte loads).
 * Non-finite activations follow the reference's arithmetic: NaN -> code 0x7 whatever its sign, +-inf -> +-6 or, under an
 * infinite group scale (e8m0 byte 255), 0 / NaN as x / inf gives (tests/test_gpu_round5.py).
 * Replaces fusedQuantizeMx{Quest,AbsMax}{,Had64,Had128}_host (fused_quantize_mx.cu:107-207) and
 * fusedQuantizeMxQuestWithMask_host (fused_quantize_mx_mask.cu:107-123); bindings.cpp:218-333.
 */
int qutlass_amd_fused_quantize_mx(const void* x, const void* h, int rot, int64_t numel, int method,
                                  void* out_e2m1, void* out_e8m0, void* out_mask, void* stream);

/*
 * NVFP4 variant: rot in {16, 32, 64, 128}; out_e4m3: numel/16 bytes (e4m3fn), flat;
 * global_scale: device fp32[1].
 * Replaces fusedQuantizeNv{Quest,AbsMax}{,Had32,Had64,Had128}_host (fused_quantize_nv.cu:109-252;
 * bindings.cpp:335-426).
 */
int qutlass_amd_fused_quantize_nv(const void* x, const void* h, int rot, int64_t numel, int method,
                                  const float* global_scale, void* out_e2m1, void* out_e4m3,
                                  void* stream);

/*
 * EXTENSION (no reference counterpart; the reference's activation path is fusedQuantizeMx -> to_blocked -> matmul, three launches,
 * qutlass/__init__.py:149-180 + qutlass/utils.py:160-193): the same quantizers, but the scale bytes are written DIRECTLY in the
 * to_blocked() layout the GEMMs consume -- one launch instead of two.  x is a (rows, k) bf16 matrix (k % max(rot, 32) == 0);
 * out_*_blocked: ceil(rows/128)*128 * ceil(k/gs/4)*4 bytes (gs = 32 MX / 16 NV), padding zero-filled; byte for byte what
 * qutlass_amd_to_blocked() makes of the flat scales of the entry above (tests/test_gpu_parity.py).  Everything else as above.
 */
int qutlass_amd_fused_quantize_mx_blocked(const void* x, const void* h, int rot, int64_t rows, int64_t k, int method,
                                          void* out_e2m1, void* out_e8m0_blocked, void* out_mask, void* stream);
int qutlass_amd_fused_quantize_nv_blocked(const void* x, const void* h, int rot, int64_t rows, int64_t k, int method,
                                          const float* global_scale, void* out_e2m1, void* out_e4m3_blocked,
                                          void* stream);

/*
 * EXTENSION (no reference counterpart): the activation of a gated MLP, alone and fused into the quantizers above.
 * x: bf16 (rows, 2 * inter), contiguous, 16-byte aligned; gate = x[:, :inter], up = x[:, inter:] (what a GEMM against stacked [W1; W3] returns).
 *     s   = bf16_rne(g / (1 + exp(-g)))      g widened to fp32; the CORRECTLY rounded bf16 of silu(g): fp32 arithmetic, redone in fp64 where that lands within
 *                                            12 fp32 ulp of a bf16 tie and for g < -16; a large negative g (below about -97) gives -0
 *     act = bf16_rne(float(s) * float(u))    -- what silu(gate) * up gives in bf16
 * qutlass_amd_silu_mul_bf16 writes act, bf16 (rows, inter); inter % 8 == 0; rows, inter < 2^31 (64-bit addressing: no byte limit).
 * qutlass_amd_fused_silu_mul_quantize_{mx,nv}: qutlass_amd_fused_quantize_{mx,nv}[_blocked] applied to act viewed as (rows, inter), byte for byte (same
 * rotation, scale rules, encoder, layouts and padding contracts: blocked == 0 writes the scales flat and leaves the rest of the caller's buffer untouched,
 * blocked != 0 writes the to_blocked layout of the (rows, inter / gs) scale matrix, padding zero-filled) -- without act ever being written to memory.
 * inter % max(rot, 32) == 0; rot as in the plain entries; hardware e2m1 convert, no clip mask.
 * LIMIT: the fused kernels address x with 32-bit offsets from one buffer descriptor: x must stay below 2 GiB (rows * inter < 2^29), QAMD_ERR_INVALID beyond
 * (run such an input as row ranges).  Non-finite gate / up values (the unwritten tail rows of a grouped GEMM's output, say) give unspecified bytes for their
 * own rotation groups only.  rows == 0 returns QAMD_OK without a launch.
 */
int qutlass_amd_silu_mul_bf16(const void* x, int64_t rows, int64_t inter, void* out, void* stream);
int qutlass_amd_fused_silu_mul_quantize_mx(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method,
                                           int blocked, void* out_e2m1, void* out_e8m0, void* stream);
int qutlass_amd_fused_silu_mul_quantize_nv(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method,
                                           const float* global_scale, int blocked, void* out_e2m1, void* out_e4m3,
                                           void* stream);

/*
 * EXTENSION (no reference counterpart): the two ends of a mixture-of-experts MLP around the grouped GEMMs -- dispatch (tokens -> rows sorted by expert, quantized)
 * and combine (sorted rows -> tokens, weighted).
 *
 * qutlass_amd_fused_gather_quantize_{mx,nv}: qutlass_amd_fused_quantize_{mx,nv} applied to xg = x[src_row], byte for byte, without xg ever being written to memory.
 *   x        bf16 (t, k), contiguous, 16-byte aligned; k % max(rot, 32) == 0; rot as in the plain entries; hardware e2m1 convert, no clip mask
 *   src_row  int32 (m), device memory, read by the kernel (no host sync: the call is graph-capturable).  An index outside [0, t) -- -1 as a padding
 *            sentinel, INT32_MIN, INT32_MAX -- gives the bytes of an all-zero row; it cannot fault and cannot read another row.
 *   out_e2m1 (m, k / 2) codes; scales FLAT and row-major in the first m * k / 32 (MX) or m * k / 16 (NV) bytes of the caller's buffer, the rest untouched: what
 *            the grouped GEMMs read as it is.
 * LIMIT: x is addressed with 32-bit offsets from one buffer descriptor: x must stay below 2 GiB (t * k < 2^30), QAMD_ERR_INVALID beyond; m * k < 2^31.
 * m == 0 returns QAMD_OK without a launch.
 *
 * qutlass_amd_moe_combine_bf16: out (t, hdim) bf16 from y (m, hdim) bf16, pos (t, topk) int32 and weights (t, topk) float32, all contiguous:
 *     acc = +0.0f
 *     for k = 0 .. topk - 1, in this order:  if 0 <= pos[t][k] < m:  acc = fadd_rn(acc, fmul_rn(weights[t][k], float(y[pos[t][k]][c])))      (two roundings, no fma)
 *     out[t][c] = bf16_rne(acc)
 * A slot whose pos lies outside [0, m) is skipped, not multiplied by zero: whatever an unreferenced row of y holds (the unwritten tail rows of a grouped GEMM's
 * output) never reaches out.  A gather without atomics: deterministic, independent of the launch geometry.  hdim % 8 == 0, 1 <= topk <= 32; y and out 16-byte
 * aligned; m, t, hdim < 2^31 (64-bit addressing: no byte limit).  t == 0 returns QAMD_OK without a launch.
 */
int qutlass_amd_fused_gather_quantize_mx(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int method,
                                         void* out_e2m1, void* out_e8m0, void* stream);
int qutlass_amd_fused_gather_quantize_nv(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int method,
                                         const float* global_scale, void* out_e2m1, void* out_e4m3, void* stream);
int qutlass_amd_moe_combine_bf16(const void* y, int64_t m, int64_t hdim, const int32_t* pos, const float* weights, int64_t t, int64_t topk, void* out,
                                 void* stream);

/*
 * EXTENSION (no reference counterpart): what a gpt-oss mixture-of-experts layer needs around the grouped GEMMs -- the clamped SwiGLU with the gate/up bias of the
 * row's expert, alone and fused into the MXFP4 and the MXFP8 (e4m3) quantizer, and moe_combine with the down projection's bias.  The reference model adds each bias to the bf16 GEMM result
 * in bf16; so do these, in the op that reads the GEMM's output.
 *   x      bf16 (rows, 2 * inter), contiguous, 16-byte aligned, [gate | up] halves as above (gpt-oss stores the columns interleaved: de-interleave the weight, its
 *          scales and its bias once at load time)
 *   alpha  fp32, finite, > 0 (gpt-oss: 1.702);  limit  > 0, finite and exactly representable in bf16 (gpt-oss: 7) -- QAMD_ERR_INVALID otherwise
 *   bias   null, or bf16 (e, 2 * inter) in the same halves, 16-byte aligned; 1 <= e <= 1024.  With a bias x is (rows, 2 * inter) SORTED rows and row r takes
 *          bias[g(r)], g(r) = min(e - 1, #{ g : offs[g] <= r }) -- the lookup of the *_nv_grouped entries above; rows at or past offs[e - 1] take expert e - 1's
 *   offs   int32 (e), device memory, 4-byte aligned: the grouped GEMMs' cumulative END rows.  Required for e > 1; never read (may be null) for e == 1.  Malformed
 *          offs select SOME expert in [0, e) and cannot address outside bias.  Without a bias, offs and e are not read.
 * Per element, g, u, bg, bu bf16:
 *     g1 = bias ? bf16_rne(fadd(float(g), float(bg))) : g       u1 = bias ? bf16_rne(fadd(float(u), float(bu))) : u        (what a bf16 tensor add computes)
 *     gc = min(g1, limit)                                       uc = min(max(u1, -limit), limit)                           (exact)
 *     s   = bf16 of the REAL number gc / (1 + exp(-alpha * gc)), correctly rounded (alpha the fp32 value, the product not rounded): fp32 arithmetic with
 *           alpha * log2 e split into a 16-bit part and a remainder, redone in fp64 within 16 fp32 ulp of a bf16 tie and for |alpha * gc| > 16
 *     act = bf16_rne(fmul(float(s), fadd(float(uc), 1.0f)))     (one fp32 add, one fp32 multiply, no fma, then RNE)
 * Fewer roundings than the model's bf16 op chain, on purpose.  For |gc| < 2^-120 the true s lies within 2^-130 (relative) of a tie between bf16 subnormals: s is
 * then within one bf16 step, and no more is promised.  NaN / +-inf in gate, up or bias give unspecified bytes for their own element (fused: their own rotation
 * group).  A zero gate, up and bias give +0: zero-padded columns (gpt-oss: 2880 -> 2944 with zero weight rows and zero bias) stay zero.
 * qutlass_amd_swiglu_oai_mul_bf16 writes act, bf16 (rows, inter); inter % 8 == 0; rows, inter < 2^31 (64-bit addressing).
 * qutlass_amd_fused_swiglu_oai_quantize_mx: qutlass_amd_fused_quantize_mx applied to act viewed as (rows, inter), byte for byte, in one launch: flat scales in the
 * first rows * inter / 32 bytes, the rest of the caller's buffer untouched; rot 32 or 64 (128: QAMD_ERR_INVALID, the message names the two-call composition);
 * inter % rot == 0; both methods; hardware e2m1 convert, no clip mask, no blocked form.  LIMIT: x, and bias, below 2 GiB (rows * inter, e * inter < 2^29).
 * qutlass_amd_fused_swiglu_oai_quantize_mxf8: qutlass_amd_fused_quantize_mxf8 (fmt e4m3) applied to act viewed as (rows, inter), byte for byte, in one launch -- the A
 * operand of qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn: out_fp8 rows * inter bytes of e4m3 codes; flat scales in the first rows * inter / 32 bytes of out_e8m0, the
 * rest of the caller's buffer untouched; rot 32 or 64 (128: QAMD_ERR_INVALID, the message names the two-call composition with fusedQuantizeMxf8); inter % rot == 0;
 * abs-max is the only method; fmt must be QAMD_FP8_E4M3 (a forward activation is e4m3 only: QAMD_ERR_INVALID otherwise); no blocked form.  LIMIT and non-finite
 * inputs as the MXFP4 entry: x, and bias, below 2 GiB (rows * inter, e * inter < 2^29); NaN / +-inf in gate, up or bias give unspecified bytes for their own rotation group.
 * qutlass_amd_moe_combine_bias_bf16: qutlass_amd_moe_combine_bf16 with bias bf16 (e, hdim), 16-byte aligned, and offs as above (required for e > 1):
 *     acc = +0.0f
 *     for k = 0 .. topk - 1, in this order:  p = pos[t][k];  if 0 <= p < m:
 *         v   = bf16_rne(fadd(float(y[p][c]), float(bias[g(p)][c])))
 *         acc = fadd_rn(acc, fmul_rn(weights[t][k], float(v)))
 *     out[t][c] = bf16_rne(acc)
 * g(p) is the group the grouped GEMM computed row p in.  Skipped slots stay skipped: nothing read of y or bias for them reaches out.  Limits as the plain entry.
 * Checks: all before any HIP call; rows == 0 / t == 0 returns QAMD_OK without a launch.
 */
int qutlass_amd_swiglu_oai_mul_bf16(const void* x, int64_t rows, int64_t inter, float alpha, float limit, const void* bias, const int32_t* offs, int64_t e,
                                    void* out, void* stream);
int qutlass_amd_fused_swiglu_oai_quantize_mx(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method, float alpha, float limit,
                                             const void* bias, const int32_t* offs, int64_t e, void* out_e2m1, void* out_e8m0, void* stream);
int qutlass_amd_fused_swiglu_oai_quantize_mxf8(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int fmt, float alpha, float limit,
                                               const void* bias, const int32_t* offs, int64_t e, void* out_fp8, void* out_e8m0, void* stream);
int qutlass_amd_moe_combine_bias_bf16(const void* y, int64_t m, int64_t hdim, const int32_t* pos, const float* weights, int64_t t, int64_t topk,
                                      const void* bias, const int32_t* offs, int64_t e, void* out, void* stream);

/*
 * EXTENSION (no reference counterpart): the two NV quantizers of the MoE chain with ONE GLOBAL SCALE PER EXPERT -- what the per-expert alpha of
 * qutlass_amd_grouped_matmul_nvf4_bf16_tn (alpha[g] = 1 / (a_gs[g] * w_gs[g])) expects of its A operand, in one graph-capturable launch.
 *   global_scales  float32 (e), device memory;  offs  int32 (e), device memory, 4-byte aligned: the grouped GEMMs' cumulative END rows (qutlass_amd_moe_sort's offs);
 *   1 <= e <= 1024.  The expert of operand row r (a sorted row: r < m for the gathering entry, r < rows for the gated one) is
 *       g(r) = min(e - 1, #{ g : offs[g] <= r })
 *   -- for non-decreasing offs the group the grouped GEMM puts the row in; rows at or past offs[e - 1] (the dropped slots, which the GEMM never reads) take expert
 *   e - 1's scale, so every output byte is defined.
 * The bytes of row r, codes and e4m3 scales, are those of the single-scale entry (qutlass_amd_fused_gather_quantize_nv / qutlass_amd_fused_silu_mul_quantize_nv with
 * blocked == 0) called with global_scales[g(r)]; everything else is the sibling's, byte for byte: rotation, scale rule, encoder, FLAT row-major scales with the rest
 * of the caller's buffer untouched (there is no blocked form: the grouped GEMMs read this buffer as it is), the zero-row rule for bad src_row entries, the 2 GiB
 * limit on x.  method quest never reads a global scale: the result is the sibling's, whatever global_scales and offs hold.
 * Malformed offs (negative, beyond the row count, decreasing) cannot fault: the kernel reads offs[0, e) and global_scales[0, e) only, every index clamped, and each
 * row is quantized with the scale of SOME expert in [0, e) -- which one is then unspecified.  No host sync, no workspace.
 * Checks: the sibling's chain in the sibling's order under the name fusedGatherQuantizeNvGrouped / fusedSiluMulQuantizeNvGrouped -- m == 0 / rows == 0 returns
 * QAMD_OK where the sibling does, a null offs joins its null-pointer check --, then e outside [1, 1024], then the alignment of offs; all before any HIP call.
 */
int qutlass_amd_fused_gather_quantize_nv_grouped(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int method,
                                                 const float* global_scales, const int32_t* offs, int64_t e, void* out_e2m1, void* out_e4m3,
                                                 void* stream);
int qutlass_amd_fused_silu_mul_quantize_nv_grouped(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method,
                                                   const float* global_scales, const int32_t* offs, int64_t e, void* out_e2m1, void* out_e4m3,
                                                   void* stream);

/*
 * EXTENSION (no reference counterpart): the rotate + quantize family with 8-BIT codes -- the producers of the A (and B) operands of qutlass_amd_matmul_mxf8_bf16_{tn,nn}
 * and qutlass_amd_grouped_matmul_mxf8_bf16_tn: MXFP8, one e8m0 scale per 32 elements along the row, e4m3fn or e5m2 codes.
 *   fmt   QAMD_FP8_E4M3 (0) or QAMD_FP8_E5M2 (1), the GEMMs' _fmt convention; the gated entry takes QAMD_FP8_E4M3 only (a forward activation has no use for e5m2).
 *   y = x_g . h exactly as qutlass_amd_fused_quantize_mx computes it (x viewed as (numel / rot, rot), h a runtime rot x rot bf16 matrix, bf16 MFMA, fp32 sums;
 *   the identity gives a plain quantizer); rot in {32, 64, 128} (no 16: the scale group is 32).  Then for every 32 consecutive y:
 *       amax = max |y|  (NaNs ignored)          E = the biased exponent field of the FP32 amax          SH = 7 (e4m3) / 14 (e5m2)
 *       e8   = 127 if amax == 0, else clamp(E - SH, 0, 254)                                              -- the scale byte, 2^(e8 - 127)
 *       q    = RNE(y * 2^(127 - e8)) to e4m3fn / e5m2; the scaling is exact, -0 keeps its sign          -- the code byte
 *   The scaled maximum lies in [128, 256) / [2^14, 2^15): no finite input saturates.  Abs-max is the only method (Quest's constant is an FP4 constant); no clip
 *   mask, no global scale.  A NaN input gives NaN codes throughout its own rotation block; the bytes of a block that holds +-inf are unspecified; no other
 *   block is affected.
 *   out_fp8: numel bytes, element order.  Scales: as the MX sibling -- flat in the first numel / 32 bytes with the rest of the caller's buffer untouched
 *   (what the grouped GEMM reads as it is), or, for the _blocked entry and blocked != 0, the to_blocked() layout of the (rows, k / 32) scale matrix, padding zero-filled
 *   (what the dense GEMMs read).
 * qutlass_amd_fused_silu_mul_quantize_mxf8 = the plain entries on act = silu(gate) * up, qutlass_amd_fused_gather_quantize_mxf8 = the plain entry on x[src_row] (an
 * index outside [0, t) gives a zero row: codes 0, scale 127), byte for byte, with the siblings' limits: x below 2 GiB, numel < 2^31.
 * Checks: each entry runs its MX sibling's chain in the sibling's order under the name fusedQuantizeMxf8 / fusedQuantizeMxf8Blocked / fusedSiluMulQuantizeMxf8[Blocked]
 * / fusedGatherQuantizeMxf8, with "invalid fmt" where the sibling has "invalid method"; all before any HIP call.
 */
int qutlass_amd_fused_quantize_mxf8(const void* x, const void* h, int rot, int64_t numel, int fmt, void* out_fp8, void* out_e8m0, void* stream);
int qutlass_amd_fused_quantize_mxf8_blocked(const void* x, const void* h, int rot, int64_t rows, int64_t k, int fmt, void* out_fp8, void* out_e8m0_blocked,
                                            void* stream);
int qutlass_amd_fused_silu_mul_quantize_mxf8(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int fmt, int blocked, void* out_fp8,
                                             void* out_e8m0, void* stream);
int qutlass_amd_fused_gather_quantize_mxf8(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int fmt, void* out_fp8,
                                           void* out_e8m0, void* stream);

/*
 * EXTENSION (no reference counterpart): the rotate + quantize family with 6-BIT codes -- the producers of the A operand of
 * qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn: MXFP6, one e8m0 scale per 32 elements along the row, e2m3 codes.
 *   The MXFP6 (e2m3) operand format: a row of K elements is 3K/4 bytes; element k occupies bits 6k ... 6k+5 of the row read as one little-endian bit string, so a
 *   32-element scale block is the 24 bytes 24j ... 24j+23.  A code is sign (bit 5), 2 exponent bits (bias 1), 3 mantissa bits: magnitudes m/8 for exponent 0 and
 *   (1 + m/8) 2^(e-1) otherwise, up to 7.5; no NaN, no infinity.  Scales are e8m0 bytes, row-major (flat).
 *   y = x_g . h exactly as qutlass_amd_fused_quantize_mxf8 computes it; rot in {32, 64, 128}.  Then for every 32 consecutive y:
 *       amax = max |y|  (NaNs ignored)          E = the biased exponent field of the FP32 amax
 *       e8   = 255 if any of the 32 y is NaN or infinite -- all 32 codes are then 0, the NaN travels in the scale byte, which the GEMM honours;
 *              127 if amax == 0; else clamp(E - 2, 0, 254)                                               -- the OCP MX rule: the scaled maximum lies in [4, 8)
 *       q    = min(RNE(|y| * 2^(127 - e8)) on the e2m3 grid, 7.5) with the sign of y                     -- ties to the even code; (7.5, 8) saturates on purpose;
 *              -0 and negative values that round to zero keep their sign
 *   Abs-max only; no clip mask, no global scale, flat scales only (the first numel / 32 bytes of out_e8m0).  out_fp6: numel * 3 / 4 bytes.
 * qutlass_amd_fused_gather_quantize_mxf6 = the plain entry on x[src_row] (an index outside [0, t) gives a zero row: codes 0, scale 127), byte for byte, with the
 * siblings' limits: x below 2 GiB, numel < 2^31.
 * Checks: each entry runs its MX sibling's chain in the sibling's order under the name fusedQuantizeMxf6 / fusedGatherQuantizeMxf6 (there is no method and no fmt to
 * reject); all before any HIP call.
 */
int qutlass_amd_fused_quantize_mxf6(const void* x, const void* h, int rot, int64_t numel, void* out_fp6, void* out_e8m0, void* stream);
int qutlass_amd_fused_gather_quantize_mxf6(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, void* out_fp6,
                                           void* out_e8m0, void* stream);

/*
 * EXTENSION (no reference counterpart): MoE routing, the step in front of the dispatch above -- router logits to expert ids and weights, and expert ids to the
 * sorted-row metadata the gathering quantizers, the grouped GEMMs and moe_combine read.  Every argument check happens before any HIP call.
 *
 * qutlass_amd_moe_topk_softmax: logits (t, e), contiguous, bf16 (elem_bytes 2) or float32 (4) -> weights (t, topk) float32 and ids (t, topk) int32.
 *   selection  the first topk experts in the order (logit descending, expert index ascending), ids[t] in that order; logits compare as floating-point numbers
 *              (-0 and +0 tie, the lower index wins); -inf is legal and sorts last.  Made on the logits, never on the probabilities.
 *   weights    fp32: m = max_j x_j, e_j = exp(x_j - m), p_j = e_j / sum_j e_j; renormalize != 0: w_k = p_k / sum over the selected p.  The order of the sums is not
 *              part of the contract.  A row holding a NaN or +inf, or nothing but -inf, gets unspecified weights; its ids are still distinct and in [0, e), and no
 *              other row is affected.
 *   1 <= e <= 1024, 1 <= topk <= min(e, 32), t < 2^31; pointers aligned to their element size (rows that start on 16-byte boundaries are read with 16-byte
 *   loads).  One launch, one wave per token, no workspace, no host sync.  t == 0 returns QAMD_OK without a launch.
 *
 * qutlass_amd_moe_sort: topk_ids (t, topk), int32 (id_bytes 4) or int64 (8) -> src_row (t * topk), offs (num_experts), pos (t, topk), all int32: a STABLE sort of
 * the n = t * topk slots by expert.
 *   key        the slot's id g; with expert_map (g_entries int32, or NULL for none): expert_map[g] for g in [0, g_entries), dropped otherwise WITHOUT reading the
 *              map.  A key outside [0, num_experts) -- -1 by convention, an expert of another rank -- DROPS the slot.
 *   src_row    the token (slot / topk) of every sorted row: rows ordered by expert, within an expert by slot; dropped slots behind every real expert
 *   offs       the cumulative END rows of the experts (the grouped GEMMs' convention); dropped slots are not counted
 *   pos        the sorted row of every slot, -1 where it was dropped
 *   A counting sort without atomics: the result does not depend on the launch geometry or on timing, and no workgroup waits on another.  Up to the one-launch
 *   bound (qutlass_amd_moe_sort_workspace_bytes(n, .) == 0) it is ONE launch of one workgroup; beyond it three launches (count, scan, scatter) over `workspace`,
 *   which must hold qutlass_amd_moe_sort_workspace_bytes(n, num_experts) bytes, 4-byte aligned (never more than 257 * 1025 * 4 bytes); its contents need not be
 *   initialised and are not kept.  1 <= num_experts <= 1024, topk >= 1, n < 2^31.  n == 0 returns QAMD_OK without a launch and writes nothing: the caller
 *   zero-fills offs (an empty sort has every offset at 0).
 */
int qutlass_amd_moe_topk_softmax(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int renormalize, float* weights, int32_t* ids,
                                 void* stream);

/*
 * EXTENSION: the grouped router of DeepSeek-V2 / V3 and Kimi-K2 -- scores, a selection bias, a top-k over the experts of the best groups -- in one launch, on
 * moe_topk_softmax's skeleton.  logits (t, e), contiguous, bf16 (elem_bytes 2) or float32 (4) -> weights (t, topk) float32, ids (t, topk) int32 and, with scores
 * != NULL, scores (t, e) float32.  All arithmetic is fp32.  x is a row, G = n_group, S = e / G.
 *   scores     scoring QAMD_MOE_SCORING_SIGMOID: s_j = 1 / (1 + exp(-x_j)) (-inf gives 0, +inf gives 1); QAMD_MOE_SCORING_SOFTMAX: moe_topk_softmax's p_j
 *              (m = max, e_j = exp(x_j - m), p_j = e_j / sum e).  The order of the sum is not part of the contract.
 *   choice     c_j = s_j + bias_j (one fp32 add, round to nearest) with a bias -- (e) float32, every entry finite or -inf --, c_j = s_j with bias == NULL.
 *              c alone decides what is selected; the bias never reaches a weight.
 *   groups     (G > 1) group g is the experts [g * S, (g + 1) * S).  Its score is the sum of its two largest c (one fp32 add; a group of one expert scores that
 *              value) with a bias, its largest c without.  The first topk_group groups in the order (score descending, group index ascending) survive; the
 *              experts of the others are NOT candidates, whatever the sign of c (a -inf mask, not a zero fill).
 *   selection  the first topk candidates in the order (c descending, expert index ascending), ids[t] in that order; c compares as a floating-point number
 *              (-0 and +0 tie).  Made on c, NOT on the logits: with a bias the two orders differ, and that is the point.
 *   weights    w_k = s_{id_k}; renormalize != 0: w_k = w_k / sum over the selected w (the order of the sum is free; a row whose selected scores sum to 0 gets
 *              unspecified weights); last w_k = w_k * routed_scaling_factor (one fp32 multiply).
 *   scores     the s_j the kernel selected on, bit for bit; asking for them changes no bit of ids or weights.
 * A row holding a NaN, or a +inf + -inf in the choice or the group score, gets unspecified weights; its ids are still distinct and in [0, e), and no other row is
 * affected.  1 <= e <= 1024, 1 <= n_group <= 64, e % n_group == 0, 1 <= topk_group <= n_group, 1 <= topk <= min(32, topk_group * S), t < 2^31; pointers aligned
 * to their element size (16-byte loads and stores where every row starts on a 16-byte boundary; same bits either way).  One launch, one wave per token, no
 * workspace, no host sync.  Every argument check happens before any HIP call.  t == 0 returns QAMD_OK without a launch.
 */
#define QAMD_MOE_SCORING_SIGMOID 0
#define QAMD_MOE_SCORING_SOFTMAX 1
int qutlass_amd_moe_topk_grouped(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int64_t n_group, int64_t topk_group, int scoring,
                                 const float* bias /* nullable */, int renormalize, float routed_scaling_factor, float* weights, int32_t* ids,
                                 float* scores /* nullable */, void* stream);
int64_t qutlass_amd_moe_sort_workspace_bytes(int64_t n, int64_t num_experts);
int qutlass_amd_moe_sort(const void* topk_ids, int id_bytes, int64_t t, int64_t topk, int64_t num_experts, const int32_t* expert_map, int64_t g_entries,
                         int32_t* src_row, int32_t* offs, int32_t* pos, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * EXTENSION: the whole routing of a decode step in ONE launch of one workgroup: qutlass_amd_moe_topk_softmax (respectively qutlass_amd_moe_topk_grouped without
 * scores) followed by qutlass_amd_moe_sort on the ids it returns, with the same five results bit for bit -- the kernels run the routers' and the sort's own device
 * code, and the sort reads its keys from LDS where the router left them instead of reading ids back from memory.
 *   arguments  those of the matching moe_topk entry without `scores`, then num_experts, expert_map (nullable), g_entries, src_row, offs, pos of
 *              qutlass_amd_moe_sort.  No workspace.
 *   limits     0 <= t <= 64; every other limit and every argument check is the two entries' (made before any HIP call); an expert_map has at least one entry.
 *              t > 64 returns QAMD_ERR_INVALID: run the two entries instead.  t == 0 returns QAMD_OK without a launch and writes nothing (the caller zero-fills offs).
 * These entries ALWAYS run the one launch.  qutlass_amd_moe_route_fused_max_tokens() is the measured bound, in [0, 64], up to which that is the faster form on an
 * MI355X for every router measured; the torch ops qutlass_amd::moe_route_fused / moe_route_grouped_fused take the one launch up to it and the
 * two entries beyond.
 */
int64_t qutlass_amd_moe_route_fused_max_tokens(void);
int qutlass_amd_moe_route_fused(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int renormalize, float* weights, int32_t* ids,
                                int64_t num_experts, const int32_t* expert_map /* nullable */, int64_t g_entries, int32_t* src_row, int32_t* offs, int32_t* pos,
                                void* stream);
int qutlass_amd_moe_route_grouped_fused(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int64_t n_group, int64_t topk_group, int scoring,
                                        const float* bias /* nullable */, int renormalize, float routed_scaling_factor, float* weights, int32_t* ids,
                                        int64_t num_experts, const int32_t* expert_map /* nullable */, int64_t g_entries, int32_t* src_row, int32_t* offs,
                                        int32_t* pos, void* stream);

/*
 * EXTENSION: the measured launch-count rule of the activation path y = Q(x h) W^T of one linear layer (reference flow: qutlass/__init__.py:149-180 ->
 * qutlass/utils.py:160-193 -> qutlass/__init__.py:34-76, three launches): returns 1 where the one-launch decode kernel below wins (M <= 16, R = 32, short K,
 * a weight of fewer than 32 x CUs rows), else 2 (quantizer with GEMM-ready scales + GEMM).  Pure host arithmetic on the current device's CU count; what
 * qutlass_amd.fused_quantize_matmul_mxf4_bf16_tn (Python) asks before it launches, so that a C caller gets the same rule.
 */
int qutlass_amd_activation_path_launches(int64_t M, int64_t N, int64_t K, int rot);

/*
 * EXTENSION: the whole decode-time activation path in ONE launch, for batches of at most 32 rows:
 *     D[M,N] (bf16) = alpha[0] * Q(x . h) (B . SFB)^T
 * x: (M, K) bf16 activations, h: 32 x 32 bf16 rotation (rot must be 32), method as above; B / B_sf: the MXFP4 weight and its
 * to_blocked e8m0 scales exactly as qutlass_amd_matmul_mxf4_bf16_tn takes them.  K % 128 == 0, N % 8 == 0, 1 <= M <= 32.
 * Bit-identical to qutlass_amd_fused_quantize_mx + qutlass_amd_to_blocked + qutlass_amd_matmul_mxf4_bf16_tn on the same
 * inputs (the three launches of qutlass/__init__.py:149-180, qutlass/utils.py:160-193, qutlass/__init__.py:34-76).
 */
int qutlass_amd_fused_quantize_matmul_mxf4_bf16_tn(const void* x, const void* h, int rot, int method, const void* B,
                                                   const void* B_sf, const float* alpha, void* D, int64_t M, int64_t N,
                                                   int64_t K, void* stream);

/* ---- QAT-backward data preparation ------------------------------------- */

/*
 * Input contract of the four ops below (and of the forward quantizers): FINITE operands.  What the reference's kernels do with NaN / inf
 * follows from the order of its fmaxf chains and is not a documented behaviour; here
 *   - backward_t_bf16 / backward_qt_bf16 reproduce the reference's arithmetic for the cases its own data can reach (all-zero groups:
 *     3 / 0 = inf, 0 * inf = NaN -> code 7; scales outside the division-free range take the reference's divisions), tests pin them;
 *   - backward_bf16_square_double_mxfp8 and mxfp4_transpose_mxfp8 take the block maximum on sign-stripped bf16 bit patterns: a NaN or inf
 *     element (or an input e8m0 byte of 255) becomes the block maximum, where an fmaxf chain would have skipped a NaN;
 *   - an input e8m0 byte of 0 (2^-127: the dequantised bf16 operand is a denormal) is outside what the MFMA rotation reproduces exactly
 *     (the matrix core flushes bf16 denormals); the forward quantizers never emit it for a non-zero group.
 * All four are deterministic and bit-stable across devices (no plan depends on the CU count in a way that changes arithmetic order).
 */

/*
 * x: bf16 (B, N, M) row-major; h: bf16 32 x 32.  For every (b, m) and every 32-group g along N:
 * y = x[b, 32g..32g+31, m] . h, abs-max MXFP4 (no epsilon, x3 before rounding).  out_e2m1: (B, M, N/2) bytes,
 * out_e8m0: (B, M, N/32) bytes.  N % 32 == 0, M % 8 == 0.
 * Replaces backward_t_bf16_cuda (qutlass/csrc/quartet_bwd_sm120.cu:237-325,430-454; include/backward_host.h:17-26;
 * bindings.cpp:429-443).
 */
int qutlass_amd_backward_t_bf16(const void* x, const void* h, int64_t B, int64_t N, int64_t M, void* out_e2m1,
                                void* out_e8m0, void* stream);

/*
 * The same on an MXFP4 operand: x_e2m1 (B, N, M/2) bytes, x_e8m0 (B, N, M/32); alpha: device fp32[1] (enters the
 * scale only: e8m0 = floor_pow2(amax / alpha), q = y * 3 / (scale * alpha)).  N % 32 == 0, M % 32 == 0.
 * Replaces backward_qt_bf16_cuda (quartet_bwd_sm120.cu:327-428,457-483; backward_host.h:4-15; bindings.cpp:445-464).
 */
int qutlass_amd_backward_qt_bf16(const void* x_e2m1, const void* x_e8m0, const void* h, const float* alpha, int64_t B,
                                 int64_t N, int64_t M, void* out_e2m1, void* out_e8m0, void* stream);

/*
 * x: bf16 (m, n).  One shared exponent per 32 x 32 block (floor(log2 amax) - 7, 127 for an all-zero block);
 * y: e4m3 (m, n); row_scales: e8m0 (m, n/32); col_scales: e8m0 (n, m/32).  m % 128 == 0 and n % 128 == 0 (the
 * reference wrapper pads m to 128 and launches n/128 blocks, qutlass/__init__.py:288-297, quartet_bwd_sm120.cu:596).
 * Replaces backward_bf16_square_double_mxfp8_cuda (quartet_bwd_sm120.cu:511-621; bindings.cpp:466-479).
 */
int qutlass_amd_backward_bf16_square_double_mxfp8(const void* x, int64_t m, int64_t n, void* y, void* row_scales,
                                                  void* col_scales, void* stream);

/*
 * x_fp4: packed e2m1 (m, n/2), scales: e8m0 (m, n/32).  y: e4m3 (n, m) = requantised transpose with one shared
 * exponent per 32 along m; out_e8m0: (n, m/32).  m % 128 == 0, n % 256 == 0 (the reference pads m to 256 and launches
 * n/256 blocks, __init__.py:299-315, quartet_bwd_sm120.cu:716).
 * Replaces mxfp4_transpose_mxfp8_cuda (quartet_bwd_sm120.cu:628-733; bindings.cpp:481-494).
 */
int qutlass_amd_mxfp4_transpose_mxfp8(const void* x_fp4, const void* scales, int64_t m, int64_t n, void* y,
                                      void* out_e8m0, void* stream);

/*
 * The same two ops for ANY row count m: the outputs are laid out for m_pad rows (a multiple of 128 >= m; the reference's
 * wrappers use ceil(m / 128) * 128 resp. ceil(m / 256) * 256) and rows m .. m_pad-1 of the input are treated as zeros (zero codes
 * with unit scales for the MXFP4 input) INSIDE the kernel.  The reference materialises that padding with
 * torch.nn.functional.pad -- a full extra copy of the operand -- and, for mxfp4_transpose_mxfp8, by writing 1.0 into rows
 * m .. m_pad-1 of the CALLER's scale tensor (qutlass/__init__.py:288-307, its own "TODO: padding in kernel"); here x / x_fp4 /
 * scales are read-only and only need their m real rows.  With m_pad == m these ARE the entries above.
 * y: (m_pad, n) resp. (n, m_pad); row_scales (m_pad, n/32), col_scales (n, m_pad/32); out_e8m0 (n, m_pad/32).
 */
int qutlass_amd_backward_bf16_square_double_mxfp8_rows(const void* x, int64_t m, int64_t m_pad, int64_t n, void* y,
                                                       void* row_scales, void* col_scales, void* stream);
int qutlass_amd_mxfp4_transpose_mxfp8_rows(const void* x_fp4, const void* scales, int64_t m, int64_t m_pad, int64_t n,
                                           void* y, void* out_e8m0, void* stream);

/* ---- block-scale swizzle ------------------------------------------------------------------------ */

/*
 * in: (rows, cols) row-major 1-byte elements; out: ceil(rows/128)*128 * ceil(cols/4)*4 bytes in the
 * 128x4 tiled order, zero padded.  Replaces qutlass/utils.py:160-193 (to_blocked) incl. the Triton
 * kernel at :16-133.
 */
int qutlass_amd_to_blocked(const void* in, int64_t rows, int64_t cols, void* out, void* stream);

/* ---- misc ----------------------------------------------------------------------------------------- */

const char* qutlass_amd_last_error(void);
const char* qutlass_amd_version(void);

/*
 * libqutlass_amd.so has NO options: this entry returns -1 for every key -- nothing a caller or another thread does can change which
 * kernel a shape gets or what it computes.  (The lab build of the same sources, libqutlass_amd_bench.so -- test and bench
 * infrastructure, see INTEGRATION.md -- accepts "gemm_variant", "nvf4_variant", "pp_flags", "splitk_wg", "splitk_min_kt",
 * "splitk_force", "transpose_nc", "quant_wg_per_cu", "pp_shift", "deepp_grid" and "hw_fp4_cvt" (0 = the software e2m1 encoder instead of
 * v_cvt_scalef32_pk_fp4_f32: same bits, tests/test_gpu_parity.py) and returns the previous value.)
 */
int qutlass_amd_set_option(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* QUTLASS_AMD_H_ */
