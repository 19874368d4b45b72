// PyTorch (ROCm) extension: the `_qutlass_C` operator library of the reference, bound to the C ABI of
// libqutlass_amd.so (include/qutlass_amd.h).  No device code here -- the kernels are the hand-written HIP in
// gemm_*.hip.h / quantize.hip.h / to_blocked.hip.h behind the C ABI.
//
// Mirrors qutlass/csrc/bindings.cpp of the reference op for op: same op names and schema strings
// (bindings.cpp:499-513), same argument validation order and messages (bindings.cpp:32-426,
// include/bindings_utils.h:67-136), same ownership (GEMMs allocate and return the bf16 result, quantizers fill
// caller-allocated outputs and return them), same stream rule (current stream of the tensor's device,
// include/common.h:40-45).  Written against the LibTorch stable ABI, like the reference, so one build serves
// every torch >= 2.10.  One extra op, qutlass_amd::to_blocked, replaces the Triton/torch swizzle of
// qutlass/utils.py:160-193.
//
// Built as qutlass/_CUDA.abi3.so: like the reference's op library it is a Python extension module (PyInit__CUDA,
// include/registration.h + bindings.cpp:537-540) whose import -- or a plain dlopen through torch.ops.load_library --
// runs the static registrations; `_qutlass_C` is opened as a FRAGMENT and implemented for the CUDA dispatch key only
// (bindings.cpp:498, :516), so a CPU tensor gets the dispatcher's own "not implemented for the CPU backend" error.
#include <Python.h>

#include <torch/csrc/inductor/aoti_torch/c/shim.h>
#include <torch/csrc/stable/accelerator.h>
#include <torch/csrc/stable/library.h>
#include <torch/csrc/stable/ops.h>
#include <torch/csrc/stable/tensor.h>
#include <torch/headeronly/core/ScalarType.h>
#include <torch/headeronly/util/Exception.h>

#include <initializer_list>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/qutlass_amd.h"

namespace {

using torch::headeronly::ScalarType;
using torch::stable::Tensor;

struct Named {
  const Tensor& t;
  const char* name;
};

std::string arg_desc(int pos, const char* name) { return "argument #" + std::to_string(pos) + " '" + name + "'"; }

// ---- the three generic checks of include/bindings_utils.h, once per op, in the reference's order ------------------------------------------
// Every tensor of `args` contiguous (argument numbers count from 0); then every tensor of `args` and of `device_only` -- tensors that need not be contiguous: a
// one-element alpha or global scale -- on a GPU; then all of them on the device of the first (numbers count through both lists).  same_gpu false: no third pass
// (the QAT-backward ops, as the reference).  head: the tensor the third pass compares with where it is not args[0] -- an optional tensor is checked on its own,
// against the op's first tensor as argument #0.
// Lists: braced lists of {tensor, name} (the default: a braced argument deduces nothing), or std::vector<Named> where a list is put together at run time
using Args = std::initializer_list<Named>;

template <class List = Args, class DeviceOnly = Args>
void check_tensors(const char* op, const List& args, const DeviceOnly& device_only = {}, bool same_gpu = true, const Named* head = nullptr) {
  int pos = 0;
  for (const Named& a : args) {
    STD_TORCH_CHECK(a.t.is_contiguous(), "Expected contiguous tensor, but got non-contiguous tensor for ", arg_desc(pos, a.name),
                    " (while checking arguments for ", op, ")");
    ++pos;
  }
  const auto on_gpu = [op](const Named& a) {
    STD_TORCH_CHECK(a.t.is_cuda(), "Expected tensor to have cuda DeviceType, but got tensor with ", a.t.is_cpu() ? "cpu" : "another",
                    " DeviceType (while checking arguments for ", op, ")");
  };
  for (const Named& a : args) on_gpu(a);
  for (const Named& a : device_only) on_gpu(a);
  if (!same_gpu) return;
  const Named& first = head ? *head : *args.begin();
  pos = head ? 1 : 0;
  const auto same = [op, &first, &pos](const Named& a) {
    if (pos > 0)
      STD_TORCH_CHECK(a.t.get_device_index() == first.t.get_device_index(), "Expected tensor for ", arg_desc(0, first.name),
                      " to have the same device as tensor for ", arg_desc(pos, a.name), "; but device ", first.t.get_device_index(),
                      " does not equal ", a.t.get_device_index(), " (while checking arguments for ", op, ")");
    ++pos;
  };
  for (const Named& a : args) same(a);
  for (const Named& a : device_only) same(a);
}

// dtype through the C shim: Tensor::scalar_type() goes through the stable IValue conversion, which in torch 2.10 does
// not know Float8_e8m0fnu yet ("Not yet supported ScalarType 44")
bool has_dtype(const Tensor& t, ScalarType want) {
  int32_t code = -1;
  TORCH_ERROR_CODE_CHECK(aoti_torch_get_dtype(t.get(), &code));
  return code == static_cast<int32_t>(want);
}

void* current_stream(const Tensor& t) {   // include/common.h:40-45
  void* s = nullptr;
  TORCH_ERROR_CODE_CHECK(aoti_torch_get_current_cuda_stream(t.get_device_index(), &s));
  return s;
}

void check_rc(int rc) { STD_TORCH_CHECK(rc == QAMD_OK, qutlass_amd_last_error()); }

// ---- block-scaled GEMMs --------------------------------------------------------------------------------------------
// scratch of a GEMM, from torch's stream-ordered caching allocator: 0 bytes -- the shape needs none -- allocate nothing and give a null pointer
struct Workspace {
  int64_t bytes;
  Tensor t;
  Workspace(const Tensor& like, int64_t n) : bytes(n), t(n > 0 ? torch::stable::new_empty(like, {n}, ScalarType::Byte) : Tensor()) {}
  void* ptr() const { return bytes > 0 ? t.data_ptr() : nullptr; }
};

enum class Gemm { MXF4, NVF4, MXF8_TN, MXF8_NN, ADA_MXF4 };

template <Gemm G>
Tensor matmul(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha) {
  constexpr bool fp8 = G == Gemm::MXF8_TN || G == Gemm::MXF8_NN;
  constexpr bool nn = G == Gemm::MXF8_NN;
  const char* op = G == Gemm::ADA_MXF4 ? "matmul_ada_mxf4_bf16_tn" : G == Gemm::MXF4 ? "matmul_mxf4_bf16_tn" : G == Gemm::NVF4 ? "matmul_nvf4_bf16_tn" : G == Gemm::MXF8_TN ? "matmul_mxf8_bf16_tn" : "matmul_mxf8_bf16_nn";
  if (fp8) check_tensors(op, {{A, "A"}, {B, "B"}, {A_sf, "A_sf"}, {B_sf, "B_sf"}, {alpha, "alpha"}});
  else check_tensors(op, {{A, "A"}, {B, "B"}, {A_sf, "A_sf"}, {B_sf, "B_sf"}}, {{alpha, "alpha"}});   // (the reference's FP4 GEMMs do not ask for a contiguous alpha)

  const ScalarType data_t = fp8 ? ScalarType::Float8_e4m3fn : ScalarType::Byte;
  const ScalarType sf_t = G == Gemm::NVF4 ? ScalarType::Float8_e4m3fn : ScalarType::Float8_e8m0fnu;
  const char* data_n = fp8 ? "float8_e4m3fn" : "uint8";
  const char* sf_n = G == Gemm::NVF4 ? "float8_e4m3fn" : "float8_e8m0fnu";
  // EXTENSION over the reference (which accepts e4m3 only, bindings.cpp:157-160, 196-199): the A operand of the MXFP8 GEMMs
  // may be float8_e5m2 -- the gradient operand of a QAT backward GEMM (BASELINE.json configs[4]); B stays e4m3.
  const bool a_e5m2 = fp8 && has_dtype(A, ScalarType::Float8_e5m2);
  STD_TORCH_CHECK(has_dtype(A, data_t) || a_e5m2, "A must be ", data_n, fp8 ? " (or float8_e5m2)" : "");
  STD_TORCH_CHECK(has_dtype(B, data_t), "B must be ", data_n);
  STD_TORCH_CHECK(has_dtype(A_sf, sf_t), "A_sf must be ", sf_n);
  STD_TORCH_CHECK(has_dtype(B_sf, sf_t), "B_sf must be ", sf_n);
  STD_TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "A and B must be 2D");
  const int64_t kmin = G == Gemm::NVF4 ? 16 : 32;
  int64_t M;
  if (nn) {
    STD_TORCH_CHECK(A.size(0) == B.size(1), "Inner dimensions must match for A.T @ B.T");
    STD_TORCH_CHECK(A.size(0) >= kmin, "A K-dim must be >= ", kmin);
    M = A.size(1);
  } else {
    STD_TORCH_CHECK(A.size(1) == B.size(1), "Inner dimensions must match for A @ B.T");
    STD_TORCH_CHECK(A.size(1) >= kmin, "A K-dim must be >= ", kmin);
    M = A.size(0);
  }
  STD_TORCH_CHECK(B.size(1) >= kmin, "B K-dim must be >= ", kmin);
  const int64_t N = B.size(0), K = B.size(1) * (fp8 ? 1 : 2);
  // the kernels read alpha as one fp32 and the scale operands through descriptors sized from M / N / K: make sure the
  // tensors are at least that large (the reference leaves both to CUTLASS' can_implement / the caller); checked before the
  // empty-shape return so that a malformed argument fails whatever the batch size
  STD_TORCH_CHECK(has_dtype(alpha, ScalarType::Float) && alpha.numel() >= 1, "alpha must be a float32 tensor with at least one element");
  {
    const int64_t gs = G == Gemm::NVF4 ? 16 : 32, kb = K / gs;
    const bool row_major_sf = G == Gemm::ADA_MXF4;   // un-swizzled (rows, K/32); every other op: to_blocked layout of the padded matrix
    const int64_t need_a = row_major_sf ? M * kb : (M + 127) / 128 * 128 * ((kb + 3) / 4 * 4);
    const int64_t need_b = row_major_sf ? N * kb : (N + 127) / 128 * 128 * ((kb + 3) / 4 * 4);
    STD_TORCH_CHECK(A_sf.numel() >= need_a, "A_sf has ", A_sf.numel(), " elements, the ", row_major_sf ? "row-major" : "blocked", " scale layout of A needs ", need_a);
    STD_TORCH_CHECK(B_sf.numel() >= need_b, "B_sf has ", B_sf.numel(), " elements, the ", row_major_sf ? "row-major" : "blocked", " scale layout of B needs ", need_b);
  }
  Tensor out = torch::stable::new_empty(A, {M, N}, ScalarType::BFloat16);
  if (M == 0 || N == 0) return out;   // empty batch / empty weight: nothing to launch (the C ABI requires positive extents)

  const torch::stable::accelerator::DeviceGuard guard(A.get_device_index());
  const float* al = static_cast<const float*>(alpha.data_ptr());
  void* s = current_stream(A);
  int rc;
  if (G == Gemm::ADA_MXF4) rc = qutlass_amd_matmul_ada_mxf4_bf16_tn(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, out.data_ptr(), M, N, K, s);
  else if (G == Gemm::MXF4 || G == Gemm::MXF8_TN) {
    // small outputs with a long K split K over scratch (the reference allocates its CUTLASS workspace per call as well, gemm.cu:160-162); 0 bytes = the shape does not split
    const Workspace ws(A, qutlass_amd_gemm_splitk_workspace_bytes(fp8 ? 8 : 4, M, N, K));
    rc = fp8 ? qutlass_amd_matmul_mxf8_bf16_tn_fmt(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, out.data_ptr(), M, N, K,
                                                   a_e5m2 ? QAMD_FP8_E5M2 : QAMD_FP8_E4M3, QAMD_FP8_E4M3, ws.ptr(), ws.bytes, s)
             : qutlass_amd_matmul_mxf4_bf16_tn_ws(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, out.data_ptr(), M, N, K, ws.ptr(), ws.bytes, s);
  }
  else if (G == Gemm::NVF4) {
    // [r3] the same for NVFP4: outputs of a few dozen 128x128 tiles with a long K split K (M = 256, N = 4096, K = 14336: 54.7 -> 39.2 us)
    const Workspace ws(A, qutlass_amd_nvf4_splitk_workspace_bytes(M, N, K));
    rc = qutlass_amd_matmul_nvf4_bf16_tn_ws(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, out.data_ptr(), M, N, K, ws.ptr(), ws.bytes, s);
  }
  else {
    // scratch for the (K, M) -> (M, K) re-layout of small problems; shapes that read the (K, M) operand in place need none
    const Workspace ws(A, qutlass_amd_mxf8_nn_workspace_bytes_for(M, N, K));
    rc = qutlass_amd_matmul_mxf8_bf16_nn_fmt(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, out.data_ptr(), M, N, K,
                                             a_e5m2 ? QAMD_FP8_E5M2 : QAMD_FP8_E4M3, QAMD_FP8_E4M3, ws.ptr(), ws.bytes, s);
  }
  check_rc(rc);
  return out;
}

// EXTENSION: grouped GEMMs for mixture-of-experts layers (qutlass_amd_grouped_matmul_{mxf4,nvf4,mxf8}_bf16_tn).  A tokens sorted by expert, B (E, N, ...) stacked expert
// weights, row-major scales, alpha of 1 or E elements, offs int32 (E,) cumulative end rows.  Rows at or past offs[E-1] are not written (left as allocated).
//   MXF4: A (M, K/2), B (E, N, K/2), e8m0 scales per 32 elements
//   NVF4: the same operands, e4m3 scales per 16 elements (fusedQuantizeNv's buffer as it is)
//   MXF8: A (M, K) e4m3 / e5m2 (e5m2 selects the e5m2-A path, as matmul_mxf8_bf16_tn), B (E, N, K) e4m3, e8m0 scales per 32 elements
//   MXF8_MXF4 (W4A8): A (M, K) e4m3 as MXF8's, B (E, N, K/2) packed e2m1 as MXF4's, e8m0 scales per 32 elements
//   MXF6_MXF4 (W4A6): A (M, 3K/4) uint8, packed e2m3 codes (include/qutlass_amd.h: the MXFP6 operand format), B and the scales as MXF8_MXF4's
enum class Grouped { MXF4, NVF4, MXF8, MXF8_MXF4, MXF6_MXF4 };

template <Grouped G>
Tensor grouped_matmul(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs) {
  constexpr bool w4a8 = G == Grouped::MXF8_MXF4;
  constexpr bool fp8 = G == Grouped::MXF8;
  constexpr bool w4a6 = G == Grouped::MXF6_MXF4;
  const char* op = G == Grouped::MXF4 ? "grouped_matmul_mxf4" : G == Grouped::NVF4 ? "grouped_matmul_nvf4" : w4a8 ? "grouped_matmul_mxf8_mxf4" : w4a6 ? "grouped_matmul_mxf6_mxf4" : "grouped_matmul_mxf8";
  check_tensors(op, {{A, "A"}, {B, "B"}, {A_sf, "A_sf"}, {B_sf, "B_sf"}, {alpha, "alpha"}, {offs, "offs"}});
  const ScalarType data_t = fp8 ? ScalarType::Float8_e4m3fn : ScalarType::Byte;                  // either operand
  const ScalarType a_alt = fp8 ? ScalarType::Float8_e5m2 : ScalarType::Float4_e2m1fn_x2;         // ... or, for A
  const ScalarType b_alt = fp8 ? ScalarType::Float8_e4m3fn : ScalarType::Float4_e2m1fn_x2;       // ... for B (MXF8: e4m3 only)
  const ScalarType sf_t = G == Grouped::NVF4 ? ScalarType::Float8_e4m3fn : ScalarType::Float8_e8m0fnu;
  const char* sf_n = G == Grouped::NVF4 ? "float8_e4m3fn" : "float8_e8m0fnu";
  if (w4a8) {   // e4m3 tokens only (e5m2 tokens have no W4A8 kernel), the weights as MXF4's
    STD_TORCH_CHECK(!has_dtype(A, ScalarType::Float8_e5m2), op, ": A must be float8_e4m3fn, float8_e5m2 tokens are not supported");
    STD_TORCH_CHECK(has_dtype(A, ScalarType::Float8_e4m3fn), op, ": A must be float8_e4m3fn");
    STD_TORCH_CHECK(has_dtype(B, ScalarType::Byte) || has_dtype(B, ScalarType::Float4_e2m1fn_x2), op, ": B must be uint8 or float4_e2m1fn_x2");
  } else if (w4a6) {   // packed e2m3 tokens have no dtype of their own: bytes; the weights as MXF4's
    STD_TORCH_CHECK(has_dtype(A, ScalarType::Byte), op, ": A must be uint8 (packed e2m3 codes)");
    STD_TORCH_CHECK(has_dtype(B, ScalarType::Byte) || has_dtype(B, ScalarType::Float4_e2m1fn_x2), op, ": B must be uint8 or float4_e2m1fn_x2");
  } else {
    STD_TORCH_CHECK(has_dtype(A, data_t) || has_dtype(A, a_alt), "A must be ", fp8 ? "float8_e4m3fn or float8_e5m2" : "uint8 or float4_e2m1fn_x2");
    STD_TORCH_CHECK(has_dtype(B, data_t) || has_dtype(B, b_alt), "B must be ", fp8 ? "float8_e4m3fn" : "uint8 or float4_e2m1fn_x2");
  }
  STD_TORCH_CHECK(has_dtype(A_sf, sf_t), "A_sf must be ", sf_n);
  STD_TORCH_CHECK(has_dtype(B_sf, sf_t), "B_sf must be ", sf_n);
  STD_TORCH_CHECK(A.dim() == 2 && B.dim() == 3, w4a6 ? "A must be 2D (M, 3K/4) and B 3D (E, N, K/2)" : w4a8 ? "A must be 2D (M, K) and B 3D (E, N, K/2)" : fp8 ? "A must be 2D (M, K) and B 3D (E, N, K)" : "A must be 2D (M, K/2) and B 3D (E, N, K/2)");
  STD_TORCH_CHECK(w4a6 ? A.size(1) * 2 == B.size(2) * 3 : A.size(1) == B.size(2) * (w4a8 ? 2 : 1), "Inner dimensions must match for A @ B[g].T");
  const int64_t M = A.size(0), E = B.size(0), N = B.size(1), K = w4a6 ? B.size(2) * 2 : A.size(1) * (fp8 || w4a8 ? 1 : 2), kb = K / (G == Grouped::NVF4 ? 16 : 32);
  STD_TORCH_CHECK(E >= 1 && E <= 1024, "the number of experts must be in [1, 1024] (got ", E, ")");
  STD_TORCH_CHECK(has_dtype(offs, ScalarType::Int) && offs.numel() == E, "offs must be an int32 tensor of E = ", E, " elements");
  STD_TORCH_CHECK(has_dtype(alpha, ScalarType::Float) && (alpha.numel() == 1 || alpha.numel() == E), "alpha must be a float32 tensor of 1 or E = ", E, " elements");
  STD_TORCH_CHECK(A_sf.numel() >= M * kb, "A_sf has ", A_sf.numel(), " elements, the row-major scale layout of A needs ", M * kb);
  STD_TORCH_CHECK(B_sf.numel() >= E * N * kb, "B_sf has ", B_sf.numel(), " elements, the row-major scale layout of B needs ", E * N * kb);
  Tensor out = torch::stable::new_empty(A, {M, N}, ScalarType::BFloat16);
  if (M == 0 || N == 0) return out;   // empty batch: nothing to launch

  const torch::stable::accelerator::DeviceGuard guard(A.get_device_index());
  const float* al = static_cast<const float*>(alpha.data_ptr());
  const int32_t* of = static_cast<const int32_t*>(offs.data_ptr());
  void* s = current_stream(A);
  int rc;
  if (G == Grouped::MXF4) rc = qutlass_amd_grouped_matmul_mxf4_bf16_tn(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, alpha.numel(), of, out.data_ptr(), M, N, K, E, s);
  else if (G == Grouped::NVF4) rc = qutlass_amd_grouped_matmul_nvf4_bf16_tn(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, alpha.numel(), of, out.data_ptr(), M, N, K, E, s);
  else if (w4a6) rc = qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, alpha.numel(), of, out.data_ptr(), M, N, K, E, s);
  else if (w4a8) rc = qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, alpha.numel(), of, out.data_ptr(), M, N, K, E, s);
  else rc = qutlass_amd_grouped_matmul_mxf8_bf16_tn(A.data_ptr(), B.data_ptr(), A_sf.data_ptr(), B_sf.data_ptr(), al, alpha.numel(), of, out.data_ptr(), M, N, K, E,
                                                    has_dtype(A, ScalarType::Float8_e5m2) ? QAMD_FP8_E5M2 : QAMD_FP8_E4M3, s);
  check_rc(rc);
  return out;
}

Tensor grouped_matmul_mxf4(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs) { return grouped_matmul<Grouped::MXF4>(A, B, A_sf, B_sf, alpha, offs); }
Tensor grouped_matmul_nvf4(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs) { return grouped_matmul<Grouped::NVF4>(A, B, A_sf, B_sf, alpha, offs); }
Tensor grouped_matmul_mxf8(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs) { return grouped_matmul<Grouped::MXF8>(A, B, A_sf, B_sf, alpha, offs); }
Tensor grouped_matmul_mxf8_mxf4(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs) { return grouped_matmul<Grouped::MXF8_MXF4>(A, B, A_sf, B_sf, alpha, offs); }
Tensor grouped_matmul_mxf6_mxf4(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs) { return grouped_matmul<Grouped::MXF6_MXF4>(A, B, A_sf, B_sf, alpha, offs); }

// EXTENSION: grouped W4A16 GEMM (qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn) -- A (M, K) bf16 tokens sorted by expert and WITHOUT scales, or with src_row (M,) int32 the
// unsorted (T, K) tokens (row r of the output reads A[src_row[r]]); B (E, N, K/2) packed e2m1 and B_sf row-major (E, N, K/32) e8m0 as grouped_matmul_mxf4's; alpha, offs as
// there.  Allocates (M, N) bf16; rows at or past offs[E-1] are not written.
Tensor grouped_matmul_bf16_mxf4(const Tensor& A, const Tensor& B, const Tensor& B_sf, const Tensor& alpha, const Tensor& offs, std::optional<Tensor> src_row) {
  const char* op = "grouped_matmul_bf16_mxf4_bf16_tn";
  check_tensors(op, {{A, "A"}, {B, "B"}, {B_sf, "B_sf"}, {alpha, "alpha"}, {offs, "offs"}});
  STD_TORCH_CHECK(has_dtype(A, ScalarType::BFloat16), op, ": A must be bfloat16");
  STD_TORCH_CHECK(has_dtype(B, ScalarType::Byte) || has_dtype(B, ScalarType::Float4_e2m1fn_x2), op, ": B must be uint8 or float4_e2m1fn_x2");
  STD_TORCH_CHECK(has_dtype(B_sf, ScalarType::Float8_e8m0fnu), "B_sf must be float8_e8m0fnu");
  STD_TORCH_CHECK(A.dim() == 2 && B.dim() == 3, "A must be 2D (M, K) and B 3D (E, N, K/2)");
  STD_TORCH_CHECK(A.size(1) == B.size(2) * 2, "Inner dimensions must match for A @ B[g].T");
  const int64_t E = B.size(0), N = B.size(1), K = A.size(1), kb = K / 32;
  int64_t M = A.size(0), T = 0;
  const int32_t* src = nullptr;
  if (src_row) {
    const Named a{A, "A"};
    check_tensors(op, {{*src_row, "src_row"}}, {}, true, &a);
    STD_TORCH_CHECK(has_dtype(*src_row, ScalarType::Int) && src_row->dim() == 1, "src_row must be a 1D int32 tensor");
    T = A.size(0);
    M = src_row->size(0);
    src = static_cast<const int32_t*>(src_row->data_ptr());
  }
  STD_TORCH_CHECK(E >= 1 && E <= 1024, "the number of experts must be in [1, 1024] (got ", E, ")");
  STD_TORCH_CHECK(has_dtype(offs, ScalarType::Int) && offs.numel() == E, "offs must be an int32 tensor of E = ", E, " elements");
  STD_TORCH_CHECK(has_dtype(alpha, ScalarType::Float) && (alpha.numel() == 1 || alpha.numel() == E), "alpha must be a float32 tensor of 1 or E = ", E, " elements");
  STD_TORCH_CHECK(B_sf.numel() >= E * N * kb, "B_sf has ", B_sf.numel(), " elements, the row-major scale layout of B needs ", E * N * kb);
  Tensor out = torch::stable::new_empty(A, {M, N}, ScalarType::BFloat16);
  if (M == 0 || N == 0) return out;   // empty batch: nothing to launch

  const torch::stable::accelerator::DeviceGuard guard(A.get_device_index());
  check_rc(qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn(A.data_ptr(), B.data_ptr(), B_sf.data_ptr(), static_cast<const float*>(alpha.data_ptr()), alpha.numel(),
                                                        static_cast<const int32_t*>(offs.data_ptr()), src, T, out.data_ptr(), M, N, K, E, current_stream(A)));
  return out;
}

Tensor matmul_mxf4_bf16_tn(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha) { return matmul<Gemm::MXF4>(A, B, A_sf, B_sf, alpha); }
Tensor matmul_ada_mxf4_bf16_tn(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha) { return matmul<Gemm::ADA_MXF4>(A, B, A_sf, B_sf, alpha); }
Tensor matmul_nvf4_bf16_tn(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha) { return matmul<Gemm::NVF4>(A, B, A_sf, B_sf, alpha); }
Tensor matmul_mxf8_bf16_tn(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha) { return matmul<Gemm::MXF8_TN>(A, B, A_sf, B_sf, alpha); }
Tensor matmul_mxf8_bf16_nn(const Tensor& A, const Tensor& B, const Tensor& A_sf, const Tensor& B_sf, const Tensor& alpha) { return matmul<Gemm::MXF8_NN>(A, B, A_sf, B_sf, alpha); }

// ---- fused rotate + quantize ---------------------------------------------------------------------------------------
int64_t nbytes(const Tensor& t) { return t.numel() * (int64_t)t.element_size(); }

// The family's checks, written once; every op below calls them in the reference's order: prelude, its own shape derivation, rotation set, its own divisibility
// check, output sizes.  gscale != nullptr is the NV format (e4m3 scale per 16, rotation 16 allowed, global scale required); nullptr is MX (e8m0 per 32).
// ts: the op's tensors in argument order, A and the rotation first; global_scale joins the device checks but need not be contiguous (one element).
// method: checked here for the ops whose schema carries it; the blocked ops leave it to the C ABI.  Returns the rotation size.
// offs (the *Grouped_ ops, the last of ts): one global scale per expert -- gscale is then (E,) for offs (E,) int32, and must be contiguous like everything else.
int64_t quant_prelude(const char* op, std::vector<Named> ts, const Tensor* gscale, const int64_t* method = nullptr, const Tensor* offs = nullptr) {
  std::vector<Named> device_only;
  if (offs) ts.push_back({*gscale, "global_scales"});
  else if (gscale) device_only.push_back({*gscale, "global_scale"});
  check_tensors(op, ts, device_only);
  const Tensor& R = ts[1].t;
  STD_TORCH_CHECK(has_dtype(ts[0].t, ScalarType::BFloat16), "A must be bf16");
  STD_TORCH_CHECK(has_dtype(R, ScalarType::BFloat16), "B must be bf16");
  if (offs) {
    STD_TORCH_CHECK(has_dtype(*offs, ScalarType::Int) && offs->dim() == 1, "offs must be a 1D int32 tensor");
    STD_TORCH_CHECK(has_dtype(*gscale, ScalarType::Float), "global_scales must be float");
    STD_TORCH_CHECK(gscale->dim() == 1 && gscale->size(0) == offs->size(0), "global_scales must have one entry per entry of offs");
  } else if (gscale) {
    STD_TORCH_CHECK(has_dtype(*gscale, ScalarType::Float), "global_scale must be float");
    STD_TORCH_CHECK(gscale->dim() == 1 && gscale->size(0) == 1, "global_scale must be a scalar");
  }
  if (method) STD_TORCH_CHECK(*method == QAMD_METHOD_QUEST || *method == QAMD_METHOD_ABSMAX, "method must be 0 (quest) or 1 (abs_max)");
  STD_TORCH_CHECK(R.dim() == 2 && R.size(0) == R.size(1), "Rotation matrix must be square");
  return R.size(0);
}

void quant_check_rot(bool nv, int64_t rot, bool mask = false) {
  const bool ok = mask ? rot == 32 : ((nv && rot == 16) || rot == 32 || rot == 64 || rot == 128);
  STD_TORCH_CHECK(ok, "Unsupported rotation size ", rot, "; expected ", mask ? "32" : nv ? "16, 32, 64, or 128" : "32, 64, or 128", ".");
}

int64_t quant_rp(int64_t rot) { return rot < 32 ? 32 : rot; }   // rows are whole tiles of max(rot, 32) elements

// the C ABI writes numel / 2 bytes of codes and one scale byte per group -- flat, or the padded to_blocked() matrix of the (numel / k, k / group) scales
// (fp8: the MXFP8 ops -- one code byte per element)
// (fp6: the MXFP6 ops -- four codes in three bytes)
void quant_check_out(bool nv, const Tensor& OUT, const Tensor& OUT_sf, int64_t numel, int64_t k, bool blocked, bool fp8 = false, bool fp6 = false) {
  const int64_t group = nv ? 16 : 32;
  STD_TORCH_CHECK(nbytes(OUT) >= (fp6 ? numel / 4 * 3 : fp8 ? numel : numel / 2), "OUT is too small");
  STD_TORCH_CHECK(nbytes(OUT_sf) >= (blocked ? (numel / k + 127) / 128 * 128 * ((k / group + 3) / 4 * 4) : numel / group), "OUT_sf is too small",
                  blocked ? " for the blocked scale layout" : "");
}

const float* gscale_ptr(const Tensor* gscale) { return static_cast<const float*>(gscale->data_ptr()); }

// The MXFP8 ops (fusedQuantizeMxf8_ ...): OUT's dtype selects the code format -- the C ABI's fmt; the scales are e8m0 (or plain bytes).  e4m3_only: the gated op.
int mxf8_fmt(const Tensor& OUT, const Tensor& OUT_sf, bool e4m3_only = false) {
  const bool e4m3 = has_dtype(OUT, ScalarType::Float8_e4m3fn), e5m2 = has_dtype(OUT, ScalarType::Float8_e5m2);
  if (e4m3_only) {
    STD_TORCH_CHECK(e4m3, "OUT must be float8_e4m3fn");
  } else {
    STD_TORCH_CHECK(e4m3 || e5m2, "OUT must be float8_e4m3fn or float8_e5m2");
  }
  STD_TORCH_CHECK(has_dtype(OUT_sf, ScalarType::Float8_e8m0fnu) || has_dtype(OUT_sf, ScalarType::Byte), "OUT_sf must be float8_e8m0fnu or uint8");
  return e5m2 ? QAMD_FP8_E5M2 : QAMD_FP8_E4M3;
}

// The MXFP6 ops (fusedQuantizeMxf6_, fusedGatherQuantizeMxf6_) go through the MXFP8 ops' functions with this value where those carry the C ABI's fmt: OUT is uint8,
// (.., 3K/4) bytes of packed e2m3 codes
constexpr int kFmtMxf6 = 2;
int mxf6_fmt(const Tensor& OUT, const Tensor& OUT_sf) {
  STD_TORCH_CHECK(has_dtype(OUT, ScalarType::Byte), "OUT must be uint8");
  STD_TORCH_CHECK(has_dtype(OUT_sf, ScalarType::Float8_e8m0fnu) || has_dtype(OUT_sf, ScalarType::Byte), "OUT_sf must be float8_e8m0fnu or uint8");
  return kFmtMxf6;
}

// OUT_mask != nullptr (MX only): Quest with clip mask (rotation 32 only).  fmt8 >= 0 (MX only): the MXFP8 op -- kFmtMxf6: the MXFP6 op --, method is not read.
void quantize(const char* op, const Tensor& A, const Tensor& R, Tensor& OUT, Tensor& OUT_sf, Tensor* OUT_mask, const Tensor* gscale, int method, int fmt8 = -1) {
  std::vector<Named> ts{{A, "A"}, {R, "B"}, {OUT, "OUT"}, {OUT_sf, "OUT_sf"}};
  if (OUT_mask) ts.push_back({*OUT_mask, "OUT_mask"});
  const int64_t rot = quant_prelude(op, ts, gscale), numel = A.numel();
  STD_TORCH_CHECK(numel % rot == 0, "A must be divisible by", rot);
  quant_check_rot(gscale, rot, OUT_mask);
  quant_check_out(gscale, OUT, OUT_sf, numel, 0, false, fmt8 >= 0, fmt8 == kFmtMxf6);
  if (OUT_mask) {
    STD_TORCH_CHECK(nbytes(*OUT_mask) >= numel / 8, "OUT_mask is too small");
  }
  const torch::stable::accelerator::DeviceGuard guard(A.get_device_index());
  if (fmt8 == kFmtMxf6)
    check_rc(qutlass_amd_fused_quantize_mxf6(A.data_ptr(), R.data_ptr(), (int)rot, numel, OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(A)));
  else if (fmt8 >= 0)
    check_rc(qutlass_amd_fused_quantize_mxf8(A.data_ptr(), R.data_ptr(), (int)rot, numel, fmt8, OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(A)));
  else if (gscale)
    check_rc(qutlass_amd_fused_quantize_nv(A.data_ptr(), R.data_ptr(), (int)rot, numel, method, gscale_ptr(gscale), OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(A)));
  else
    check_rc(qutlass_amd_fused_quantize_mx(A.data_ptr(), R.data_ptr(), (int)rot, numel, method, OUT.data_ptr(), OUT_sf.data_ptr(),
                                           OUT_mask ? OUT_mask->data_ptr() : nullptr, current_stream(A)));
}

std::tuple<Tensor, Tensor> fusedQuantizeMxQuest(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf) {
  quantize("fusedQuantizeMxQuest", A, R, OUT, OUT_sf, nullptr, nullptr, QAMD_METHOD_QUEST);
  return {OUT, OUT_sf};
}
std::tuple<Tensor, Tensor> fusedQuantizeMxAbsMax(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf) {
  quantize("fusedQuantizeMxAbsMax", A, R, OUT, OUT_sf, nullptr, nullptr, QAMD_METHOD_ABSMAX);
  return {OUT, OUT_sf};
}
std::tuple<Tensor, Tensor, Tensor> fusedQuantizeMxQuestWithMask(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, Tensor OUT_mask) {
  quantize("fusedQuantizeMxQuestWithMask", A, R, OUT, OUT_sf, &OUT_mask, nullptr, QAMD_METHOD_QUEST);
  return {OUT, OUT_sf, OUT_mask};
}

std::tuple<Tensor, Tensor> fusedQuantizeNvQuest(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, const Tensor& global_scale) {
  quantize("fusedQuantizeNvQuest", A, R, OUT, OUT_sf, nullptr, &global_scale, QAMD_METHOD_QUEST);
  return {OUT, OUT_sf};
}
std::tuple<Tensor, Tensor> fusedQuantizeNvAbsMax(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, const Tensor& global_scale) {
  quantize("fusedQuantizeNvAbsMax", A, R, OUT, OUT_sf, nullptr, &global_scale, QAMD_METHOD_ABSMAX);
  return {OUT, OUT_sf};
}

// ---- in-place twins of the reference's output-filling ops, schemas with the mutation declared (`Tensor(a!)`) ------------------------
// The reference's schemas (bindings.cpp:504-513, kept verbatim above) declare neither that the quantizers write OUT / OUT_sf and return
// aliases of them, nor that the QAT-backward ops fill their last arguments.  Eager dispatch does not care; AOTAutograd / inductor do: an
// undeclared write is dead code to them (the call is removed, or OUT's storage reused while the returned alias is live).  The Python
// wrappers (qutlass_amd/__init__.py) therefore call these twins -- same checks, same C-ABI call -- and hand the caller the tensors they
// allocated; the `_qutlass_C` ops stay for callers that use them directly (eager), WITHOUT fake kernels, so tracing them fails loudly.
void fusedQuantizeMx_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, int64_t method) {
  STD_TORCH_CHECK(method == QAMD_METHOD_QUEST || method == QAMD_METHOD_ABSMAX, "method must be 0 (quest) or 1 (abs_max)");
  quantize(method == QAMD_METHOD_QUEST ? "fusedQuantizeMxQuest" : "fusedQuantizeMxAbsMax", A, R, OUT, OUT_sf, nullptr, nullptr, (int)method);
}
void fusedQuantizeMxMask_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, Tensor OUT_mask) {
  quantize("fusedQuantizeMxQuestWithMask", A, R, OUT, OUT_sf, &OUT_mask, nullptr, QAMD_METHOD_QUEST);
}
void fusedQuantizeNv_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, const Tensor& global_scale, int64_t method) {
  STD_TORCH_CHECK(method == QAMD_METHOD_QUEST || method == QAMD_METHOD_ABSMAX, "method must be 0 (quest) or 1 (abs_max)");
  quantize(method == QAMD_METHOD_QUEST ? "fusedQuantizeNvQuest" : "fusedQuantizeNvAbsMax", A, R, OUT, OUT_sf, nullptr, &global_scale, (int)method);
}

// ---- EXTENSION: quantizers that emit GEMM-ready (to_blocked-layout) scales: one launch instead of quantize + to_blocked ----------
// A is (.., K); OUT_sf must hold the padded blocked matrix of the (numel / K, K / gs) scales.  method: 0 quest, 1 abs_max.
void quantize_blocked(const char* op, const Tensor& A, const Tensor& R, Tensor& OUT, Tensor& OUT_sf, const Tensor* gscale, int64_t method, int fmt8 = -1) {
  const int64_t rot = quant_prelude(op, {{A, "A"}, {R, "B"}, {OUT, "OUT"}, {OUT_sf, "OUT_sf"}}, gscale);
  STD_TORCH_CHECK(A.dim() >= 1 && A.numel() > 0, "A must be a non-empty tensor");
  const int64_t numel = A.numel(), k = A.size(A.dim() - 1), rows = numel / k;
  quant_check_rot(gscale, rot);
  STD_TORCH_CHECK(k % quant_rp(rot) == 0, "the last dimension of A must be divisible by", quant_rp(rot));
  quant_check_out(gscale, OUT, OUT_sf, numel, k, true, fmt8 >= 0);
  const torch::stable::accelerator::DeviceGuard guard(A.get_device_index());
  if (fmt8 >= 0)
    check_rc(qutlass_amd_fused_quantize_mxf8_blocked(A.data_ptr(), R.data_ptr(), (int)rot, rows, k, fmt8, OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(A)));
  else if (gscale)
    check_rc(qutlass_amd_fused_quantize_nv_blocked(A.data_ptr(), R.data_ptr(), (int)rot, rows, k, (int)method, gscale_ptr(gscale), OUT.data_ptr(), OUT_sf.data_ptr(),
                                                   current_stream(A)));
  else
    check_rc(qutlass_amd_fused_quantize_mx_blocked(A.data_ptr(), R.data_ptr(), (int)rot, rows, k, (int)method, OUT.data_ptr(), OUT_sf.data_ptr(), nullptr,
                                                   current_stream(A)));
}
void fusedQuantizeMxBlocked(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, int64_t method) { quantize_blocked("fusedQuantizeMxBlocked", A, R, OUT, OUT_sf, nullptr, method); }
void fusedQuantizeNvBlocked(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, const Tensor& gscale, int64_t method) {
  quantize_blocked("fusedQuantizeNvBlocked", A, R, OUT, OUT_sf, &gscale, method);
}

// ---- EXTENSION: the gated-MLP activation act = silu(gate) * up of X = (.., 2 I) [gate | up], alone and fused into the quantizers ----------
// OUT / OUT_sf are sized as for the plain quantizers on a (.., I) tensor.  method: 0 quest, 1 abs_max; blocked: scales in the to_blocked layout.
struct GateUp {
  int64_t rows, inter;
};
GateUp gate_up_shape(const Tensor& X, const char* name) {   // X (.., 2 I) as `rows` rows of [gate | up], I = inter
  STD_TORCH_CHECK(X.dim() >= 1 && X.size(X.dim() - 1) > 0 && X.size(X.dim() - 1) % 2 == 0, "the last dimension of ", name, " must be 2 * I");
  const int64_t inter = X.size(X.dim() - 1) / 2;
  return {X.numel() / (2 * inter), inter};
}
// siluAndMul_ and swigluOaiAndMul_: X (.., 2 I) bf16 -> OUT of at least rows * I bf16
GateUp activation_checks(const char* op, const Tensor& X, const Tensor& OUT) {
  check_tensors(op, {{X, "X"}, {OUT, "OUT"}});
  STD_TORCH_CHECK(has_dtype(X, ScalarType::BFloat16) && has_dtype(OUT, ScalarType::BFloat16), "X and OUT must be bf16");
  const GateUp g = gate_up_shape(X, "X");
  STD_TORCH_CHECK(g.inter % 8 == 0, "the gate / up width must be divisible by", 8);
  STD_TORCH_CHECK(OUT.numel() >= g.rows * g.inter, "OUT is too small");
  return g;
}
void siluAndMul_(const Tensor& X, Tensor OUT) {
  const auto [rows, inter] = activation_checks("siluAndMul_", X, OUT);
  const torch::stable::accelerator::DeviceGuard guard(X.get_device_index());
  check_rc(qutlass_amd_silu_mul_bf16(X.data_ptr(), rows, inter, OUT.data_ptr(), current_stream(X)));
}

// offs != nullptr (NV, flat scales): one global scale per expert, gscale (E,) with the grouped GEMMs' offs (E,) int32
void silu_mul_quantize(const char* op, const Tensor& X, const Tensor& R, Tensor& OUT, Tensor& OUT_sf, const Tensor* gscale, int64_t method, bool blocked,
                       const Tensor* offs = nullptr, int fmt8 = -1) {
  std::vector<Named> ts{{X, "A"}, {R, "B"}, {OUT, "OUT"}, {OUT_sf, "OUT_sf"}};
  if (offs) ts.push_back({*offs, "offs"});
  const int64_t rot = quant_prelude(op, ts, gscale, &method, offs);
  const auto [rows, inter] = gate_up_shape(X, "A");
  quant_check_rot(gscale, rot);
  STD_TORCH_CHECK(inter % quant_rp(rot) == 0, "the gate / up width must be divisible by", quant_rp(rot));
  quant_check_out(gscale, OUT, OUT_sf, rows * inter, inter, blocked, fmt8 >= 0);
  const torch::stable::accelerator::DeviceGuard guard(X.get_device_index());
  if (fmt8 >= 0)
    check_rc(qutlass_amd_fused_silu_mul_quantize_mxf8(X.data_ptr(), R.data_ptr(), (int)rot, rows, inter, fmt8, blocked ? 1 : 0, OUT.data_ptr(), OUT_sf.data_ptr(),
                                                      current_stream(X)));
  else if (offs)
    check_rc(qutlass_amd_fused_silu_mul_quantize_nv_grouped(X.data_ptr(), R.data_ptr(), (int)rot, rows, inter, (int)method, gscale_ptr(gscale),
                                                            static_cast<const int32_t*>(offs->data_ptr()), offs->size(0), OUT.data_ptr(), OUT_sf.data_ptr(),
                                                            current_stream(X)));
  else if (gscale)
    check_rc(qutlass_amd_fused_silu_mul_quantize_nv(X.data_ptr(), R.data_ptr(), (int)rot, rows, inter, (int)method, gscale_ptr(gscale), blocked ? 1 : 0, OUT.data_ptr(),
                                                    OUT_sf.data_ptr(), current_stream(X)));
  else
    check_rc(qutlass_amd_fused_silu_mul_quantize_mx(X.data_ptr(), R.data_ptr(), (int)rot, rows, inter, (int)method, blocked ? 1 : 0, OUT.data_ptr(), OUT_sf.data_ptr(),
                                                    current_stream(X)));
}
void fusedSiluMulQuantizeMx_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, int64_t method, bool blocked) {
  silu_mul_quantize(blocked ? "fusedSiluMulQuantizeMxBlocked" : "fusedSiluMulQuantizeMx", A, R, OUT, OUT_sf, nullptr, method, blocked);
}
void fusedSiluMulQuantizeNv_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, const Tensor& global_scale, int64_t method, bool blocked) {
  silu_mul_quantize(blocked ? "fusedSiluMulQuantizeNvBlocked" : "fusedSiluMulQuantizeNv", A, R, OUT, OUT_sf, &global_scale, method, blocked);
}
void fusedSiluMulQuantizeNvGrouped_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, const Tensor& global_scales, const Tensor& offs, int64_t method) {
  silu_mul_quantize("fusedSiluMulQuantizeNvGrouped", A, R, OUT, OUT_sf, &global_scales, method, false, &offs);
}

// ---- EXTENSION: MoE dispatch and combine around the grouped GEMMs ---------------------------------------------------------------------
// fusedGatherQuantize{Mx,Nv}_: fusedQuantize{Mx,Nv}_ of A.index_select(0, src_row) in one launch, byte for byte; A (T, K) bf16, src_row (M) int32 read on the device (no
// host sync).  OUT / OUT_sf are sized as for the plain quantizers on an (M, K) tensor; flat scales.
void gather_quantize(const char* op, const Tensor& X, const Tensor& R, const Tensor& src_row, Tensor& OUT, Tensor& OUT_sf, const Tensor* gscale, int64_t method,
                     const Tensor* offs = nullptr, int fmt8 = -1) {
  std::vector<Named> ts{{X, "A"}, {R, "B"}, {src_row, "src_row"}, {OUT, "OUT"}, {OUT_sf, "OUT_sf"}};
  if (offs) ts.push_back({*offs, "offs"});
  const int64_t rot = quant_prelude(op, ts, gscale, &method, offs);
  STD_TORCH_CHECK(X.dim() == 2 && X.size(1) > 0, "A must be 2D (T, K)");
  STD_TORCH_CHECK(has_dtype(src_row, ScalarType::Int) && src_row.dim() == 1, "src_row must be a 1D int32 tensor");
  const int64_t T = X.size(0), K = X.size(1), M = src_row.size(0);
  quant_check_rot(gscale, rot);
  STD_TORCH_CHECK(K % quant_rp(rot) == 0, "the last dimension of A must be divisible by", quant_rp(rot));
  quant_check_out(gscale, OUT, OUT_sf, M * K, K, false, fmt8 >= 0, fmt8 == kFmtMxf6);
  const torch::stable::accelerator::DeviceGuard guard(X.get_device_index());
  if (fmt8 == kFmtMxf6)
    check_rc(qutlass_amd_fused_gather_quantize_mxf6(X.data_ptr(), R.data_ptr(), (int)rot, T, K, static_cast<const int32_t*>(src_row.data_ptr()), M, OUT.data_ptr(),
                                                    OUT_sf.data_ptr(), current_stream(X)));
  else if (fmt8 >= 0)
    check_rc(qutlass_amd_fused_gather_quantize_mxf8(X.data_ptr(), R.data_ptr(), (int)rot, T, K, static_cast<const int32_t*>(src_row.data_ptr()), M, fmt8, OUT.data_ptr(),
                                                    OUT_sf.data_ptr(), current_stream(X)));
  else if (offs)
    check_rc(qutlass_amd_fused_gather_quantize_nv_grouped(X.data_ptr(), R.data_ptr(), (int)rot, T, K, static_cast<const int32_t*>(src_row.data_ptr()), M, (int)method,
                                                          gscale_ptr(gscale), static_cast<const int32_t*>(offs->data_ptr()), offs->size(0), OUT.data_ptr(),
                                                          OUT_sf.data_ptr(), current_stream(X)));
  else if (gscale)
    check_rc(qutlass_amd_fused_gather_quantize_nv(X.data_ptr(), R.data_ptr(), (int)rot, T, K, static_cast<const int32_t*>(src_row.data_ptr()), M, (int)method,
                                                  gscale_ptr(gscale), OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(X)));
  else
    check_rc(qutlass_amd_fused_gather_quantize_mx(X.data_ptr(), R.data_ptr(), (int)rot, T, K, static_cast<const int32_t*>(src_row.data_ptr()), M, (int)method,
                                                  OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(X)));
}
void fusedGatherQuantizeMx_(const Tensor& A, const Tensor& R, const Tensor& src_row, Tensor OUT, Tensor OUT_sf, int64_t method) {
  gather_quantize("fusedGatherQuantizeMx", A, R, src_row, OUT, OUT_sf, nullptr, method);
}
void fusedGatherQuantizeNv_(const Tensor& A, const Tensor& R, const Tensor& src_row, Tensor OUT, Tensor OUT_sf, const Tensor& global_scale, int64_t method) {
  gather_quantize("fusedGatherQuantizeNv", A, R, src_row, OUT, OUT_sf, &global_scale, method);
}
void fusedGatherQuantizeNvGrouped_(const Tensor& A, const Tensor& R, const Tensor& src_row, Tensor OUT, Tensor OUT_sf, const Tensor& global_scales, const Tensor& offs,
                                   int64_t method) {
  gather_quantize("fusedGatherQuantizeNvGrouped", A, R, src_row, OUT, OUT_sf, &global_scales, method, &offs);
}

// ---- EXTENSION: the MXFP8 quantizers -- e4m3 / e5m2 codes with one e8m0 scale per 32 elements, abs-max; the same four forms through the same four functions ------
// OUT is (.., K) float8_e4m3fn or float8_e5m2 (the dtype selects the format; the gated op takes e4m3 only), OUT_sf as for the MX ops.
void fusedQuantizeMxf8_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf) {
  quantize("fusedQuantizeMxf8", A, R, OUT, OUT_sf, nullptr, nullptr, QAMD_METHOD_ABSMAX, mxf8_fmt(OUT, OUT_sf));
}
void fusedQuantizeMxf8Blocked_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf) {
  quantize_blocked("fusedQuantizeMxf8Blocked", A, R, OUT, OUT_sf, nullptr, QAMD_METHOD_ABSMAX, mxf8_fmt(OUT, OUT_sf));
}
void fusedSiluMulQuantizeMxf8_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, bool blocked) {
  silu_mul_quantize(blocked ? "fusedSiluMulQuantizeMxf8Blocked" : "fusedSiluMulQuantizeMxf8", A, R, OUT, OUT_sf, nullptr, QAMD_METHOD_ABSMAX, blocked, nullptr,
                    mxf8_fmt(OUT, OUT_sf, true));
}
void fusedGatherQuantizeMxf8_(const Tensor& A, const Tensor& R, const Tensor& src_row, Tensor OUT, Tensor OUT_sf) {
  gather_quantize("fusedGatherQuantizeMxf8", A, R, src_row, OUT, OUT_sf, nullptr, QAMD_METHOD_ABSMAX, nullptr, mxf8_fmt(OUT, OUT_sf));
}

// ---- EXTENSION: the MXFP6 quantizers -- e2m3 codes, four in three bytes, with one e8m0 scale per 32 elements, abs-max; the plain and the gathering form ------
// OUT is (.., 3K/4) uint8, OUT_sf as for the MX ops (flat).
void fusedQuantizeMxf6_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf) {
  quantize("fusedQuantizeMxf6", A, R, OUT, OUT_sf, nullptr, nullptr, QAMD_METHOD_ABSMAX, mxf6_fmt(OUT, OUT_sf));
}
void fusedGatherQuantizeMxf6_(const Tensor& A, const Tensor& R, const Tensor& src_row, Tensor OUT, Tensor OUT_sf) {
  gather_quantize("fusedGatherQuantizeMxf6", A, R, src_row, OUT, OUT_sf, nullptr, QAMD_METHOD_ABSMAX, nullptr, mxf6_fmt(OUT, OUT_sf));
}

// ---- EXTENSION: gpt-oss -- the clamped SwiGLU with per-expert gate/up biases, alone and fused into the MXFP4 and the MXFP8 (e4m3) quantizer, and moe_combine with the down bias ------
// bias: (E, 2 I) bf16, or an EMPTY tensor for "no bias"; offs: (E,) int32, or an empty tensor where there is no bias or E == 1.  The arithmetic is spelled out at
// qutlass_amd_swiglu_oai_mul_bf16 (include/qutlass_amd.h).
struct OaiBias {
  const void* bias = nullptr;
  const int32_t* offs = nullptr;
  int64_t e = 0;
};
OaiBias oai_bias(const char* op, const Tensor& X, const Tensor& bias, const Tensor& offs, int64_t width) {
  OaiBias b;
  if (bias.numel() == 0) {
    STD_TORCH_CHECK(offs.numel() == 0, "offs without a bias");
    return b;
  }
  const Named x{X, "X"};
  check_tensors(op, {{bias, "bias"}}, {}, true, &x);
  STD_TORCH_CHECK(has_dtype(bias, ScalarType::BFloat16), "bias must be bf16");
  STD_TORCH_CHECK(bias.dim() == 2 && bias.size(1) == width, "bias must be (E, ", width, ")");
  b.bias = bias.data_ptr();
  b.e = bias.size(0);
  STD_TORCH_CHECK(b.e >= 1 && b.e <= 1024, "the number of experts must be in [1, 1024] (got ", b.e, ")");
  if (offs.numel() == 0) {
    STD_TORCH_CHECK(b.e == 1, "a bias of E = ", b.e, " experts needs offs");
    return b;
  }
  check_tensors(op, {{offs, "offs"}}, {}, true, &x);
  STD_TORCH_CHECK(has_dtype(offs, ScalarType::Int) && offs.dim() == 1 && offs.size(0) == b.e, "offs must be an int32 tensor of E = ", b.e, " elements");
  b.offs = static_cast<const int32_t*>(offs.data_ptr());
  return b;
}

void swigluOaiAndMul_(const Tensor& X, Tensor OUT, double alpha, double limit, const Tensor& bias, const Tensor& offs) {
  const auto [rows, inter] = activation_checks("swigluOaiAndMul_", X, OUT);
  const OaiBias b = oai_bias("swigluOaiAndMul_", X, bias, offs, 2 * inter);
  const torch::stable::accelerator::DeviceGuard guard(X.get_device_index());
  check_rc(qutlass_amd_swiglu_oai_mul_bf16(X.data_ptr(), rows, inter, (float)alpha, (float)limit, b.bias, b.offs, b.e, OUT.data_ptr(), current_stream(X)));
}

// fmt8 < 0: the MXFP4 op (plain = fusedQuantizeMx; method read); fmt8 >= 0: the e4m3 op (plain = fusedQuantizeMxf8; abs-max, method not read)
void swiglu_oai_quantize(const char* op, const char* plain, const Tensor& A, const Tensor& R, Tensor& OUT, Tensor& OUT_sf, double alpha, double limit, const Tensor& bias,
                         const Tensor& offs, int64_t method, int fmt8 = -1) {
  const int64_t rot = quant_prelude(op, {{A, "A"}, {R, "B"}, {OUT, "OUT"}, {OUT_sf, "OUT_sf"}}, nullptr, fmt8 < 0 ? &method : nullptr);
  const auto [rows, inter] = gate_up_shape(A, "A");
  STD_TORCH_CHECK(rot != 128, "rotation size 128 is not supported; expected 32 or 64 (use swiglu_oai_and_mul followed by ", plain, ")");
  STD_TORCH_CHECK(rot == 32 || rot == 64, "Unsupported rotation size ", rot, "; expected 32 or 64.");
  STD_TORCH_CHECK(inter % rot == 0, "the gate / up width must be divisible by", rot);
  quant_check_out(false, OUT, OUT_sf, rows * inter, inter, false, fmt8 >= 0);
  const OaiBias b = oai_bias(op, A, bias, offs, 2 * inter);
  const torch::stable::accelerator::DeviceGuard guard(A.get_device_index());
  if (fmt8 >= 0)
    check_rc(qutlass_amd_fused_swiglu_oai_quantize_mxf8(A.data_ptr(), R.data_ptr(), (int)rot, rows, inter, fmt8, (float)alpha, (float)limit, b.bias, b.offs, b.e,
                                                        OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(A)));
  else
    check_rc(qutlass_amd_fused_swiglu_oai_quantize_mx(A.data_ptr(), R.data_ptr(), (int)rot, rows, inter, (int)method, (float)alpha, (float)limit, b.bias, b.offs, b.e,
                                                      OUT.data_ptr(), OUT_sf.data_ptr(), current_stream(A)));
}
void fusedSwigluOaiQuantizeMx_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, double alpha, double limit, const Tensor& bias, const Tensor& offs,
                               int64_t method) {
  swiglu_oai_quantize("fusedSwigluOaiQuantizeMx", "fusedQuantizeMx", A, R, OUT, OUT_sf, alpha, limit, bias, offs, method);
}
// the W4A8 form: OUT (.., I) float8_e4m3fn (a forward activation: e4m3 only), OUT_sf as for the MX op
void fusedSwigluOaiQuantizeMxf8_(const Tensor& A, const Tensor& R, Tensor OUT, Tensor OUT_sf, double alpha, double limit, const Tensor& bias, const Tensor& offs) {
  swiglu_oai_quantize("fusedSwigluOaiQuantizeMxf8", "fusedQuantizeMxf8", A, R, OUT, OUT_sf, alpha, limit, bias, offs, QAMD_METHOD_ABSMAX, mxf8_fmt(OUT, OUT_sf, true));
}

// moeCombine_: OUT[t] = sum_k weights[t][k] * Y[pos[t][k]] (the arithmetic is spelled out at qutlass_amd_moe_combine_bf16); slots with pos outside [0, M) are skipped
// moeCombineBias_ (bias != nullptr): the same with bias (E, H) bf16 added to every gathered row in bf16; offs (E,) int32, or empty for E == 1
void moe_combine(const char* op, const Tensor& Y, const Tensor& pos, const Tensor& weights, const Tensor* bias, const Tensor* offs, Tensor& OUT) {
  check_tensors(op, {{Y, "Y"}, {pos, "pos"}, {weights, "weights"}, {OUT, "OUT"}});
  STD_TORCH_CHECK(has_dtype(Y, ScalarType::BFloat16) && has_dtype(OUT, ScalarType::BFloat16), "Y and OUT must be bf16");
  STD_TORCH_CHECK(has_dtype(pos, ScalarType::Int), "pos must be int32");
  STD_TORCH_CHECK(has_dtype(weights, ScalarType::Float), "weights must be float32");
  STD_TORCH_CHECK(Y.dim() == 2 && Y.size(1) > 0, "Y must be 2D (M, H)");
  STD_TORCH_CHECK(pos.dim() == 2 && weights.dim() == 2 && pos.size(0) == weights.size(0) && pos.size(1) == weights.size(1), "pos and weights must both be (T, topk)");
  const int64_t M = Y.size(0), H = Y.size(1), T = pos.size(0), topk = pos.size(1);
  STD_TORCH_CHECK(H % 8 == 0, "the row length of Y must be divisible by", 8);
  STD_TORCH_CHECK(topk >= 1 && topk <= 32, "topk must be in [1, 32] (got ", topk, ")");
  STD_TORCH_CHECK(OUT.numel() >= T * H, "OUT is too small");
  OaiBias b;
  if (bias) {
    STD_TORCH_CHECK(bias->numel() > 0, "bias must be (E, ", H, ")");
    b = oai_bias(op, Y, *bias, *offs, H);
  }
  const torch::stable::accelerator::DeviceGuard guard(Y.get_device_index());
  const int32_t* p = static_cast<const int32_t*>(pos.data_ptr());
  const float* w = static_cast<const float*>(weights.data_ptr());
  check_rc(bias ? qutlass_amd_moe_combine_bias_bf16(Y.data_ptr(), M, H, p, w, T, topk, b.bias, b.offs, b.e, OUT.data_ptr(), current_stream(Y))
                : qutlass_amd_moe_combine_bf16(Y.data_ptr(), M, H, p, w, T, topk, OUT.data_ptr(), current_stream(Y)));
}
void moeCombine_(const Tensor& Y, const Tensor& pos, const Tensor& weights, Tensor OUT) { moe_combine("moeCombine_", Y, pos, weights, nullptr, nullptr, OUT); }
void moeCombineBias_(const Tensor& Y, const Tensor& pos, const Tensor& weights, const Tensor& bias, const Tensor& offs, Tensor OUT) {
  moe_combine("moeCombineBias_", Y, pos, weights, &bias, &offs, OUT);
}

// ---- EXTENSION: MoE routing in front of the dispatch ---------------------------------------------------------------------------------------------
// moeTopkSoftmax_: router logits (T, E) bf16 / float32 -> weights (T, topk) float32 and ids (T, topk) int32; topk is the outputs' second dimension
// the checks both routers make behind the generic ones; returns whether the logits are float32
bool topk_checks(const Tensor& logits, const Tensor& weights, const Tensor& ids) {
  const bool f32 = has_dtype(logits, ScalarType::Float);
  STD_TORCH_CHECK(f32 || has_dtype(logits, ScalarType::BFloat16), "logits must be bf16 or float32");
  STD_TORCH_CHECK(has_dtype(weights, ScalarType::Float), "weights must be float32");
  STD_TORCH_CHECK(has_dtype(ids, ScalarType::Int), "ids must be int32");
  STD_TORCH_CHECK(logits.dim() == 2, "logits must be 2D (T, E)");
  STD_TORCH_CHECK(weights.dim() == 2 && ids.dim() == 2 && weights.size(0) == logits.size(0) && ids.size(0) == logits.size(0) && weights.size(1) == ids.size(1),
                  "weights and ids must both be (T, topk)");
  return f32;
}
void moeTopkSoftmax_(const Tensor& logits, Tensor weights, Tensor ids, bool renormalize) {
  check_tensors("moeTopkSoftmax_", {{logits, "logits"}, {weights, "weights"}, {ids, "ids"}});
  const bool f32 = topk_checks(logits, weights, ids);
  const torch::stable::accelerator::DeviceGuard guard(logits.get_device_index());
  check_rc(qutlass_amd_moe_topk_softmax(logits.data_ptr(), f32 ? 4 : 2, logits.size(0), logits.size(1), ids.size(1), renormalize ? 1 : 0,
                                        static_cast<float*>(weights.data_ptr()), static_cast<int32_t*>(ids.data_ptr()), current_stream(logits)));
}

// moeTopkGrouped_: the grouped router (qutlass_amd_moe_topk_grouped); topk is the outputs' second dimension; an EMPTY bias means "no bias", an EMPTY scores "not asked for"
void moeTopkGrouped_(const Tensor& logits, const Tensor& bias, Tensor weights, Tensor ids, Tensor scores, int64_t n_group, int64_t topk_group, int64_t scoring,
                     bool renormalize, double routed_scaling_factor) {
  check_tensors("moeTopkGrouped_", {{logits, "logits"}, {bias, "bias"}, {weights, "weights"}, {ids, "ids"}, {scores, "scores"}});
  const bool f32 = topk_checks(logits, weights, ids);
  const bool use_bias = bias.numel() > 0, want_scores = scores.numel() > 0;
  STD_TORCH_CHECK(!use_bias || (has_dtype(bias, ScalarType::Float) && bias.dim() == 1 && bias.size(0) == logits.size(1)), "bias must be a float32 tensor of (E,)");
  STD_TORCH_CHECK(!want_scores || (has_dtype(scores, ScalarType::Float) && scores.dim() == 2 && scores.size(0) == logits.size(0) && scores.size(1) == logits.size(1)),
                  "scores must be a float32 tensor of (T, E)");
  const torch::stable::accelerator::DeviceGuard guard(logits.get_device_index());
  check_rc(qutlass_amd_moe_topk_grouped(logits.data_ptr(), f32 ? 4 : 2, logits.size(0), logits.size(1), ids.size(1), n_group, topk_group, (int)scoring,
                                        use_bias ? static_cast<const float*>(bias.data_ptr()) : nullptr, renormalize ? 1 : 0, (float)routed_scaling_factor,
                                        static_cast<float*>(weights.data_ptr()), static_cast<int32_t*>(ids.data_ptr()),
                                        want_scores ? static_cast<float*>(scores.data_ptr()) : nullptr, current_stream(logits)));
}

// moeSort_: the stable sort of the (T, topk) slots by expert (qutlass_amd_moe_sort); an EMPTY expert_map means "no map" (a map has at least one entry); workspace is
// caller scratch of at least qutlass_amd_moe_sort_workspace_bytes bytes (it may be empty below the one-launch bound)
void moeSort_(const Tensor& topk_ids, const Tensor& expert_map, int64_t num_experts, Tensor src_row, Tensor offs, Tensor pos, Tensor workspace) {
  const char* op = "moeSort_";
  const Named ids{topk_ids, "topk_ids"};
  check_tensors(op, {ids, {src_row, "src_row"}, {offs, "offs"}, {pos, "pos"}, {workspace, "workspace"}});
  const bool i64 = has_dtype(topk_ids, ScalarType::Long);
  STD_TORCH_CHECK(i64 || has_dtype(topk_ids, ScalarType::Int), "topk_ids must be int32 or int64");
  STD_TORCH_CHECK(topk_ids.dim() == 2, "topk_ids must be 2D (T, topk)");
  STD_TORCH_CHECK(has_dtype(src_row, ScalarType::Int) && has_dtype(offs, ScalarType::Int) && has_dtype(pos, ScalarType::Int), "src_row, offs and pos must be int32");
  const int64_t T = topk_ids.size(0), topk = topk_ids.size(1);
  STD_TORCH_CHECK(src_row.numel() >= T * topk && pos.numel() >= T * topk && offs.numel() >= num_experts, "src_row, offs or pos is too small");
  const bool use_map = expert_map.numel() > 0;
  int64_t G = 0;
  if (use_map) {
    check_tensors(op, {{expert_map, "expert_map"}}, {}, true, &ids);
    STD_TORCH_CHECK(has_dtype(expert_map, ScalarType::Int) && expert_map.dim() == 1, "expert_map must be a 1D int32 tensor");
    G = expert_map.size(0);
  }
  const torch::stable::accelerator::DeviceGuard guard(topk_ids.get_device_index());
  check_rc(qutlass_amd_moe_sort(topk_ids.data_ptr(), i64 ? 8 : 4, T, topk, num_experts, use_map ? static_cast<const int32_t*>(expert_map.data_ptr()) : nullptr, G,
                                static_cast<int32_t*>(src_row.data_ptr()), static_cast<int32_t*>(offs.data_ptr()), static_cast<int32_t*>(pos.data_ptr()),
                                workspace.numel() > 0 ? workspace.data_ptr() : nullptr, nbytes(workspace), current_stream(topk_ids)));
}

// moe_route_fused / moe_route_grouped_fused: FUNCTIONAL ops -- the five results of the routing (weights, ids, src_row, offs, pos) are allocated here, as the grouped
// GEMMs allocate theirs.  Up to qutlass_amd_moe_route_fused_max_tokens() tokens: the one-launch entry; beyond: the router's entry and qutlass_amd_moe_sort with its
// scratch -- the same bits either way.  No fill: T > 0 is one graph node up to the bound (two, three or four beyond).  grouped: the arguments behind topk are read, else ignored.
using Routed = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor>;
Routed moe_route_fused_impl(const char* op, bool grouped, const Tensor& logits, const std::optional<Tensor>& bias, const std::optional<Tensor>& expert_map, int64_t topk,
                            int64_t num_experts, int64_t n_group, int64_t topk_group, int64_t scoring, bool renormalize, double routed_scaling_factor) {
  check_tensors(op, {{logits, "logits"}});
  const bool f32 = has_dtype(logits, ScalarType::Float);
  STD_TORCH_CHECK(f32 || has_dtype(logits, ScalarType::BFloat16), "logits must be bf16 or float32");
  STD_TORCH_CHECK(logits.dim() == 2, "logits must be 2D (T, E)");
  const int64_t T = logits.size(0), E = logits.size(1);
  STD_TORCH_CHECK(topk >= 1 && topk <= 32, "topk must be in [1, 32] (got ", topk, ")");
  STD_TORCH_CHECK(num_experts >= 1 && num_experts <= 1024, "the number of experts must be in [1, 1024] (got ", num_experts, ")");
  const Named lg{logits, "logits"};
  const float* b = nullptr;
  if (bias) {
    check_tensors(op, {{*bias, "bias"}}, {}, true, &lg);
    STD_TORCH_CHECK(grouped && has_dtype(*bias, ScalarType::Float) && bias->dim() == 1 && bias->size(0) == E, "bias must be a float32 tensor of (E,)");
    b = static_cast<const float*>(bias->data_ptr());
  }
  const int32_t* map = nullptr;
  int64_t G = 0;
  if (expert_map) {
    check_tensors(op, {{*expert_map, "expert_map"}}, {}, true, &lg);
    STD_TORCH_CHECK(has_dtype(*expert_map, ScalarType::Int) && expert_map->dim() == 1 && expert_map->size(0) >= 1, "expert_map must be a 1D int32 tensor of at least one entry");
    map = static_cast<const int32_t*>(expert_map->data_ptr());
    G = expert_map->size(0);
  }
  Tensor weights = torch::stable::new_empty(logits, {T, topk}, ScalarType::Float), ids = torch::stable::new_empty(logits, {T, topk}, ScalarType::Int);
  Tensor src_row = torch::stable::new_empty(logits, {T * topk}, ScalarType::Int);
  // offs: every sort form writes all of it whenever there is a slot (one workgroup: moe_sort_workgroup<0>; three launches: moe_sort_scan_kernel), so no fill is
  // launched; only T == 0, which launches nothing, needs the zeros.  (T is a concrete size in here: no branch is traced.)
  Tensor offs = T > 0 ? torch::stable::new_empty(logits, {num_experts}, ScalarType::Int) : torch::stable::new_zeros(logits, {num_experts}, ScalarType::Int);
  Tensor pos = torch::stable::new_empty(logits, {T, topk}, ScalarType::Int);
  const torch::stable::accelerator::DeviceGuard guard(logits.get_device_index());
  void* s = current_stream(logits);
  float* w = static_cast<float*>(weights.data_ptr());
  int32_t *id = static_cast<int32_t*>(ids.data_ptr()), *sr = static_cast<int32_t*>(src_row.data_ptr()), *of = static_cast<int32_t*>(offs.data_ptr()),
          *ps = static_cast<int32_t*>(pos.data_ptr());
  const int eb = f32 ? 4 : 2, rn = renormalize ? 1 : 0;
  if (T <= qutlass_amd_moe_route_fused_max_tokens()) {
    check_rc(grouped ? qutlass_amd_moe_route_grouped_fused(logits.data_ptr(), eb, T, E, topk, n_group, topk_group, (int)scoring, b, rn, (float)routed_scaling_factor, w, id,
                                                           num_experts, map, G, sr, of, ps, s)
                     : qutlass_amd_moe_route_fused(logits.data_ptr(), eb, T, E, topk, rn, w, id, num_experts, map, G, sr, of, ps, s));
  } else {
    check_rc(grouped ? qutlass_amd_moe_topk_grouped(logits.data_ptr(), eb, T, E, topk, n_group, topk_group, (int)scoring, b, rn, (float)routed_scaling_factor, w, id, nullptr, s)
                     : qutlass_amd_moe_topk_softmax(logits.data_ptr(), eb, T, E, topk, rn, w, id, s));
    const Workspace ws(logits, qutlass_amd_moe_sort_workspace_bytes(T * topk, num_experts));
    check_rc(qutlass_amd_moe_sort(id, 4, T, topk, num_experts, map, G, sr, of, ps, ws.ptr(), ws.bytes, s));
  }
  return Routed(weights, ids, src_row, offs, pos);
}
Routed moe_route_fused(const Tensor& logits, std::optional<Tensor> expert_map, int64_t topk, int64_t num_experts, bool renormalize) {
  return moe_route_fused_impl("moe_route_fused", false, logits, std::nullopt, expert_map, topk, num_experts, 1, 1, 0, renormalize, 1.0);
}
Routed moe_route_grouped_fused(const Tensor& logits, std::optional<Tensor> bias, std::optional<Tensor> expert_map, int64_t topk, int64_t num_experts, int64_t n_group,
                               int64_t topk_group, int64_t scoring, bool renormalize, double routed_scaling_factor) {
  return moe_route_fused_impl("moe_route_grouped_fused", true, logits, bias, expert_map, topk, num_experts, n_group, topk_group, scoring, renormalize, routed_scaling_factor);
}

// ---- EXTENSION: rotate + quantize + MXFP4 GEMM in one launch for decode batches (M <= 32) ---------------------------------------
Tensor fusedQuantizeMatmulMxf4(const Tensor& X, const Tensor& R, const Tensor& B, const Tensor& B_sf, const Tensor& alpha, int64_t method) {
  const char* op = "fusedQuantizeMatmulMxf4";
  check_tensors(op, {{X, "X"}, {R, "R"}, {B, "B"}, {B_sf, "B_sf"}}, {{alpha, "alpha"}});
  STD_TORCH_CHECK(has_dtype(X, ScalarType::BFloat16) && has_dtype(R, ScalarType::BFloat16), "X and R must be bf16");
  STD_TORCH_CHECK(has_dtype(B, ScalarType::Byte), "B must be uint8");
  STD_TORCH_CHECK(has_dtype(B_sf, ScalarType::Float8_e8m0fnu), "B_sf must be float8_e8m0fnu");
  STD_TORCH_CHECK(has_dtype(alpha, ScalarType::Float) && alpha.numel() >= 1, "alpha must be a float32 tensor with at least one element");
  STD_TORCH_CHECK(X.dim() >= 1 && B.dim() == 2, "X must be at least 1-D and B 2-D");
  STD_TORCH_CHECK(R.dim() == 2 && R.size(0) == R.size(1), "Rotation matrix must be square");
  const int64_t K = X.size(X.dim() - 1), M = K > 0 ? X.numel() / K : 0, N = B.size(0);
  STD_TORCH_CHECK(B.size(1) * 2 == K, "Inner dimensions must match for Q(X) @ B.T");
  STD_TORCH_CHECK(B_sf.numel() >= (N + 127) / 128 * 128 * ((K / 32 + 3) / 4 * 4), "B_sf is too small for the blocked scale layout of B");
  Tensor out = torch::stable::new_empty(X, {M, N}, ScalarType::BFloat16);
  if (M == 0 || N == 0) return out;
  const torch::stable::accelerator::DeviceGuard guard(X.get_device_index());
  check_rc(qutlass_amd_fused_quantize_matmul_mxf4_bf16_tn(X.data_ptr(), R.data_ptr(), (int)R.size(0), (int)method, B.data_ptr(), B_sf.data_ptr(),
                                                          static_cast<const float*>(alpha.data_ptr()), out.data_ptr(), M, N, K, current_stream(X)));
  return out;
}

// ---- QAT-backward data preparation (bindings.cpp:429-494: no validation there; the Python wrappers assert dtypes and
//      contiguity, qutlass/__init__.py:206-315 -- the C ABI checks the shape constraints) --------------------------------
void backward_t_bf16(const Tensor& x, const Tensor& h, Tensor xh_e2m1, Tensor xh_e8m0) {
  const char* op = "backward_t_bf16";
  check_tensors(op, {{x, "x"}, {h, "h"}, {xh_e2m1, "xh_e2m1"}, {xh_e8m0, "xh_e8m0"}}, {}, false);
  STD_TORCH_CHECK(has_dtype(x, ScalarType::BFloat16) && has_dtype(h, ScalarType::BFloat16), "x and h must be bf16");
  STD_TORCH_CHECK(x.dim() >= 2 && h.numel() == 32 * 32, "x must be at least 2-D and h 32 x 32");
  const int64_t M = x.size(x.dim() - 1), N = x.size(x.dim() - 2), B = x.numel() / (M * N);
  STD_TORCH_CHECK(nbytes(xh_e2m1) >= B * M * N / 2 && nbytes(xh_e8m0) >= B * M * N / 32, "output tensors are too small");
  const torch::stable::accelerator::DeviceGuard guard(x.get_device_index());
  check_rc(qutlass_amd_backward_t_bf16(x.data_ptr(), h.data_ptr(), B, N, M, xh_e2m1.data_ptr(), xh_e8m0.data_ptr(), current_stream(x)));
}

void backward_qt_bf16(const Tensor& x_e2m1, const Tensor& x_e8m0, const Tensor& h, const Tensor& alpha, Tensor xh_e2m1, Tensor xh_e8m0) {
  const char* op = "backward_qt_bf16";
  check_tensors(op, {{x_e2m1, "x_e2m1"}, {x_e8m0, "x_e8m0"}, {h, "h"}, {xh_e2m1, "xh_e2m1"}, {xh_e8m0, "xh_e8m0"}}, {{alpha, "alpha"}}, false);
  STD_TORCH_CHECK(has_dtype(h, ScalarType::BFloat16) && has_dtype(alpha, ScalarType::Float), "h must be bf16 and alpha float");
  STD_TORCH_CHECK(x_e2m1.dim() >= 2 && x_e2m1.element_size() == 1 && x_e8m0.element_size() == 1 && h.numel() == 32 * 32,
                  "x_e2m1 / x_e8m0 must be 1-byte tensors of at least 2 dimensions and h 32 x 32");
  const int64_t M = x_e2m1.size(x_e2m1.dim() - 1) * 2, N = x_e2m1.size(x_e2m1.dim() - 2), B = x_e2m1.numel() * 2 / (M * N);
  STD_TORCH_CHECK(x_e8m0.numel() == B * N * M / 32, "x_e8m0 must hold one scale per 32 elements of x_e2m1");
  STD_TORCH_CHECK(nbytes(xh_e2m1) >= B * M * N / 2 && nbytes(xh_e8m0) >= B * M * N / 32, "output tensors are too small");
  const torch::stable::accelerator::DeviceGuard guard(h.get_device_index());
  check_rc(qutlass_amd_backward_qt_bf16(x_e2m1.data_ptr(), x_e8m0.data_ptr(), h.data_ptr(), static_cast<const float*>(alpha.data_ptr()), B, N, M,
                                        xh_e2m1.data_ptr(), xh_e8m0.data_ptr(), current_stream(h)));
}

void backward_bf16_square_double_mxfp8(const Tensor& x_bf16, Tensor x_fp8, Tensor row_scales, Tensor column_scales) {
  const char* op = "backward_bf16_square_double_mxfp8";
  check_tensors(op, {{x_bf16, "x_bf16"}, {x_fp8, "x_fp8"}, {row_scales, "row_scales"}, {column_scales, "column_scales"}}, {}, false);
  STD_TORCH_CHECK(has_dtype(x_bf16, ScalarType::BFloat16) && x_bf16.dim() == 2, "x_bf16 must be a 2-D bf16 tensor");
  // x_bf16 may have any row count m: the outputs carry the padded extent m_pad = x_fp8.size(0) (a multiple of 128 >= m) and the kernel
  // treats the missing rows as zeros (the reference pads x_bf16 with a copy before the call, qutlass/__init__.py:288-290)
  STD_TORCH_CHECK(x_fp8.dim() == 2 && x_fp8.size(1) == x_bf16.size(1), "x_fp8 must be (m_pad, n)");
  const int64_t m = x_bf16.size(0), n = x_bf16.size(1), m_pad = x_fp8.size(0);
  STD_TORCH_CHECK(m_pad >= m && m_pad % 128 == 0, "x_fp8 must have a multiple of 128 rows, at least as many as x_bf16");
  STD_TORCH_CHECK(nbytes(row_scales) >= m_pad * n / 32 && nbytes(column_scales) >= m_pad * n / 32, "output tensors are too small");
  const torch::stable::accelerator::DeviceGuard guard(x_bf16.get_device_index());
  check_rc(qutlass_amd_backward_bf16_square_double_mxfp8_rows(x_bf16.data_ptr(), m, m_pad, n, x_fp8.data_ptr(), row_scales.data_ptr(), column_scales.data_ptr(),
                                                              current_stream(x_bf16)));
}

void mxfp4_transpose_mxfp8(const Tensor& x_fp4, const Tensor& scales, Tensor x_fp8, Tensor shared_exps) {
  const char* op = "mxfp4_transpose_mxfp8";
  check_tensors(op, {{x_fp4, "x_fp4"}, {scales, "scales"}, {x_fp8, "x_fp8"}, {shared_exps, "shared_exps"}}, {}, false);
  STD_TORCH_CHECK(x_fp4.dim() == 2 && x_fp4.element_size() == 1 && scales.element_size() == 1, "x_fp4 must be a 2-D 1-byte tensor, scales 1-byte");
  // any row count m: x_fp8 is (n, m_pad) with m_pad a multiple of 128 >= m; rows m .. m_pad-1 count as zero codes with unit scales
  // inside the kernel -- `scales` is read-only and needs only its m real rows (the reference pads x_fp4 with a copy and writes 1.0 into
  // the caller's scale tensor, qutlass/__init__.py:299-307)
  const int64_t m = x_fp4.size(0), n = x_fp4.size(1) * 2;
  STD_TORCH_CHECK(x_fp8.dim() == 2 && x_fp8.size(0) == n, "x_fp8 must be (n, m_pad)");
  const int64_t m_pad = x_fp8.size(1);
  STD_TORCH_CHECK(m_pad >= m && m_pad % 128 == 0, "x_fp8 must have a multiple of 128 columns, at least as many as x_fp4 has rows");
  STD_TORCH_CHECK(scales.numel() >= m * n / 32, "scales must hold one e8m0 per 32 elements");
  STD_TORCH_CHECK(nbytes(shared_exps) >= m_pad * n / 32, "output tensors are too small");
  const torch::stable::accelerator::DeviceGuard guard(x_fp4.get_device_index());
  check_rc(qutlass_amd_mxfp4_transpose_mxfp8_rows(x_fp4.data_ptr(), scales.data_ptr(), m, m_pad, n, x_fp8.data_ptr(), shared_exps.data_ptr(), current_stream(x_fp4)));
}

// ---- block-scale swizzle -------------------------------------------------------------------------------------------
Tensor to_blocked(const Tensor& in) {
  STD_TORCH_CHECK(in.dim() == 2, "to_blocked expects a 2-D matrix");
  STD_TORCH_CHECK(in.element_size() == 1, "Expected element size to be 1 byte (8 bits)");
  STD_TORCH_CHECK(in.is_contiguous(), "Input tensor must be contiguous");
  STD_TORCH_CHECK(in.is_cuda(), "to_blocked: expected a GPU tensor (no CPU path in qutlass_amd)");
  const int64_t rows = in.size(0), cols = in.size(1);
  const int64_t pr = (rows + 127) / 128 * 128, pc = (cols + 3) / 4 * 4;
  Tensor out = torch::stable::new_empty(in, {pr * pc});
  const torch::stable::accelerator::DeviceGuard guard(in.get_device_index());
  check_rc(qutlass_amd_to_blocked(in.data_ptr(), rows, cols, out.data_ptr(), current_stream(in)));
  return out;
}

}  // namespace

// Schema strings: bindings.cpp:499-513.  FRAGMENT, as in the reference (bindings.cpp:498): another library may add to `_qutlass_C`.
STABLE_TORCH_LIBRARY_FRAGMENT(_qutlass_C, m) {
  m.def("matmul_mxf4_bf16_tn(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha) -> Tensor");
  m.def("matmul_nvf4_bf16_tn(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha) -> Tensor");
  m.def("matmul_ada_mxf4_bf16_tn(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha) -> Tensor");
  m.def("matmul_mxf8_bf16_tn(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha) -> Tensor");
  m.def("matmul_mxf8_bf16_nn(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha) -> Tensor");
  m.def("fusedQuantizeMxQuest(Tensor A, Tensor R, Tensor OUT, Tensor OUT_sf) -> (Tensor, Tensor)");
  m.def("fusedQuantizeMxAbsMax(Tensor A, Tensor R, Tensor OUT, Tensor OUT_sf) -> (Tensor, Tensor)");
  m.def("fusedQuantizeNvQuest(Tensor A, Tensor R, Tensor OUT, Tensor OUT_sf, Tensor global_scale) -> (Tensor, Tensor)");
  m.def("fusedQuantizeNvAbsMax(Tensor A, Tensor R, Tensor OUT, Tensor OUT_sf, Tensor global_scale) -> (Tensor, Tensor)");
#ifndef QUTLASS_MINIMAL_BUILD   // the reference's trimmed build (bindings.cpp:254, :428, :508): inference ops only -- no clip-mask quantizer, no QAT-backward data prep
  m.def("fusedQuantizeMxQuestWithMask(Tensor A, Tensor R, Tensor OUT, Tensor OUT_sf, Tensor OUT_mask) -> (Tensor, Tensor, Tensor)");
  m.def("backward_t_bf16(Tensor x, Tensor h, Tensor xh_e2m1, Tensor xh_e8m0) -> ()");
  m.def("backward_qt_bf16(Tensor x_e2m1, Tensor x_e8m0, Tensor h, Tensor alpha, Tensor xh_e2m1, Tensor xh_e8m0) -> ()");
  m.def("backward_bf16_square_double_mxfp8(Tensor x_bf16, Tensor x_fp8, Tensor row_scales, Tensor column_scales) -> ()");
  m.def("mxfp4_transpose_mxfp8(Tensor x_fp4, Tensor scales, Tensor x_fp8, Tensor shared_exps) -> ()");
#endif
}

STABLE_TORCH_LIBRARY_FRAGMENT(qutlass_amd, m) {
  m.def("to_blocked(Tensor input_matrix) -> Tensor");
  // every op that fills caller tensors says so: `Tensor(a!)`, no aliasing return (see the note above fusedQuantizeMx_)
  m.def("fusedQuantizeMxBlocked(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, int method) -> ()");
  m.def("fusedQuantizeNvBlocked(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor global_scale, int method) -> ()");
  m.def("fusedQuantizeMx_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, int method) -> ()");
  m.def("fusedQuantizeNv_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor global_scale, int method) -> ()");
#ifndef QUTLASS_MINIMAL_BUILD
  m.def("fusedQuantizeMxMask_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor(c!) OUT_mask) -> ()");
  m.def("backward_t_bf16_(Tensor x, Tensor h, Tensor(a!) xh_e2m1, Tensor(b!) xh_e8m0) -> ()");
  m.def("backward_qt_bf16_(Tensor x_e2m1, Tensor x_e8m0, Tensor h, Tensor alpha, Tensor(a!) xh_e2m1, Tensor(b!) xh_e8m0) -> ()");
  m.def("backward_bf16_square_double_mxfp8_(Tensor x_bf16, Tensor(a!) x_fp8, Tensor(b!) row_scales, Tensor(c!) column_scales) -> ()");
  m.def("mxfp4_transpose_mxfp8_(Tensor x_fp4, Tensor scales, Tensor(a!) x_fp8, Tensor(b!) shared_exps) -> ()");
#endif
  m.def("siluAndMul_(Tensor X, Tensor(a!) OUT) -> ()");   // inference ops: in the minimal library too
  m.def("fusedSiluMulQuantizeMx_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, int method, bool blocked) -> ()");
  m.def("fusedSiluMulQuantizeNv_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor global_scale, int method, bool blocked) -> ()");
  m.def("fusedGatherQuantizeMx_(Tensor A, Tensor R, Tensor src_row, Tensor(a!) OUT, Tensor(b!) OUT_sf, int method) -> ()");
  m.def("fusedGatherQuantizeNv_(Tensor A, Tensor R, Tensor src_row, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor global_scale, int method) -> ()");
  m.def("fusedGatherQuantizeNvGrouped_(Tensor A, Tensor R, Tensor src_row, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor global_scales, Tensor offs, int method) -> ()");
  m.def("fusedSiluMulQuantizeNvGrouped_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, Tensor global_scales, Tensor offs, int method) -> ()");
  m.def("fusedQuantizeMxf8_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf) -> ()");   // OUT's dtype (float8_e4m3fn / float8_e5m2) selects the code format
  m.def("fusedQuantizeMxf8Blocked_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf) -> ()");
  m.def("fusedSiluMulQuantizeMxf8_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, bool blocked) -> ()");
  m.def("fusedGatherQuantizeMxf8_(Tensor A, Tensor R, Tensor src_row, Tensor(a!) OUT, Tensor(b!) OUT_sf) -> ()");
  m.def("moeCombine_(Tensor Y, Tensor pos, Tensor weights, Tensor(a!) OUT) -> ()");
  m.def("swigluOaiAndMul_(Tensor X, Tensor(a!) OUT, float alpha, float limit, Tensor bias, Tensor offs) -> ()");
  m.def("fusedSwigluOaiQuantizeMx_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, float alpha, float limit, Tensor bias, Tensor offs, int method) -> ()");
  m.def("fusedSwigluOaiQuantizeMxf8_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf, float alpha, float limit, Tensor bias, Tensor offs) -> ()");
  m.def("moeCombineBias_(Tensor Y, Tensor pos, Tensor weights, Tensor bias, Tensor offs, Tensor(a!) OUT) -> ()");
  m.def("moeTopkSoftmax_(Tensor logits, Tensor(a!) weights, Tensor(b!) ids, bool renormalize) -> ()");
  m.def("moeTopkGrouped_(Tensor logits, Tensor bias, Tensor(a!) weights, Tensor(b!) ids, Tensor(c!) scores, int n_group, int topk_group, int scoring, bool renormalize, float routed_scaling_factor) -> ()");
  m.def("moeSort_(Tensor topk_ids, Tensor expert_map, int num_experts, Tensor(a!) src_row, Tensor(b!) offs, Tensor(c!) pos, Tensor(d!) workspace) -> ()");
  m.def("fusedQuantizeMatmulMxf4(Tensor X, Tensor R, Tensor B, Tensor B_sf, Tensor alpha, int method) -> Tensor");
  // the one-launch routing for decode: functional ops that allocate their five results (weights, ids, src_row, offs, pos); inference ops: in the minimal library too
  m.def("moe_route_fused(Tensor logits, Tensor? expert_map, int topk, int num_experts, bool renormalize) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("moe_route_grouped_fused(Tensor logits, Tensor? bias, Tensor? expert_map, int topk, int num_experts, int n_group, int topk_group, int scoring, bool renormalize, float routed_scaling_factor) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("grouped_matmul_mxf4(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha, Tensor offs) -> Tensor");   // inference op: in the minimal library too
  m.def("grouped_matmul_mxf8(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha, Tensor offs) -> Tensor");   // inference op: in the minimal library too
  m.def("grouped_matmul_mxf8_mxf4(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha, Tensor offs) -> Tensor");   // W4A8, inference op: in the minimal library too
  m.def("grouped_matmul_mxf6_mxf4(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha, Tensor offs) -> Tensor");   // W4A6, inference op: in the minimal library too
  m.def("grouped_matmul_bf16_mxf4_bf16_tn(Tensor A, Tensor B, Tensor B_sf, Tensor alpha, Tensor offs, Tensor? src_row) -> Tensor");   // W4A16, inference op: in the minimal library too
  m.def("grouped_matmul_nvf4(Tensor A, Tensor B, Tensor A_sf, Tensor B_sf, Tensor alpha, Tensor offs) -> Tensor");   // inference op: in the minimal library too
}

// CUDA dispatch key only, as the reference (bindings.cpp:516-535); there is no CPU compute path.
// the in-place twins of the MXFP6 quantizers, in a namespace of their own: the set of output-filling ops of `qutlass_amd` is a pinned list (tests/test_op_tables_cpu.py)
STABLE_TORCH_LIBRARY_FRAGMENT(qutlass_amd_mxf6, m) {
  m.def("fusedQuantizeMxf6_(Tensor A, Tensor R, Tensor(a!) OUT, Tensor(b!) OUT_sf) -> ()");   // OUT (.., 3K/4) uint8: packed e2m3 codes
  m.def("fusedGatherQuantizeMxf6_(Tensor A, Tensor R, Tensor src_row, Tensor(a!) OUT, Tensor(b!) OUT_sf) -> ()");
}
STABLE_TORCH_LIBRARY_IMPL(qutlass_amd_mxf6, CUDA, m) {
  m.impl("fusedQuantizeMxf6_", TORCH_BOX(&fusedQuantizeMxf6_));
  m.impl("fusedGatherQuantizeMxf6_", TORCH_BOX(&fusedGatherQuantizeMxf6_));
}

STABLE_TORCH_LIBRARY_IMPL(_qutlass_C, CUDA, m) {
  m.impl("matmul_mxf4_bf16_tn", TORCH_BOX(&matmul_mxf4_bf16_tn));
  m.impl("matmul_nvf4_bf16_tn", TORCH_BOX(&matmul_nvf4_bf16_tn));
  m.impl("matmul_ada_mxf4_bf16_tn", TORCH_BOX(&matmul_ada_mxf4_bf16_tn));
  m.impl("matmul_mxf8_bf16_tn", TORCH_BOX(&matmul_mxf8_bf16_tn));
  m.impl("matmul_mxf8_bf16_nn", TORCH_BOX(&matmul_mxf8_bf16_nn));
  m.impl("fusedQuantizeMxQuest", TORCH_BOX(&fusedQuantizeMxQuest));
  m.impl("fusedQuantizeMxAbsMax", TORCH_BOX(&fusedQuantizeMxAbsMax));
  m.impl("fusedQuantizeNvQuest", TORCH_BOX(&fusedQuantizeNvQuest));
  m.impl("fusedQuantizeNvAbsMax", TORCH_BOX(&fusedQuantizeNvAbsMax));
#ifndef QUTLASS_MINIMAL_BUILD
  m.impl("fusedQuantizeMxQuestWithMask", TORCH_BOX(&fusedQuantizeMxQuestWithMask));
  m.impl("backward_t_bf16", TORCH_BOX(&backward_t_bf16));
  m.impl("backward_qt_bf16", TORCH_BOX(&backward_qt_bf16));
  m.impl("backward_bf16_square_double_mxfp8", TORCH_BOX(&backward_bf16_square_double_mxfp8));
  m.impl("mxfp4_transpose_mxfp8", TORCH_BOX(&mxfp4_transpose_mxfp8));
#endif
}
STABLE_TORCH_LIBRARY_IMPL(qutlass_amd, CUDA, m) {
  m.impl("to_blocked", TORCH_BOX(&to_blocked));
  m.impl("fusedQuantizeMxBlocked", TORCH_BOX(&fusedQuantizeMxBlocked));
  m.impl("fusedQuantizeNvBlocked", TORCH_BOX(&fusedQuantizeNvBlocked));
  m.impl("fusedQuantizeMx_", TORCH_BOX(&fusedQuantizeMx_));
  m.impl("fusedQuantizeNv_", TORCH_BOX(&fusedQuantizeNv_));
#ifndef QUTLASS_MINIMAL_BUILD
  m.impl("fusedQuantizeMxMask_", TORCH_BOX(&fusedQuantizeMxMask_));
  m.impl("backward_t_bf16_", TORCH_BOX(&backward_t_bf16));
  m.impl("backward_qt_bf16_", TORCH_BOX(&backward_qt_bf16));
  m.impl("backward_bf16_square_double_mxfp8_", TORCH_BOX(&backward_bf16_square_double_mxfp8));
  m.impl("mxfp4_transpose_mxfp8_", TORCH_BOX(&mxfp4_transpose_mxfp8));
#endif
  m.impl("siluAndMul_", TORCH_BOX(&siluAndMul_));
  m.impl("fusedSiluMulQuantizeMx_", TORCH_BOX(&fusedSiluMulQuantizeMx_));
  m.impl("fusedSiluMulQuantizeNv_", TORCH_BOX(&fusedSiluMulQuantizeNv_));
  m.impl("fusedGatherQuantizeMx_", TORCH_BOX(&fusedGatherQuantizeMx_));
  m.impl("fusedGatherQuantizeNv_", TORCH_BOX(&fusedGatherQuantizeNv_));
  m.impl("fusedGatherQuantizeNvGrouped_", TORCH_BOX(&fusedGatherQuantizeNvGrouped_));
  m.impl("fusedSiluMulQuantizeNvGrouped_", TORCH_BOX(&fusedSiluMulQuantizeNvGrouped_));
  m.impl("fusedQuantizeMxf8_", TORCH_BOX(&fusedQuantizeMxf8_));
  m.impl("fusedQuantizeMxf8Blocked_", TORCH_BOX(&fusedQuantizeMxf8Blocked_));
  m.impl("fusedSiluMulQuantizeMxf8_", TORCH_BOX(&fusedSiluMulQuantizeMxf8_));
  m.impl("fusedGatherQuantizeMxf8_", TORCH_BOX(&fusedGatherQuantizeMxf8_));
  m.impl("moeCombine_", TORCH_BOX(&moeCombine_));
  m.impl("swigluOaiAndMul_", TORCH_BOX(&swigluOaiAndMul_));
  m.impl("fusedSwigluOaiQuantizeMx_", TORCH_BOX(&fusedSwigluOaiQuantizeMx_));
  m.impl("fusedSwigluOaiQuantizeMxf8_", TORCH_BOX(&fusedSwigluOaiQuantizeMxf8_));
  m.impl("moeCombineBias_", TORCH_BOX(&moeCombineBias_));
  m.impl("moeTopkSoftmax_", TORCH_BOX(&moeTopkSoftmax_));
  m.impl("moeTopkGrouped_", TORCH_BOX(&moeTopkGrouped_));
  m.impl("moeSort_", TORCH_BOX(&moeSort_));
  m.impl("fusedQuantizeMatmulMxf4", TORCH_BOX(&fusedQuantizeMatmulMxf4));
  m.impl("grouped_matmul_mxf4", TORCH_BOX(&grouped_matmul_mxf4));
  m.impl("grouped_matmul_mxf8", TORCH_BOX(&grouped_matmul_mxf8));
  m.impl("grouped_matmul_mxf8_mxf4", TORCH_BOX(&grouped_matmul_mxf8_mxf4));
  m.impl("grouped_matmul_nvf4", TORCH_BOX(&grouped_matmul_nvf4));
}

// The functional routing ops and the W4A16 and W4A6 grouped GEMMs are registered for no particular device, like the functional ops of qutlass_amd/ops.py (CompositeExplicitAutograd: one kernel whatever
// the tensors' device; their own check_tensors turns a CPU tensor away with the message every op here gives).  The CUDA key stays the list of the ops that fill or
// allocate one result each, which tests/test_gpu_ext_rejections.py walks.
STABLE_TORCH_LIBRARY_IMPL(qutlass_amd, CompositeExplicitAutograd, m) {
  m.impl("moe_route_fused", TORCH_BOX(&moe_route_fused));
  m.impl("moe_route_grouped_fused", TORCH_BOX(&moe_route_grouped_fused));
  m.impl("grouped_matmul_bf16_mxf4_bf16_tn", TORCH_BOX(&grouped_matmul_bf16_mxf4));   // (an optional tensor, as theirs)
  m.impl("grouped_matmul_mxf6_mxf4", TORCH_BOX(&grouped_matmul_mxf6_mxf4));           // W4A6: its rejections are tests/test_gpu_grouped_w4a6.py's
}

// `import qutlass._CUDA` (reference: include/registration.h REGISTER_EXTENSION(_CUDA), bindings.cpp:537-540): an empty module
// whose only purpose is that loading it runs the registrations above.
// (QUTLASS_MINIMAL_BUILD drops it with the reference, bindings.cpp:537-540: such a library is loaded with torch.ops.load_library, not imported.)
#ifndef QUTLASS_MINIMAL_BUILD
extern "C" __attribute__((visibility("default"))) PyObject* PyInit__CUDA(void) {
  static struct PyModuleDef module = {PyModuleDef_HEAD_INIT, "_CUDA", nullptr, 0, nullptr};
  return PyModule_Create(&module);
}
#endif
