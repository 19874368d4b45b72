// The ONE list of the dense MX GEMMs' kernel forms (matmul_mxf4_bf16_tn, matmul_mxf8_bf16_tn with its _fmt / _nn relatives, matmul_ada_mxf4_bf16_tn), as NV_FORMS
// (gemm_nvf4.hip.h) is for NVFP4 and the GroupedFormat tables (gemm_mx_grouped.hip.h) are for the grouped ops.  Host code only: no kernel reads it.
// The values are the lab library's "gemm_variant" numbers: qutlass_amd_debug_gemm_plan / _ada_plan report them, profiles/ records them and the tests assert them.
// capi.hip's plans (mx_plan, plan_small, ks_plan, os_plan, os64_plan, os8_plan, os16_wide_plan, ada_plan) take a form's tile from its row, launch_mx_form launches a
// product form from its row, and qutlass_amd_debug_mx_forms hands the rows to the tests: a new form is a row here plus its kernel.
#pragma once
#include <stdint.h>

namespace qamd {

enum MxVariant : int {
  MXV_AUTO = 0,
  // pipelined schedule (gemm_mx_ringp) on a 2-deep LDS ring, two workgroups per CU: 128x128, 256x128 on eight waves, 128x64, 64x128, 64x64
  MXV_P128 = 24, MXV_P256x128_W8 = 25, MXV_P128x64 = 27, MXV_P64x128 = 28, MXV_P64 = 29,
  MXV_P256x128 = 58,                                                       // 256x128 on FOUR waves of 128x64, 3-deep ring, one workgroup per CU
  MXV_SKINNY = 60,                                                         // LDS-free split-K kernel (gemm_mx_skinny.hip.h): MXFP4, small M
  MXV_RING64 = 70, MXV_RING128x64 = 71, MXV_RING64x128 = 72, MXV_RING128 = 73,   // pipelined schedule on a 3-deep ring (+ split-K over caller scratch)
  MXV_PERSISTENT = 90,                                                     // persistent deep schedule, 256x256 (fp4: gemm_mx_deepp, fp8: gemm_mx_deepp8)
  MXV_HETERO = 98,                                                         // 90 over the full rounds + the residual tiles as 128x128 quarter tiles in the same grid
  MXV_KS32 = 561, MXV_KS32x64 = 562,                                       // K split inside the workgroup (gemm_mx_ks.hip.h), 32x32 / 32x64 tiles: MXFP4
  MXV_OS32 = 568, MXV_OS16 = 569, MXV_OS64 = 570,                          // wave-owned K stages (gemm_mx_os.hip.h): 32x32, 32x16, 64x32 tiles
  MXV_D16 = 571, MXV_D32 = 572, MXV_D48 = 573, MXV_D56 = 574, MXV_D64 = 575,   // its decode form: 16 x (16 / 32 / 48 / 56 / 64) tiles on the 16x16x128 MFMA
};
// MXF_PIPELINED: mid-size and large outputs, one K range; MXF_RING: the small-output regime, the forms the plans may split along K
enum MxFamily : int { MXF_PIPELINED, MXF_RING, MXF_PERSISTENT, MXF_HETERO, MXF_SKINNY, MXF_KSPLIT, MXF_OS, MXF_DECODE };
// the ops a form has a kernel for: MXFP4, MXFP8 with an e4m3 / e5m2 A operand (blocked scales), matmul_ada_mxf4_bf16_tn (MXFP4, row-major scales)
enum MxOp : int { MXOP_F4 = 1, MXOP_F8 = 2, MXOP_F8_E5M2 = 4, MXOP_ADA = 8, MXOP_TN = MXOP_F4 | MXOP_F8 | MXOP_F8_E5M2, MXOP_ALL = MXOP_TN | MXOP_ADA };
constexpr int mx_op(int ebits, int afmt, bool rm) { return rm ? MXOP_ADA : ebits == 4 ? MXOP_F4 : afmt == 1 ? MXOP_F8_E5M2 : MXOP_F8; }

// tm x tn: rows x columns of a workgroup's tile; wm x wn: its wave grid; depth: LDS ring depth (MXF_HETERO: of the quarter tiles, which are tm / 2 x tn / 2;
// MXF_KSPLIT: up to 24 K stages of 256, 6 beyond; MXF_SKINNY: 16-byte segments per wave per trip; the wave-owned families size their slots by K in the launcher);
// product: a product plan can return it (the lab library forces any row, and knows more numbers than these: capi.hip dispatch_lab_variant)
struct MxFormRow { int variant, family, tm, tn, wm, wn, depth, ops; bool product; };
constexpr MxFormRow MX_FORMS[] = {
    {MXV_P128, MXF_PIPELINED, 128, 128, 2, 2, 2, MXOP_TN, true},   {MXV_P256x128_W8, MXF_PIPELINED, 256, 128, 4, 2, 2, MXOP_TN, true},
    {MXV_P128x64, MXF_PIPELINED, 128, 64, 2, 2, 2, MXOP_TN, true}, {MXV_P64x128, MXF_PIPELINED, 64, 128, 2, 2, 2, MXOP_TN, true},
    {MXV_P64, MXF_PIPELINED, 64, 64, 2, 2, 2, MXOP_TN, true},      {MXV_P256x128, MXF_PIPELINED, 256, 128, 2, 2, 3, MXOP_TN, true},
    {MXV_SKINNY, MXF_SKINNY, 32, 32, 8, 1, 4, MXOP_F4 | MXOP_ADA, true},
    {MXV_RING64, MXF_RING, 64, 64, 2, 2, 3, MXOP_ALL, true},  {MXV_RING128x64, MXF_RING, 128, 64, 2, 2, 3, MXOP_TN, true},
    {MXV_RING64x128, MXF_RING, 64, 128, 2, 2, 3, MXOP_TN, true}, {MXV_RING128, MXF_RING, 128, 128, 2, 2, 3, MXOP_TN, true},
    {MXV_PERSISTENT, MXF_PERSISTENT, 256, 256, 2, 2, 2, MXOP_TN, true}, {MXV_HETERO, MXF_HETERO, 256, 256, 2, 2, 4, MXOP_TN, true},
    {MXV_KS32, MXF_KSPLIT, 32, 32, 4, 1, 4, MXOP_F4, true},    {MXV_KS32x64, MXF_KSPLIT, 32, 64, 4, 1, 4, MXOP_F4, true},
    {MXV_OS32, MXF_OS, 32, 32, 4, 1, 0, MXOP_ALL, true},       {MXV_OS16, MXF_OS, 32, 16, 4, 1, 0, MXOP_ALL, true},   {MXV_OS64, MXF_OS, 64, 32, 4, 1, 0, MXOP_ALL, true},
    // (ascending columns: os16_form takes the first that leaves one workgroup per CU)
    {MXV_D16, MXF_DECODE, 16, 16, 4, 1, 0, MXOP_ALL, true},    {MXV_D32, MXF_DECODE, 16, 32, 4, 1, 0, MXOP_ALL, true}, {MXV_D48, MXF_DECODE, 16, 48, 4, 1, 0, MXOP_ALL, true},
    {MXV_D56, MXF_DECODE, 16, 56, 4, 1, 0, MXOP_ALL, true},    {MXV_D64, MXF_DECODE, 16, 64, 4, 1, 0, MXOP_ALL, true},
};
constexpr int MX_NFORMS = (int)(sizeof(MX_FORMS) / sizeof(MX_FORMS[0]));
constexpr const MxFormRow* mx_form(int v) {
  for (const MxFormRow& f : MX_FORMS)
    if (f.variant == v) return &f;
  return nullptr;
}
// a form named at compile time: a variant without a row does not compile
template <int V>
inline constexpr MxFormRow kMxForm = *mx_form(V);
// workgroups (per K range) of form V on an M x N output
template <int V>
constexpr int64_t mx_tiles(int64_t M, int64_t N) {
  return ((M + kMxForm<V>.tm - 1) / kMxForm<V>.tm) * ((N + kMxForm<V>.tn - 1) / kMxForm<V>.tn);
}

}  // namespace qamd
