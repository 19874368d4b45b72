// C ABI (include/qutlass_amd.h) -> kernel launches.  No torch types, no allocation, no sync.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>

#include "../../include/qutlass_amd.h"
#include "gemm_mx.hip.h"
#include "gemm_mx_forms.hip.h"
#include "gemm_mx_deepp.hip.h"
#include "gemm_mx_deepp16.hip.h"
#if QAMD_BENCH   // csrc/lab/: sources of the LAB library only -- not read by the product build, not shipped by setup.py
#include "lab/gemm_mx_duo.hip.h"         // [r6] the 8-wave persistent kernel (built, bit-identical, slower under the power cap: DESIGN.md section 7)
#include "lab/gemm_mx_deepp_lab.hip.h"   // the lab copy (namespace qamd::labk): traces, ablations, stream-K, retirement experiments
#endif
#include "gemm_mx_skinny.hip.h"
#include "gemm_mx_ks.hip.h"
#include "gemm_mx_os.hip.h"
#include "gemm_mx_os_w4a8.hip.h"
#include "gemm_mx_os_w4a16.hip.h"
#include "gemm_mx_os_w4a6.hip.h"
#include "gemm_mx_fusedq.hip.h"
#include "gemm_nvf4.hip.h"
#include "gemm_nvf4_pk.hip.h"
#include "gemm_nvf4_os.hip.h"
#include "quantize.hip.h"
#include "moe_route.hip.h"
#include "to_blocked.hip.h"
#include "transpose_u8.hip.h"
#include "quartet_bwd.hip.h"
#if QAMD_BENCH
#include "lab/quartet_bwd_lab.hip.h"     // backward_qt_bf16's whole-line panel kernel (built, bit-identical, not faster)
#endif

using namespace qamd;

// One source, several translation units, two libraries.
//   libqutlass_amd.so        the PRODUCT: the C ABI of include/qutlass_amd.h and exactly the kernels its dispatch rules can
//                            reach.  No process-wide switch can change which kernel runs or what it computes: qutlass_amd_set_option
//                            knows no key ([r4] the "hw_fp4_cvt" encoder switch of rounds 1-3 lives in the lab build only).
//   libqutlass_amd_bench.so  the LAB (-DQAMD_BENCH=1): the same entry points plus every schedule variant, ablation, trace
//                            and clock-probe instantiation the design record cites, selectable through
//                            qutlass_amd_set_option("gemm_variant" / "nvf4_variant" / "pp_flags" / ...).  Only
//                            tests/native, the sweeps under tools/ and the forced-tile parity tests load it.
// build.py compiles this file once per QAMD_TU value in parallel: every heavy template family is instantiated in exactly
// one unit (explicit instantiation) and only declared (`extern template`) in the others.  QAMD_TU = 0 (a plain
// `hipcc capi.hip`) still gives a whole library in one unit.
//   1  C entry points, dispatch rules, small kernels      2  MXFP4 tile / schedule variants      3  MXFP8 variants
//   4  NVFP4 kernels + MXFP8 with an e5m2 A operand        5  fused quantizers
//   6  MXFP4 ablations (100+, 200+, 300+; lab only)       7  NVFP4 v2 ablations (gemm_nvf4.hip.h; lab only)
//   8  the persistent NVFP4 kernel (gemm_nvf4_pk.hip.h)
#ifndef QAMD_TU
#define QAMD_TU 0
#endif
#define QAMD_DEF(n) (QAMD_TU == 0 || QAMD_TU == (n))
#ifndef QAMD_BENCH
#define QAMD_BENCH 0
#endif

namespace qamd_host {

#if QAMD_DEF(1)
thread_local char g_err[512] = "";
#if QAMD_BENCH
std::atomic<int> g_hw_fp4_cvt{1};   // lab: 0 = the software e2m1 encoder (device-verified bit-identical to v_cvt_scalef32_pk_fp4_f32, tests/native/probe.hip P2)
std::atomic<int> g_gemm_variant{0};
std::atomic<int> g_nvf4_variant{0};
std::atomic<int> g_splitk_wg{0};        // split-K: target workgroup count ("splitk_wg"; one per CU measured best, profiles/native_r1_splitk_wg.log)
std::atomic<int> g_splitk_min_kt{32};   // split-K: minimum number of 128-byte K stages ("splitk_min_kt"; 16 loses at K = 4096, 48 leaves K = 8192 .. 11008 unsplit)
std::atomic<int> g_transpose_nc{0};     // lab: kernel forcing of mxfp4_transpose_mxfp8 (128 / 256 / 3 / 4 / 2) and backward_bf16_square_double_mxfp8 (1 / 4 / 8); 0 = the product rules
std::atomic<int> g_pp_shift{2};
std::atomic<int> g_pp_flags{1};
std::atomic<int> g_quant_wg_per_cu{0};  // 0 = auto
std::atomic<int> g_deepp_grid{0};       // lab: workgroups of the persistent deep kernels (0 = the balanced-rounds rule)
std::atomic<int> g_bwd_variant{0};      // lab: 1 = the round-3 backward_t / backward_qt kernel (8 waves meeting at two barriers per tile) instead of the wave-owned-lines one
std::atomic<int> g_moe_sort_one_launch_max{0};   // lab: moe_sort's one-workgroup bound in slots (0 = the product's; 1 forces the three-launch form from two slots on)
std::atomic<int> g_splitk_force{0};     // lab: K splits for a FORCED ring variant ("gemm_variant" 70..73); 0 = the plan's
std::atomic<uint32_t*> g_dbg{nullptr};
#endif

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(QAMD_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return QAMD_OK;
}

// Per-launch number of the fused split-K kernels (host state only; no device memory behind it): starts at a value drawn
// from the clock and the process, then counts up.  56 bits of it tag the arrival slots of one launch.
unsigned long long next_launch_tag() {
  static std::atomic<unsigned long long> tag{[] {
    unsigned long long x = (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count() ^ ((unsigned long long)(uintptr_t)&g_err << 17);
    x ^= x >> 31; x *= 0x9e3779b97f4a7c15ull; x ^= x >> 29;
    return x | 1ull;
  }()};
  return tag.fetch_add(1, std::memory_order_relaxed) + 1;
}
#else
unsigned long long next_launch_tag();
#if QAMD_BENCH
extern std::atomic<int> g_hw_fp4_cvt, g_gemm_variant, g_nvf4_variant, g_splitk_wg, g_splitk_min_kt, g_transpose_nc, g_pp_shift, g_pp_flags, g_quant_wg_per_cu, g_splitk_force, g_deepp_grid, g_bwd_variant, g_moe_sort_one_launch_max;
extern std::atomic<uint32_t*> g_dbg;
#endif
int fail(int code, const char* fmt, ...);
int check_launch(const char* what);
#endif

// Tuning state.  In the product library these are compile-time constants: nothing a caller (or another thread) does can
// change which kernel a shape gets.  The lab library reads them from qutlass_amd_set_option().
#if QAMD_BENCH
inline bool opt_hw_fp4() { return g_hw_fp4_cvt.load() != 0; }
inline int opt_gemm_variant() { return g_gemm_variant.load(); }
inline int opt_nvf4_variant() { return g_nvf4_variant.load(); }
inline int opt_splitk_wg() { return g_splitk_wg.load(); }   // 0 = one workgroup per CU
inline int opt_splitk_min_kt() { return g_splitk_min_kt.load(); }
inline int opt_transpose_nc() { return g_transpose_nc.load(); }
inline int opt_pp_shift() { return g_pp_shift.load(); }
inline int opt_pp_flags() { return g_pp_flags.load(); }
inline int opt_quant_wg_per_cu() { return g_quant_wg_per_cu.load(); }
inline int opt_splitk_force() { return g_splitk_force.load(); }
inline int opt_deepp_grid() { return g_deepp_grid.load(); }
inline int opt_bwd_variant() { return g_bwd_variant.load(); }
inline int opt_moe_sort_one_launch_max() { return g_moe_sort_one_launch_max.load(); }
inline uint32_t* opt_dbg() { return g_dbg.load(); }
#else
constexpr bool opt_hw_fp4() { return true; }   // the product ships ONE e2m1 encoder: the hardware convert
constexpr int opt_gemm_variant() { return 0; }
constexpr int opt_nvf4_variant() { return 0; }
constexpr int opt_splitk_wg() { return 0; }
constexpr int opt_splitk_min_kt() { return 32; }
constexpr int opt_transpose_nc() { return 0; }
constexpr int opt_pp_shift() { return 2; }
constexpr int opt_pp_flags() { return 1; }
constexpr int opt_quant_wg_per_cu() { return 0; }
constexpr int opt_splitk_force() { return 0; }
constexpr int opt_deepp_grid() { return 0; }
constexpr int opt_bwd_variant() { return 0; }
constexpr int opt_moe_sort_one_launch_max() { return 0; }
constexpr uint32_t* opt_dbg() { return nullptr; }
#endif

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Compute units of the current device, asked once per device (hipDeviceAttributeMultiprocessorCount: 256 on an MI355X in SPX
// mode; fewer in a partitioned / CU-masked configuration).  Every grid size and occupancy threshold below derives from it.
// (The kernels' blockIdx -> XCD remap assumes the dispatcher's round-robin over 8 XCDs; it is a bijection for any grid, so
// on another XCD count it only costs L2 locality.)  The dispatch rules take the count as an argument: the debug entries pass 256.
#if QAMD_DEF(1)
int chip_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cache[dev].load(std::memory_order_relaxed);
  if (v <= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
    v = n;
  }
  return v;
}
#else
int chip_cus();
#endif


template <class C, int PP>
int launch_gemm(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, C::BM);
  p.tiles_n = (int)cdiv(p.N, C::BN);
  p.raster_magic = raster_magic(p.tiles_n);
  if (PP != 7 && PP != 9) { p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0; }   // only the (blocked-scale) ring schedules know about split-K
  hipLaunchKernelGGL((gemm_mx_kernel<C, PP>), dim3(p.tiles_m * p.tiles_n, p.splits), dim3(C::THREADS), 0, s, p);
  return check_launch("gemm_mx_kernel");
}

// Workgroups of a persistent deep launch over T tiles of 256x256 on the 256 CUs of an MI355X (one 512-register workgroup per
// CU): BALANCED rounds -- R = ceil(T / 256) tiles per workgroup, G = ceil(T / R) workgroups rounded up to a multiple of 8 (one
// share per XCD) -- instead of 256 workgroups with a ragged last round.  The kernels run at the socket power limit, so the CUs
// a smaller grid leaves idle are not lost: the others clock higher (896 tiles: 224 workgroups x 4 tiles beat 256 workgroups
// x 3.5 rounds, profiles/native_r2_deepp_grid.log).
inline int deepp_grid(int tiles) {
  const int forced = opt_deepp_grid();
  if (forced > 0) return std::min(forced, tiles);
  const int cus = chip_cus();
  const int rounds = (tiles + cus - 1) / cus;
  const int g = ((tiles + rounds - 1) / rounds + 7) / 8 * 8;
  return std::min(std::min(g, cus), tiles);
}

// persistent deep schedule (gemm_mx_deepp.hip.h): one workgroup per CU walks the tiles; 136 KiB of static LDS
// ONEFORM: MFMA shape of the one-tile form (grid == tile count, even stage count): 0 = the product's choice (kDeeppOneTile16, gemm_mx_deepp16.hip.h); 32 / 16 force
// v_mfma_scale_f32_32x32x64 / _16x16x128 (lab: "gemm_variant" 190 / 191, so that both can be timed in one process and small grids reach either); 160 + KL forces the
// 16x16x128 form with the K loop KL (gemm_mx_deepp16.hip.h KL_ bits; lab: 192 ... 197), 16 is the one the product runs (kDeepp16KLoop)
template <class C, bool TRACE = false, int ST_AUX = 0, int LAB = 0, int ONEFORM = 0>
int launch_gemm_deepp(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, C::BM);
  p.tiles_n = (int)cdiv(p.N, C::BN);
  p.raster_magic = raster_magic(p.tiles_n);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  const int grid = deepp_grid(p.tiles_m * p.tiles_n);
#if QAMD_BENCH
#ifdef QAMD_ROUTE_LABK   // side builds for schedule A/Bs (tools/build_variant.py --lab ... -DQAMD_ROUTE_LABK): the plain entry runs the LAB copy of the kernel, no ablation
  if constexpr (!TRACE && LAB == 0) {
    hipLaunchKernelGGL((labk::gemm_mx_deepp_kernel<C, false, ST_AUX, 8>), dim3(grid), dim3(C::THREADS), 0, s, p);
    return check_launch("labk::gemm_mx_deepp_kernel");
  }
#endif
  if constexpr (TRACE || LAB != 0) {   // stage traces and result-changing ablations: the lab copy of the kernel
    hipLaunchKernelGGL((labk::gemm_mx_deepp_kernel<C, TRACE, ST_AUX, LAB>), dim3(grid), dim3(C::THREADS), 0, s, p);
    return check_launch("labk::gemm_mx_deepp_kernel");
  }
#else
  static_assert(!TRACE && LAB == 0, "traces / ablations: lab build only");
#endif
  // [r6] two host-side choices of the kernel form (gemm_mx_deepp.hip.h): ODD -- an odd number (>= 3) of K stages runs without the empty stage; ONETILE -- every workgroup
  // walks exactly one tile (grid == tile count), so nothing is prefetched for a next tile
  const int64_t kt = cdiv((int64_t)p.K * C::EBITS / 8, 128);
  const bool odd = (kt & 1) && kt >= 3, one = grid == p.tiles_m * p.tiles_n;
  if (odd && one) hipLaunchKernelGGL((gemm_mx_deepp_kernel<C, ST_AUX, true, true>), dim3(grid), dim3(C::THREADS), 0, s, p);
  else if (odd) hipLaunchKernelGGL((gemm_mx_deepp_kernel<C, ST_AUX, true, false>), dim3(grid), dim3(C::THREADS), 0, s, p);
  else if (one) {
    static_assert(ONEFORM == 0 || ONEFORM == 16 || ONEFORM == 32 || (ONEFORM >= 160 && ONEFORM < 168), "one-tile form");
    static_assert(ONEFORM == 0 || QAMD_BENCH, "forced one-tile forms: lab build only");
    if constexpr (ONEFORM >= 160) hipLaunchKernelGGL((gemm_mx_deepp16_kernel<C, ST_AUX, ONEFORM - 160>), dim3(grid), dim3(C::THREADS), 0, s, p);
    else if constexpr (ONEFORM == 16 || (ONEFORM == 0 && kDeeppOneTile16)) hipLaunchKernelGGL((gemm_mx_deepp16_kernel<C, ST_AUX>), dim3(grid), dim3(C::THREADS), 0, s, p);
    else hipLaunchKernelGGL((gemm_mx_deepp_kernel<C, ST_AUX, false, true>), dim3(grid), dim3(C::THREADS), 0, s, p);
  }
  else hipLaunchKernelGGL((gemm_mx_deepp_kernel<C, ST_AUX>), dim3(grid), dim3(C::THREADS), 0, s, p);
  return check_launch("gemm_mx_deepp_kernel");
}

#if QAMD_BENCH
// [r6] the 8-wave persistent schedule (lab/gemm_mx_duo.hip.h): same grid rule, 144 KiB of static LDS.  RET: retirement placement (0 burst, 1 behind the last k-slice)
template <class C, int ST_AUX = 17, int RET = 0, bool TRACE = false>
int launch_gemm_duo(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, C::BM);
  p.tiles_n = (int)cdiv(p.N, C::BN);
  p.raster_magic = raster_magic(p.tiles_n);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  const int grid = deepp_grid(p.tiles_m * p.tiles_n);
  hipLaunchKernelGGL((gemm_mx_duo_kernel<C, ST_AUX, RET, TRACE>), dim3(grid), dim3(C::THREADS), 0, s, p);
  return check_launch("gemm_mx_duo_kernel");
}
#endif

// [r6] small-batch kernel with the K split inside the workgroup (gemm_mx_ks.hip.h): one 32x32 / 32x64 / 64x32 tile per workgroup of four waves
template <int TM, int TN, int D = 8>
int launch_gemm_ks(GemmParams p, hipStream_t s) {
  using C = KsCfg<TM, TN, D>;
  p.tiles_m = (int)cdiv(p.M, TM);
  p.tiles_n = (int)cdiv(p.N, TN);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  hipLaunchKernelGGL((gemm_mx_ks_kernel<C>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, s, p);
  return check_launch("gemm_mx_ks_kernel");
}

// [r6] small-batch kernel whose waves own K stages (gemm_mx_os.hip.h): wave w owns stages w, w + 4, ...; the tile's whole K extent requested up front while it fits the
// LDS (16 stages of 128 bytes per row for a 32-row tile, 12 for a 64-row tile), wave-owned rings beyond
// (RM: row-major scale operands -- matmul_ada_mxf4_bf16_tn; TN: columns per workgroup, 32 or 16; EBITS 8: MXFP8, AFMT 1: e5m2 A operand; TM: rows per workgroup, 32 or 64)
// the kernel by the K stage count, for the dense op (GRP false: p is GemmParams) and the grouped one (GroupedParams, row-major scales): slots per wave = ceil(KT / 4) up to
// SMAX, the most that fit the LDS; wave-owned rings of SMAX slots beyond
template <bool RM, int TN, int EBITS, int TM, int AFMT, bool GRP, class P>
void launch_os_by_stages(int64_t KT, dim3 grid, const P& p, hipStream_t s) {
  const dim3 block(256);
  constexpr int SMAX = TM == 32 ? 4 : 3;
  if (KT <= 4) hipLaunchKernelGGL((gemm_mx_os_kernel<OsCfg<1, TN, EBITS, TM, AFMT>, RM, false, GRP>), grid, block, 0, s, p);
  else if (KT <= 8) hipLaunchKernelGGL((gemm_mx_os_kernel<OsCfg<2, TN, EBITS, TM, AFMT>, RM, false, GRP>), grid, block, 0, s, p);
  else if (KT <= 12) hipLaunchKernelGGL((gemm_mx_os_kernel<OsCfg<3, TN, EBITS, TM, AFMT>, RM, false, GRP>), grid, block, 0, s, p);
  else if (KT <= 4 * SMAX) hipLaunchKernelGGL((gemm_mx_os_kernel<OsCfg<SMAX, TN, EBITS, TM, AFMT>, RM, false, GRP>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((gemm_mx_os_kernel<OsCfg<SMAX, TN, EBITS, TM, AFMT>, RM, true, GRP>), grid, block, 0, s, p);
}
template <bool RM = false, int TN = 32, int EBITS = 4, int TM = 32, int AFMT = 0>
int launch_gemm_os(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, TM);
  p.tiles_n = (int)cdiv(p.N, TN);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  launch_os_by_stages<RM, TN, EBITS, TM, AFMT, false>(cdiv((int64_t)p.K * EBITS / 8, 128), dim3(p.tiles_m * p.tiles_n), p, s);
  return check_launch("gemm_mx_os_kernel");
}
// [r6] its decode form (gemm_mx_os16_kernel: 16 x TN tiles on the 16x16x128 MFMA, rows in tiles of 16): one shot while the tile's K extent fits the LDS (SMAX slots per wave),
// wave-owned rings of SMAX slots beyond
template <int EBITS = 4, int AFMT = 0, bool RM = false, int TN = 16>
int launch_gemm_os16(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, 16);
  p.tiles_n = (int)cdiv(p.N, TN);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  const int64_t KT = cdiv((int64_t)p.K * EBITS / 8, 128);
  const dim3 grid(p.tiles_m * p.tiles_n), block(256);
  constexpr int STAGE = Os16Cfg<1, EBITS, AFMT, TN>::STAGE;
  constexpr int SFIT = 160 * 1024 / (4 * STAGE), SMAX = SFIT >= 8 ? 8 : SFIT >= 4 ? 4 : SFIT;   // slots per wave that fit the LDS: 8 (TN = 16), 4 (32 ... 56), 3 (64)
  static_assert(SMAX >= 3, "LDS budget");
  if (KT <= 4) hipLaunchKernelGGL((gemm_mx_os16_kernel<Os16Cfg<1, EBITS, AFMT, TN>, false, RM>), grid, block, 0, s, p);
  else if (KT <= 8) hipLaunchKernelGGL((gemm_mx_os16_kernel<Os16Cfg<2, EBITS, AFMT, TN>, false, RM>), grid, block, 0, s, p);
  else if (KT <= 16 && SMAX >= 4) hipLaunchKernelGGL((gemm_mx_os16_kernel<Os16Cfg<(SMAX >= 4 ? 4 : SMAX), EBITS, AFMT, TN>, false, RM>), grid, block, 0, s, p);
  else if (KT <= 4 * SMAX) hipLaunchKernelGGL((gemm_mx_os16_kernel<Os16Cfg<SMAX, EBITS, AFMT, TN>, false, RM>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((gemm_mx_os16_kernel<Os16Cfg<SMAX, EBITS, AFMT, TN>, true, RM>), grid, block, 0, s, p);
  return check_launch("gemm_mx_os16_kernel");
}
// the decode form for M <= 16: the narrowest of its column tiles (MX_FORMS: 16 / 32 / 48 / 56 / 64) that leaves at most one workgroup per CU; nullptr = none does
inline const MxFormRow* os16_form(int64_t N, int64_t cus) {
  for (const MxFormRow& f : MX_FORMS)
    if (f.family == MXF_DECODE && cdiv(N, f.tn) <= cus) return &f;
  return nullptr;
}
// [r6] M <= 16 against a weight too wide for 16-column workgroups: the decode form with 32 / 48 / 56 / 64 columns per workgroup (variants 572 ... 575) where it was measured ahead
// (tools/calib_os2.py, profiles/calib_os16w_r7.txt; K in stages of 128 bytes per row).  MXFP4: N = 11008 / 12288 x K = 4096 5.0-5.2 -> 3.8-4.0 us (48 columns: 64 rows per
// stage where the 32x64 K-split ring kernel fetched 96 and met at a barrier per stage), 14336 x 4096 5.9-6.1 -> 4.6-4.9 (56 columns = exactly 256 workgroups), 12288 x 5120
// 7.5-8.0 -> 5.6-6.1, 16384 x 4096 -7 %; N = 5120 ... 8192 (32 columns against the 32x32 form's 64 rows per stage) -3 ... -7 % at K = 3072 ... 8192, +3 % at K = 2048.
// Past the one-shot range the wider forms lose (14336 x 8192: +3 %).  MXFP8: 32 columns -6 ... -12 % at K = 2048 ... 8192, 48 columns -9 % at 11008 x 4096; 14336 x 4096 loses.
// Returns the variant or 0.
inline int os16_wide_plan(int ebits, int64_t N, int64_t K, int64_t cus) {
  const MxFormRow* f = os16_form(N, cus);
  const int tn = f ? f->tn : 0;
  const int64_t KT = cdiv(K * ebits / 8, 128);
  if (ebits == 4) {
    if (tn == 32) return (KT >= 12 && KT <= 32) ? f->variant : 0;
    if (tn == 48) return (KT >= 8 && KT <= 24) ? f->variant : 0;
    if (tn == 56) return (KT >= 8 && KT <= 16) ? f->variant : 0;
    if (tn == 64) return (KT >= 8 && KT <= 16) ? f->variant : 0;
    return 0;
  }
  if (tn == 32) return (KT >= 16 && KT <= 64) ? f->variant : 0;
  if (tn == 48) return (KT >= 16 && KT <= 32) ? f->variant : 0;
  return 0;
}
// Does the one-shot kernel take the shape, and with how many columns per workgroup?  Returns 0 (no), 32 or 16.  32x32 tiles, one per CU at most; 16 columns per
// workgroup whenever that still leaves one workgroup per CU (N = 4096, M <= 32: 256 workgroups pulling half the bytes each -- 3.34 -> 3.22 us at K = 4096, 7.8 -> 6.9 at
// K = 14336).  K <= 16 stages of 256: always.  Longer K (wave-owned rings): up to 32 stages when the tiles fill a quarter of the chip, up to 64 stages (K = 16384) when
// they fill half of it (N = 1024, K = 14336: 32 workgroups take 7.4 us where the split-K plans take 5.7-6.9); with 32 columns per workgroup the blocked-scale op also keeps
// M < 8 against more than 32 stages on the LDS-free split-K kernel (4096 x 11008, M = 1: 6.07 vs 6.40 us).  ada: matmul_ada_mxf4_bf16_tn (row-major scales: its other
// kernels are 25-45 % slower on every such shape).  profiles/calib_os_r6q.txt, calib_osring_r6q.txt, calib_ada_r6q.txt, calib_os16_r6s.txt
inline int os_plan(int64_t M, int64_t N, int64_t K, int64_t cus, bool ada = false) {
  const int64_t T32 = mx_tiles<MXV_OS32>(M, N), T16 = mx_tiles<MXV_OS16>(M, N), KT = cdiv(K, 256);
  if (T32 > cus) return 0;
  const int tn = T16 <= cus ? 16 : 32;
  if (KT <= 16) return tn;
  if (KT <= 32) return 4 * T32 >= cus ? tn : 0;
  if (KT > 64 || 2 * T32 < cus) return 0;   // (measured with 128 and 256 tiles only: fewer tiles against K > 8192 stay with the split plans)
  return (ada || M >= 8 || tn == 16) ? tn : 0;
}

// [r6, third session] ... and its 64-row form (variant 570: two m-tiles per stage owner) for MXFP4 batches whose 32x32 tiles no longer fit one per CU while 64x32 tiles do
// (M = 65 ... 128 at N = 4096, M = 33 ... 64 at N = 8192).  A 64x32 tile's K extent fits the LDS up to 12 stages (K <= 3072) -- there it is the one-shot kernel and wins
// 8-13 % (4096 x 2048, M = 96 / 128: 4.10 / 4.14 -> 3.57 / 3.63 us; 2048^2, M = 160 ... 256: 4.07-4.22 -> 3.51-3.70).  Beyond, the wave-owned rings hold three stages per
// wave and a fourth costs a second memory round trip: K = 4096 ... 6144 lose 0-8 % against the 64x64 ring tiles (N = K = 4096, M = 128: 5.20 vs 5.60 us) and stay there; from
// ~40 stages on the round trips overlap and it wins again (4096 x 11008, M = 96 / 128: 12.05 / 12.59 -> 9.19 / 9.73; x 14336: 13.5 / 14.1 -> 11.7 / 12.4; 8192^2, M = 64,
// 32 stages on every CU: 11.65 -> 9.66).  profiles/calib_os2_fp4_r7.txt
// ada: matmul_ada_mxf4_bf16_tn has no scratch argument, so no split-K plan competes -- every measured K wins there (4096 x 4096, M = 96 / 128: 6.5 / 6.7 -> 6.0 / 6.3 us;
// x 8192: 10.1 -> 8.9; x 14336: 20.9 / 22.6 -> 14.4 / 15.3; profiles/calib_ada_570_r7.txt)
inline bool os64_plan(int64_t M, int64_t N, int64_t K, int64_t cus, bool ada = false) {
  const int64_t T32 = mx_tiles<MXV_OS32>(M, N), T64 = mx_tiles<MXV_OS64>(M, N), KT = cdiv(K, 256);
  if (T32 <= cus || T64 > cus) return false;
  if (ada) return KT <= 64;
  return KT <= 12 || (KT >= 40 && KT <= 64) || (KT >= 32 && KT < 40 && T64 == cus && M <= 64);   // (the last: 8192^2, M = 64; 4096 x 8192, M = 128 -- two tile rows -- loses 3 %)
}
// [r6, third session] The same kernel on MXFP8 operands (EBITS = 8: a stage is 128 elements, so K = 4096 is 32 stages and the one-shot form ends at K = 2048): returns the
// variant (568 = 32x32 tiles, 569 = 32x16, 570 = 64x32) or 0.  Measured against the plans below -- 64x64 ring tiles, split-K with caller scratch -- on M = 1 ... 256 x 21
// (N, K) (tools/calib_os2.py, profiles/calib_os2_fp8_r7.txt): N = K = 4096, M = 1 ... 32 5.9-7.0 -> 4.8-5.4 us, M = 64 8.6 -> 6.4; 8192 x 4096, M <= 32 10.3-10.7 -> 6.0-7.0;
// N = K = 2048, M <= 128 4.8-5.1 -> 3.1-3.5; 4096 x 14336, M <= 32 13.2-15.0 -> 10.9-12.6.
//   * 32-row tiles, one per CU at most (G workgroups; 16 columns per workgroup when that still fits): always up to 40 stages (K <= 5120); up to 64 stages when they fill
//     3/4 of the chip (N = 1024 / 2048 against K = 8192 on 64 / 128 workgroups: 7-20 % behind the split-K plans); up to 128 stages for one m-tile or a weight of N >= 4096
//     (2048 x 14336, M = 64: a tie); up to 256 stages (K = 32768) for one m-tile.
//   * 64-row tiles where the 32-row ones overflow the chip: 17 ... 128 stages (4096 x 8192, M = 96 / 128: 15.6 / 14.8 -> 12.0 / 12.5 us; 8192 x 4096, M = 64: 11.3 -> 9.3;
//     K <= 2048 ties, K = 28672 loses 13 %).
inline int os8_plan(int64_t M, int64_t N, int64_t K, int64_t cus) {
  const int64_t T32 = mx_tiles<MXV_OS32>(M, N), T16 = mx_tiles<MXV_OS16>(M, N), T64 = mx_tiles<MXV_OS64>(M, N), KT = cdiv(K, 128);
  if (M <= 16) {   // the decode form with 32 / 48 columns per workgroup
    if (const int v = os16_wide_plan(8, N, K, cus)) return v;
  }
  if (T32 <= cus) {
    const int v = T16 <= cus ? MXV_OS16 : MXV_OS32;
    const int64_t G = T16 <= cus ? T16 : T32;
    // decode form (16x16 tiles on the 16x16x128 MFMA) where those fit one per CU, up to 64 stages (N = K = 4096, M <= 16: 4.85-4.98 -> 3.65-3.82 us; K = 14336: +2 ... 4 %)
    const bool d16 = mx_tiles<MXV_D16>(M, N) <= cus;
    if (KT <= 40) return d16 ? MXV_D16 : v;
    if (4 * G < 3 * cus) return 0;
    if (KT <= 64) return d16 ? MXV_D16 : v;
    if (KT <= 128) return (M <= 32 || N >= 4096) ? v : 0;
    return (KT <= 256 && M <= 32) ? v : 0;
  }
  return (T64 <= cus && KT > 16 && KT <= 128) ? MXV_OS64 : 0;
}

// ---- grouped MXFP4 GEMM (gemm_mx_grouped.hip.h): one launch over E experts ----------------------------------------------------------------------------------------
// Forms: 590 = 32x32 tiles of the wave-owned kernel, 591 = 32x16, 592 = 64x32 (one shot while a tile's K extent fits the LDS, wave-owned rings beyond), 593 = the 64x64
// ring kernel with row-major scale fetch.  Measured on the decode and prefill shapes of Qwen3-30B-A3B and Mixtral-8x7B (profiles/calib_grouped_r7.txt): the per-workgroup
// cost of a grouped tile (the offsets' round trip before the first weight request) favours the fewest, largest tiles -- 593 is fastest everywhere except a short K
// (Qwen3 down, K = 768, 4 rows per expert: 37.6 us against 41.0), where the wave-owned kernel's single round trip wins; 591 and 592 never lead.  So: mean rows per group
// M / E <= 32 and K <= 1024 -> 590, otherwise 593.  N and the CU count are arguments so that a rule re-taken from more measurements can use them.
inline int grouped_plan(int64_t M, int64_t N, int64_t K, int64_t E, int cus) {
  (void)N; (void)cus;
  return (M <= 32 * E && K <= 1024) ? 590 : 593;
}
// workgroups of form v of format F (gemm_mx_grouped.hip.h: the tile table and the grid formula)
inline int64_t grouped_grid(const GroupedFormat& F, int v, int64_t M, int64_t N, int64_t E) {
  return grouped_workgroups(M, N, E, F.tile[v - F.form0].tm, F.tile[v - F.form0].tn);
}
// form F.form0 + I (a wave-owned form) of an MX format; AFMT 1: e5m2 A (grouped_matmul_mxf8_bf16_tn)
template <const GroupedFormat& F, int I, int AFMT = 0>
int launch_grouped_os(GroupedParams q, hipStream_t s) {
  constexpr int TM = F.tile[I].tm, TN = F.tile[I].tn, EBITS = F.ebits;
  q.tiles_m = 1;
  q.tiles_n = (int)cdiv(q.N, TN);
  launch_os_by_stages<true, TN, EBITS, TM, AFMT, true>(cdiv((int64_t)q.K * EBITS / 8, 128), dim3((int)grouped_workgroups(q.M, q.N, q.E, TM, TN)), q, s);
  return check_launch("gemm_mx_os_kernel (grouped)");
}
// form F.form0 + 3 (the ring form) of an MX format
template <const GroupedFormat& F, class C>
int launch_grouped_ring(GroupedParams q, hipStream_t s) {
  static_assert(C::BM == F.tile[3].tm && C::BN == F.tile[3].tn && C::EBITS == F.ebits, "the ring configuration is the format's fourth form");
  q.tiles_m = 1;
  q.tiles_n = (int)cdiv(q.N, C::BN);
  hipLaunchKernelGGL((gemm_mx_grouped_ring_kernel<C>), dim3((int)grouped_workgroups(q.M, q.N, q.E, C::BM, C::BN)), dim3(C::THREADS), 0, s, q);
  return check_launch("gemm_mx_grouped_ring_kernel");
}
// form v of an MX format: C = its ring configuration
template <const GroupedFormat& F, class C, int AFMT = 0>
int launch_grouped_mx(int v, const GroupedParams& q, hipStream_t s) {
  if (v == F.form0) return launch_grouped_os<F, 0, AFMT>(q, s);
  if (v == F.form0 + 1) return launch_grouped_os<F, 1, AFMT>(q, s);
  if (v == F.form0 + 2) return launch_grouped_os<F, 2, AFMT>(q, s);
  return launch_grouped_ring<F, C>(q, s);
}

// ---- grouped MXFP8 GEMM: the same two tile bodies on 8-bit elements (a stage is 128 elements, so a row has twice the stages of an MXFP4 row of the same K) ----------
// Forms: 594 = 32x32 tiles of the wave-owned kernel, 595 = 32x16, 596 = 64x32 (one shot while a tile's K extent fits the LDS, wave-owned rings beyond), 597 = the 64x64
// ring kernel with row-major scale fetch (matmul_mxf8_bf16_tn's ring tiles).
// Measured on the decode and prefill shapes of Qwen3-30B-A3B and Mixtral-8x7B (profiles/calib_grouped_mxf8_r7.txt; these are not the MXFP4 thresholds): 597 is fastest
// everywhere but one case, a short K included (Qwen3 down, K = 768, 4 rows per expert: 53.1 us against 66.4 for 594 -- where MXFP4's 590 won); 595 and 596 never lead.
// The exception is a long K at few rows per expert (Mixtral down, K = 14336, 16 rows per expert: 594 takes 107.8 / 112.6 us uniform / skewed against 106.9 / 145.8 for
// 597), while the same rows at K = 4096 stay with 597 (Mixtral gate/up: 224.6 / 240.5 against 275.9 / 295.9).  So: mean rows per group M / E <= 32 and K >= 8192 -> 594,
// otherwise 597.  N and the CU count are arguments so that a rule re-taken from more measurements can use them.
inline int grouped8_plan(int64_t M, int64_t N, int64_t K, int64_t E, int cus) {
  (void)N; (void)cus;
  return (M <= 32 * E && K >= 8192) ? 594 : 597;
}

// ---- grouped W4A8 GEMM (gemm_mx_os_w4a8.hip.h): MXFP8 tokens against MXFP4 expert weights ------------------------------------------------------------------------------
// Forms: 602 = 32x32 tiles of the mixed-width wave-owned kernel, 603 = 32x16, 604 = 64x32 (one shot while a tile's K extent fits the LDS, wave-owned rings beyond).  There
// is no 64x64 ring form: GemmCtx, which every product GEMM shares, has one row width for both operands -- so prefill-sized groups run on the decode tiles.
// Measured on the decode and prefill shapes of Qwen3-30B-A3B, Mixtral-8x7B and gpt-oss-20b / 120b and on a sweep of 16 ... 128 rows per expert at K = 768 ... 2944
// (profiles/calib_grouped_w4a8.txt): 603 never leads.  Up to K = 1536 -- the 32-row tile's stages of a wave fit three slots, two workgroups share a CU -- 602 leads
// at every row count (K = 1536, 128 rows per expert: 358.0 us against 449.1 for 604; K = 768, Qwen3 down prefill: 369.2 against 594.6).  From K = 2048 on 604 leads as
// soon as the groups fill its 64 rows halfway (K = 2048: 32 rows 224.5 against 249.1, 128 rows 574.0 against 728.4; Mixtral gate/up prefill 4072.6 against 6415.6):
// it fetches each weight row once for two m-tiles; at 16 rows and below 602 leads at every K (K = 2944: 202.3 against 237.2; Mixtral down decode, K = 14336: 60.8
// against 66.6).  So: mean rows per group M / E >= 32 and K > 1536 -> 604, otherwise 602.  N and the CU count are arguments so that a rule re-taken from more
// measurements can use them.
inline int grouped_w4a8_plan(int64_t M, int64_t N, int64_t K, int64_t E, int cus) {
  (void)N; (void)cus;
  return (M >= 32 * E && K > 1536) ? 604 : 602;
}
// form GRP_MXF8_MXF4.form0 + I: the one-shot ladder up to 4 SMAX stages, wave-owned rings of SMAX slots beyond.  The smaller stage moves SMAX: 6 slots per wave for
// the 32-row tiles (one shot up to K = 3072), 3 for the 64-row tile (K = 1536)
template <int I>
int launch_grouped_w4a8_os(GroupedParams q, hipStream_t s) {
  constexpr const GroupedFormat& F = GRP_MXF8_MXF4;
  constexpr int TM = F.tile[I].tm, TN = F.tile[I].tn, SMAX = os_w4a8_smax(TM);
  q.tiles_m = 1;
  q.tiles_n = (int)cdiv(q.N, TN);
  const int64_t KT = q.K / 128;
  const dim3 grid((int)grouped_workgroups(q.M, q.N, q.E, TM, TN)), block(256);
  if (KT <= 4) hipLaunchKernelGGL((gemm_mx_os_w4a8_kernel<OsW4A8Cfg<1, TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 8) hipLaunchKernelGGL((gemm_mx_os_w4a8_kernel<OsW4A8Cfg<2, TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 12) hipLaunchKernelGGL((gemm_mx_os_w4a8_kernel<OsW4A8Cfg<3, TN, TM>, false>), grid, block, 0, s, q);
  else if (SMAX > 4 && KT <= 16) hipLaunchKernelGGL((gemm_mx_os_w4a8_kernel<OsW4A8Cfg<(SMAX > 4 ? 4 : SMAX), TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 4 * SMAX) hipLaunchKernelGGL((gemm_mx_os_w4a8_kernel<OsW4A8Cfg<SMAX, TN, TM>, false>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((gemm_mx_os_w4a8_kernel<OsW4A8Cfg<SMAX, TN, TM>, true>), grid, block, 0, s, q);   // wave-owned rings of SMAX slots
  return check_launch("gemm_mx_os_w4a8_kernel");
}
// form v of the W4A8 op; its kernels ride in the persistent NVFP4 kernel's unit, the shortest of the parallel build
int launch_grouped_w4a8(int v, const GroupedParams& q, hipStream_t s)
#if QAMD_DEF(8)
{
  constexpr const GroupedFormat& F = GRP_MXF8_MXF4;
  static_assert(F.nforms == 3 && F.ebits == 8 && F.ebits_b == 4, "the three wave-owned forms of the mixed-width kernel");
  if (v == F.form0) return launch_grouped_w4a8_os<0>(q, s);
  if (v == F.form0 + 1) return launch_grouped_w4a8_os<1>(q, s);
  if (v == F.form0 + 2) return launch_grouped_w4a8_os<2>(q, s);
  return fail(QAMD_ERR_INVALID, "%s: unknown form %d", F.name, v);
}
#else
;
#endif

// ---- grouped W4A16 GEMM (gemm_mx_os_w4a16.hip.h): bf16 tokens against MXFP4 expert weights ---------------------------------------------------------------------------
// Forms: 606 = 32x32 tiles of the bf16-token wave-owned kernel, 607 = 32x16, 608 = 64x32 (one shot while a tile's K extent fits the LDS, wave-owned rings beyond).  No
// 64x64 ring form, as for W4A8.
// Measured on the decode and prefill shapes of Qwen3-30B-A3B, Mixtral-8x7B and gpt-oss-20b / 120b and on a sweep of 16 ... 128 rows per expert at K = 512 ... 2944
// (profiles/calib_grouped_w4a16.txt, taken under the provisional rule -- W4A8's structure with the K threshold at 1024): 607 never leads.  At 16 rows per expert and
// below 606 leads at every K (K = 768: 139.6 us against 154.8 for 608; K = 2944: 248.6 against 290.0).  From 32 rows per expert on 608 leads at every K from 768
// (K = 768: 32 rows 168.8 against 199.5, 128 rows 394.9 against 556.0 -- the provisional rule's miss, Qwen3 down prefill 698.4 against 1020.3; K = 2944, 128 rows:
// 831.4 against 1078.3): it converts each weight fragment once for two m-tiles.  At K = 512 the two are level (32 rows 75.0 for 606 against 82.7; 48 rows 96.5
// against 91.0; 128 rows 203.7 against 189.1): left with 606.  So: mean rows per group M / E >= 32 and K > 512 -> 608, otherwise 606.  N and the CU count are
// arguments so that a rule re-taken from more measurements can use them.
inline int grouped_w4a16_plan(int64_t M, int64_t N, int64_t K, int64_t E, int cus) {
  (void)N; (void)cus;
  return (M >= 32 * E && K > 512) ? 608 : 606;
}
// form GRP_BF16_MXF4.form0 + I: the one-shot ladder up to 4 SMAX stages, wave-owned rings of SMAX slots beyond -- 3 slots per wave for the 32-row tiles (one shot up to
// K = 1536), 2 for the 64-row tile (K = 1024); GATHER: A rows through q.src_row
template <int I, bool GATHER>
int launch_grouped_w4a16_os(W4A16Params q, hipStream_t s) {
  constexpr const GroupedFormat& F = GRP_BF16_MXF4;
  constexpr int TM = F.tile[I].tm, TN = F.tile[I].tn, SMAX = os_w4a16_smax(TM);
  static_assert(SMAX == 2 || SMAX == 3, "the ladder below");
  q.tiles_m = 1;
  q.tiles_n = (int)cdiv(q.N, TN);
  const int64_t KT = q.K / 128;
  const dim3 grid((int)grouped_workgroups(q.M, q.N, q.E, TM, TN)), block(256);
  if (KT <= 4) hipLaunchKernelGGL((gemm_mx_os_w4a16_kernel<OsW4A16Cfg<1, TN, TM>, false, GATHER>), grid, block, 0, s, q);
  else if (KT <= 8) hipLaunchKernelGGL((gemm_mx_os_w4a16_kernel<OsW4A16Cfg<2, TN, TM>, false, GATHER>), grid, block, 0, s, q);
  else if (KT <= 4 * SMAX) hipLaunchKernelGGL((gemm_mx_os_w4a16_kernel<OsW4A16Cfg<SMAX, TN, TM>, false, GATHER>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((gemm_mx_os_w4a16_kernel<OsW4A16Cfg<SMAX, TN, TM>, true, GATHER>), grid, block, 0, s, q);   // wave-owned rings of SMAX slots
  return check_launch("gemm_mx_os_w4a16_kernel");
}
// form v of the W4A16 op; its kernels ride in the persistent NVFP4 kernel's unit beside W4A8's, still the shortest of the parallel build
int launch_grouped_w4a16(int v, const W4A16Params& q, hipStream_t s)
#if QAMD_DEF(8)
{
  constexpr const GroupedFormat& F = GRP_BF16_MXF4;
  static_assert(F.nforms == 3 && F.ebits == 16 && F.ebits_b == 4, "the three wave-owned forms of the bf16-token kernel");
  const bool gather = q.src_row != nullptr;
  if (v == F.form0) return gather ? launch_grouped_w4a16_os<0, true>(q, s) : launch_grouped_w4a16_os<0, false>(q, s);
  if (v == F.form0 + 1) return gather ? launch_grouped_w4a16_os<1, true>(q, s) : launch_grouped_w4a16_os<1, false>(q, s);
  if (v == F.form0 + 2) return gather ? launch_grouped_w4a16_os<2, true>(q, s) : launch_grouped_w4a16_os<2, false>(q, s);
  return fail(QAMD_ERR_INVALID, "%s: unknown form %d", F.name, v);
}
#else
;
#endif

// ---- grouped W4A6 GEMM (gemm_mx_os_w4a6.hip.h): MXFP6 (e2m3) tokens against MXFP4 expert weights --------------------------------------------------------------------
// Forms: 610 = 32x32 tiles of the 6-bit-token wave-owned kernel, 611 = 32x16, 612 = 64x32 (one shot while a tile's K extent fits the LDS, wave-owned rings beyond).  No
// 64x64 ring form, as for W4A8.
// Started from W4A8's rule with its K threshold rescaled by the stage size -- which leaves it at 1536: there 604 takes over where the 32-row tile's stages of a wave stop
// fitting three slots (3 x 6.5 KiB x 4 waves = 78 KiB, two workgroups per CU); the 5.5 KiB stage keeps three slots up to the same K and a fourth would not let two
// workgroups share a CU (4 x 5.5 x 4 = 88 KiB > 80).  Measured on the decode and prefill shapes of Qwen3-30B-A3B, Mixtral-8x7B and gpt-oss-20b / 120b and on a sweep of
// 16 ... 128 rows per expert at K = 768 ... 3712 (profiles/calib_grouped_w4a6.txt, taken under that provisional rule): 611 never leads.  From K = 2048 on 612 leads from
// 32 rows per expert (K = 2048: 32 rows 199.9 us against 246.8 for 610, 128 rows 517.6 against 710.4; K = 3712, 128 rows: 801.5 against 1110.2), 610 at 16 rows at every K
// (K = 3712: 256.9 against 259.3; K = 768: 52.6 against 72.5).  At K = 1536 -- the 64-row tile runs three slots per wave, 102 KiB, one workgroup per CU -- 610 leads at
// every row count (128 rows: 342.9 against 433.5).  Up to K = 1024 the 64-row tile runs at most two slots (68 KiB, two workgroups per CU) and 612 leads from 48 rows on
// (K = 768: 48 rows 86.7 against 94.9, 128 rows 181.0 against 200.6; K = 1024: 48 rows 91.4 against 105.1; Qwen3 down prefill, K = 768, 256 rows: 313.7 against 358.5 --
// the provisional rule's one miss), while at 32 rows 610 leads (K = 768: 73.6 against 79.5).  So: mean rows per group M / E >= 32 and K > 1536, or M / E >= 48 and
// K <= 1024 -> 612; otherwise 610.  N and the CU count are arguments so that a rule re-taken from more measurements can use them.
inline int grouped_w4a6_plan(int64_t M, int64_t N, int64_t K, int64_t E, int cus) {
  (void)N; (void)cus;
  return ((M >= 32 * E && K > 1536) || (M >= 48 * E && K <= 1024)) ? 612 : 610;
}
// form GRP_MXF6_MXF4.form0 + I: the one-shot ladder up to 4 SMAX stages, wave-owned rings of SMAX slots beyond -- 7 slots per wave for the 32-row tiles (one shot up to
// K = 3584), 4 for the 64-row tile (K = 2048)
template <int I>
int launch_grouped_w4a6_os(GroupedParams q, hipStream_t s) {
  constexpr const GroupedFormat& F = GRP_MXF6_MXF4;
  constexpr int TM = F.tile[I].tm, TN = F.tile[I].tn, SMAX = os_w4a6_smax(TM);
  static_assert(SMAX >= 4, "the ladder below");
  q.tiles_m = 1;
  q.tiles_n = (int)cdiv(q.N, TN);
  const int64_t KT = q.K / 128;
  const dim3 grid((int)grouped_workgroups(q.M, q.N, q.E, TM, TN)), block(256);
  if (KT <= 4) hipLaunchKernelGGL((gemm_mx_os_w4a6_kernel<OsW4A6Cfg<1, TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 8) hipLaunchKernelGGL((gemm_mx_os_w4a6_kernel<OsW4A6Cfg<2, TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 12) hipLaunchKernelGGL((gemm_mx_os_w4a6_kernel<OsW4A6Cfg<3, TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 16) hipLaunchKernelGGL((gemm_mx_os_w4a6_kernel<OsW4A6Cfg<4, TN, TM>, false>), grid, block, 0, s, q);
  else if (KT <= 4 * SMAX) hipLaunchKernelGGL((gemm_mx_os_w4a6_kernel<OsW4A6Cfg<SMAX, TN, TM>, false>), grid, block, 0, s, q);
  else hipLaunchKernelGGL((gemm_mx_os_w4a6_kernel<OsW4A6Cfg<SMAX, TN, TM>, true>), grid, block, 0, s, q);   // wave-owned rings of SMAX slots
  return check_launch("gemm_mx_os_w4a6_kernel");
}
// form v of the W4A6 op; its kernels ride in the persistent NVFP4 kernel's unit beside W4A8's and W4A16's
int launch_grouped_w4a6(int v, const GroupedParams& q, hipStream_t s)
#if QAMD_DEF(8)
{
  constexpr const GroupedFormat& F = GRP_MXF6_MXF4;
  static_assert(F.nforms == 3 && F.ebits == 6 && F.ebits_b == 4, "the three wave-owned forms of the 6-bit-token kernel");
  if (v == F.form0) return launch_grouped_w4a6_os<0>(q, s);
  if (v == F.form0 + 1) return launch_grouped_w4a6_os<1>(q, s);
  if (v == F.form0 + 2) return launch_grouped_w4a6_os<2>(q, s);
  return fail(QAMD_ERR_INVALID, "%s: unknown form %d", F.name, v);
}
#else
;
#endif

// ---- what the grouped entries share: the argument checks, the choice of a form and the parameter fill ----------------------------------------------------------
// the grouped ops' argument checks, F the format (gemm_mx_grouped.hip.h): every argument is checked before any HIP call; the grid bound covers every form
inline int grouped_check(const GroupedFormat& F, const char* name, const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                         const int32_t* offs, const void* D, int64_t M, int64_t N, int64_t K, int64_t E) {
  if (!A || !B || !A_sf || !B_sf || !alpha || !offs || !D) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (E < 1 || E > GRP_MAX_E) return fail(QAMD_ERR_INVALID, "%s: E must be in [1, %d] (got %lld)", name, GRP_MAX_E, (long long)E);
  if (n_alpha != 1 && n_alpha != E) return fail(QAMD_ERR_INVALID, "%s: alpha must have 1 or E = %lld elements (got %lld)", name, (long long)E, (long long)n_alpha);
  if (M < 0 || N <= 0) return fail(QAMD_ERR_INVALID, "%s: M must be >= 0 and N positive (got M=%lld N=%lld)", name, (long long)M, (long long)N);
  if (K < 128 || K % 128) return fail(QAMD_ERR_INVALID, "%s: K must be a positive multiple of 128 (got %lld)", name, (long long)K);
  if (N % 8) return fail(QAMD_ERR_INVALID, "%s: N must be a multiple of 8 (got %lld)", name, (long long)N);
  const char* rowa = F.row_bytes(K) == 2 * K ? "2K" : F.row_bytes(K) == K ? "K" : F.ebits == 6 ? "3K/4" : "K/2";
  const char* rowb = F.row_bytes_b(K) == K ? "K" : "K/2";
  const int64_t rows_2g = ((1ll << 31) - 1) / F.row_bytes(K) + 1;   // rows of a row's bytes that reach 2 GiB (no product that can overflow)
  const int64_t rows_2g_b = ((1ll << 31) - 1) / F.row_bytes_b(K) + 1;
  if (N >= rows_2g_b) return fail(QAMD_ERR_INVALID, "%s: one expert's weight (N * %s bytes, N=%lld K=%lld) must stay below 2 GiB", name, rowb, (long long)N, (long long)K);
  if (M >= rows_2g) return fail(QAMD_ERR_INVALID, "%s: the token matrix (M * %s bytes, M=%lld K=%lld) must stay below 2 GiB", name, rowa, (long long)M, (long long)K);
  if (M * N >= (1ll << 40)) return fail(QAMD_ERR_INVALID, "%s: an output of 2^40 elements is not supported", name);
  for (int v = F.form0; F.has(v); ++v)
    if (grouped_grid(F, v, M, N, E) >= (1ll << 24)) return fail(QAMD_ERR_INVALID, "%s: %lld x %lld over %lld experts needs more than 2^24 workgroups", name, (long long)M, (long long)N, (long long)E);
  return QAMD_OK;
}
// the form of a launch: the lab's gemm_variant option forces one of the format's four, otherwise the op's plan rule on this chip
using GroupedPlan = int (*)(int64_t M, int64_t N, int64_t K, int64_t E, int cus);
inline int grouped_form(const GroupedFormat& F, GroupedPlan plan, int64_t M, int64_t N, int64_t K, int64_t E) {
  const int forced = opt_gemm_variant();
  return F.has(forced) ? forced : plan(M, N, K, E, chip_cus());
}
// the fields of GroupedParams the dense MX kernels' base brings along: the lab's options, no split-K, no raster
inline void grouped_mx_defaults(GroupedParams& q) {
  q.pp_shift = opt_pp_shift(); q.pp_flags = opt_pp_flags(); q.dbg = opt_dbg();
  q.ws = nullptr; q.ctr = nullptr; q.tag = 0; q.raster_magic = 0; q.sk_tiles = 0;
}
// the fields GroupedParams and NvGroupedParams share (different bases, the same names)
template <class P>
void grouped_fill(P& q, const GroupedFormat& F, const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                  const int32_t* offs, void* D, int64_t M, int64_t N, int64_t K, int64_t E) {
  const int64_t rowbytes = F.row_bytes(K), KB = K / F.sgroup;
  q.A = (const uint8_t*)A; q.B = (const uint8_t*)B; q.SFA = (const uint8_t*)A_sf; q.SFB = (const uint8_t*)B_sf;
  q.alpha = alpha; q.D = (uint16_t*)D; q.M = (int)M; q.N = (int)N; q.K = (int)K; q.ldd = (int)N;
  q.a_bytes = (uint32_t)(M * rowbytes); q.b_bytes = (uint32_t)(N * F.row_bytes_b(K));     // b_bytes / sfb_bytes: ONE expert's (the kernel rebases per expert)
  q.sfa_bytes = (uint32_t)(M * KB); q.sfb_bytes = (uint32_t)(N * KB);
  q.offs = offs; q.E = (int)E; q.n_alpha = (int)n_alpha; q.splits = 1;
}

// [r4] stream-K form of the two persistent kernels (lab variant 89): one workgroup per CU; p.ws / p.ctr / p.tag / p.sk_tiles set by mx_launch
#if QAMD_BENCH
template <class C>
int launch_gemm_deepp_sk(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, C::BM);
  p.tiles_n = (int)cdiv(p.N, C::BN);
  p.raster_magic = raster_magic(p.tiles_n);
  p.splits = 1;
  const int grid = chip_cus();
  if constexpr (C::EBITS == 4) hipLaunchKernelGGL((labk::gemm_mx_deepp_kernel<C, false, 17, 0, true>), dim3(grid), dim3(C::THREADS), 0, s, p);
  else hipLaunchKernelGGL((labk::gemm_mx_deepp8_kernel<C, 17, false, 0, true>), dim3(grid), dim3(C::THREADS), 0, s, p);
  return check_launch("gemm_mx_deepp_kernel (stream-K)");
}
#endif

template <class C, bool NN = false, int NNABL = 0>
int launch_gemm_deepp8(GemmParams p, hipStream_t s) {   // the fp8 twin (gemm_mx_deepp8), write-through output stores; NN: A is (K, M)
  p.tiles_m = (int)cdiv(p.M, C::BM);
  p.tiles_n = (int)cdiv(p.N, C::BN);
  p.raster_magic = raster_magic(p.tiles_n);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  const int grid = deepp_grid(p.tiles_m * p.tiles_n);
#if QAMD_BENCH
  if constexpr (NNABL != 0) {   // the NN-operand ablations: the lab copy of the kernel
    hipLaunchKernelGGL((labk::gemm_mx_deepp8_kernel<C, 17, NN, NNABL>), dim3(grid), dim3(C::THREADS), 0, s, p);
    return check_launch("labk::gemm_mx_deepp8_kernel");
  }
#else
  static_assert(NNABL == 0, "ablations: lab build only");
#endif
  if (grid == p.tiles_m * p.tiles_n) hipLaunchKernelGGL((gemm_mx_deepp8_kernel<C, 17, NN, true>), dim3(grid), dim3(C::THREADS), 0, s, p);   // [r6] one tile per workgroup
  else hipLaunchKernelGGL((gemm_mx_deepp8_kernel<C, 17, NN>), dim3(grid), dim3(C::THREADS), 0, s, p);
  return check_launch("gemm_mx_deepp8_kernel");
}

// Heterogeneous launch (gemm_mx_hetero_kernel): the persistent 256x256 kernel over the full rounds of `cus` tiles + the residual
// tiles as 128x128 quarter tiles on extra workgroups of the SAME grid, dispatched CU by CU as the persistent workgroups retire.
template <class CB, class CT, int ST_AUX>
int launch_gemm_hetero(GemmParams p, hipStream_t s) {
  p.tiles_m = (int)cdiv(p.M, CB::BM);
  p.tiles_n = (int)cdiv(p.N, CB::BN);
  p.raster_magic = raster_magic(p.tiles_n);
  p.ws = nullptr; p.splits = 1; p.ctr = nullptr; p.tag = 0;
  const int T = p.tiles_m * p.tiles_n;
  const int forced = opt_deepp_grid();
  const int g_big = std::min(forced > 0 ? forced : chip_cus(), T);
  const int t_main = T / g_big * g_big;
  const int nsmall = 4 * (T - t_main);
  if (nsmall == 0) {   // a whole number of rounds: nothing residual, the plain persistent kernel
    if constexpr (CB::EBITS == 4) return launch_gemm_deepp<CB, false, ST_AUX>(p, s);
    else return launch_gemm_deepp8<CB>(p, s);
  }
  if constexpr (CB::EBITS == 4) {   // [r6] odd number of K stages: the persistent workgroups run without the empty stage
    if (const int64_t kt = cdiv((int64_t)p.K, 256); (kt & 1) && kt >= 3) {
      hipLaunchKernelGGL((gemm_mx_hetero_kernel<CB, CT, ST_AUX, true>), dim3(g_big + nsmall), dim3(256), 0, s, p, g_big, t_main);
      return check_launch("gemm_mx_hetero_kernel (odd stage count)");
    }
  }
  hipLaunchKernelGGL((gemm_mx_hetero_kernel<CB, CT, ST_AUX>), dim3(g_big + nsmall), dim3(256), 0, s, p, g_big, t_main);
  return check_launch("gemm_mx_hetero_kernel");
}

// Persistent launch or heterogeneous launch for T tiles of 256x256?  Cost in units of one full-chip round of `cus` tiles, fitted to the
// steady-state A/B of 18 shapes, K = 1024 .. 14336 (tests/native/qamd_check heterobench, profiles/native_r3_heterobench.log):
//   balanced rounds   R = ceil(T / cus) rounds at occupancy o = T / (R cus).  The kernels run at the socket power limit, so a round that
//                     leaves CUs idle is cheaper -- but never cheaper than the clock ceiling allows: f(o) = max(0.45 + 0.55 o, 0.78)
//                     (measured: 272 / 320 / 384 / 448 / 576 tiles = 1.56 / 1.62 / 1.77 / 1.90 / 2.62 rounds)
//   heterogeneous     the full rounds + waves of 128x128 quarter tiles: 0.05 once, then 0.25 + 0.13 x fill per wave of `cus` quarter tiles
//                     (a quarter tile walks K at ~0.6 us per stage against 1.79 us for the 256x256 tile, plus its own prologue /
//                     epilogue; measured: 272 / 288 / 320 / 384 / 448 / 576 tiles = 1.30 / 1.32 / 1.43 / 1.87 / 2.25 / 2.43 rounds)
// 4096 x 5120 x 4096: 52.3 us balanced, 49.9 us as two launches (round 2), 46.8 us heterogeneous; 3072 x 6144: 51.5 / 47.4 / 43.3.
inline bool hetero_wins(int64_t T, int cus) {
  const int64_t r = T / cus, rem = T % cus;
  if (r < 1 || rem == 0) return false;
  const int64_t R = r + 1;
  const double a = (double)R * std::max(0.45 + 0.55 * (double)T / (double)(R * cus), 0.78);
  const int64_t nsmall = 4 * rem, waves = nsmall / cus;
  const double last = (double)(nsmall % cus) / (double)cus;
  const double b = (double)r + 0.05 + 0.38 * (double)waves + (last > 0 ? 0.25 + 0.13 * last : 0.0);
  return b < a;
}

// Tile/schedule variants (0 = auto; the lab library can force one through the "gemm_variant" option).  The PRODUCT forms -- what the auto rules below can pick -- are the rows of
// MX_FORMS (gemm_mx_forms.hip.h: number, family, tile, wave grid, ring depth, ops); launch_mx_form launches one from its row.  Every other number is LAB only
// (dispatch_lab_variant; 44 ... 49 and 89 also in mx_launch):
//   [r4]  89  = 90 as a stream-K walk (tiles of a part-filled round cut along K, fp32 parts parked in caller scratch).  Correct and
//     deterministic (tests/test_gpu_round4.py) and NOT adopted: a cut tile moves 256 KiB of fp32 sums through memory twice, and a stream over G + T % G
//     tiles cuts ~G - gcd tiles -- 128 ... 255 parked tiles = 64 ... 128 MB per launch at ~3.7 TB/s: +18 us at 384 tiles, +34 us at 320 (MXFP4,
//     K = 4096: 74.8 / 86.1 us against 57.0 balanced / 48.2 heterogeneous); break-even only beyond K ~ 14336, where the heterogeneous launch still
//     matches or beats it (MXFP8 3072 x 8192 x 28672: 612 us stream-K, 601 heterogeneous, 666 balanced).  profiles/ab_mxsk_r4c.txt
//   30 = the per-tile deep schedule of round 1 (fp4, 256x256, 4 waves of 128x128, LDS-DMA)      99 = 98 with a 3-deep ring for the residual tiles
//   1  256x256 ping-pong     5  256x256 lockstep     6..9  queue schedule (256x256, 128x128, 256x128, 128x256)
//   20 / 224 / 225 / 26  simple schedule (256x256, 128x128, 256x128, 128x256)      170..173  the round-1 ring schedule on the tiles of 70..73
//   40  regstage (the tiling of 30, copy through registers)      44..49  other shapes of the skinny split-K kernel (waves, segments per trip, chunk mapping)
//   31..36, 41..43, 50..56  ablations / traces / clock probes of those (bench only)      2 / 3 / 4  128x128 (small M or N) / 256x128 / 128x256 lockstep
// bench-only ablations of the 8-wave 256x256 MXFP4 schedules: 100 + b ping-pong, 200 + b lockstep, 300 + b queue, b = OR
// of ABL_* bits.  Returns -1 for any other variant.
#if QAMD_BENCH
#if QAMD_DEF(6)
int dispatch_ablation_mx4(int v, const GemmParams& p, hipStream_t s) {
  switch (v) {
#define QAMD_ABL(b) \
    case 100 + b: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, b>, 1>(p, s); \
    case 200 + b: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, b>, 0>(p, s); \
    case 300 + b: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, b>, 2>(p, s);
    QAMD_ABL(1) QAMD_ABL(2) QAMD_ABL(3) QAMD_ABL(4) QAMD_ABL(8) QAMD_ABL(9) QAMD_ABL(10) QAMD_ABL(11) QAMD_ABL(16) QAMD_ABL(17) QAMD_ABL(18) QAMD_ABL(41) QAMD_ABL(40) QAMD_ABL(42)
#undef QAMD_ABL
  }
  return -1;
}
#else
int dispatch_ablation_mx4(int v, const GemmParams& p, hipStream_t s);
#endif
#endif   // QAMD_BENCH

int launch_mx_skinny(bool rm, const GemmParams& p, hipStream_t s);   // the LDS-free split-K kernel (rm: row-major scales) is small and stays in unit 1, with the entries
// Row I of MX_FORMS for the op (EBITS, AFMT: 1 = e5m2 A, RM: row-major scales = matmul_ada_mxf4_bf16_tn): the row holds what picks the kernel configuration
template <int I, int EBITS, int AFMT, bool RM>
int launch_mx_row(const GemmParams& p, hipStream_t s) {
  constexpr MxFormRow F = MX_FORMS[I];
  static_assert(F.product && (F.ops & mx_op(EBITS, AFMT, RM)) != 0, "the form has no kernel for this op");
  constexpr bool SPLIT = EBITS == 8;   // GemmCfg F8SPLIT: the fp8 kernels' split register layout
  if constexpr (F.family == MXF_PIPELINED || F.family == MXF_RING || F.family == MXF_PERSISTENT) {
    using C = GemmCfg<F.tm, F.tn, F.wm, F.wn, EBITS, SPLIT, 0, F.depth, AFMT>;
    // pipelined schedule on an LDS ring (gemm_mx_ringp; row-major scales: its scale fetch of matmul_ada_mxf4_bf16_tn): NSTAGE-deep ring, NSTAGE - 1 stages in flight, the
    // next stage's fragments are read during this stage's MFMAs.  2-deep (24 ... 29): the LDS footprint of the round-1 "simple" schedule, two workgroups per CU: -3 .. -13 %
    // against the simple schedule on every mid-size shape measured (profiles/native_r2_midtile2.log).
    // [r3] 58: 256x128 on FOUR waves of 128x64, 3-deep ring, one workgroup per CU: 0.75 KiB of LDS fragment reads per MFMA against 1 KiB for the 64x64 wave
    // tiles of 24 / 25 -- half-chip outputs with a long K (2048 x 4096 x 8192: 36.9 -> 35.4 us, x 14336: 60.6 -> 57.1; profiles/native_r3_halftile.log)
    if constexpr (F.family != MXF_PERSISTENT) return launch_gemm<C, RM ? 10 : 9>(p, s);
    // persistent deep schedule; output stores write through (sc0 sc1): nothing dirty is left for the end-of-kernel L2
    // write-back (4096^3: 34.6 -> 33.4 .. 34.4 us, never slower; profiles/native_r2_store_policy.log)
    // The one-tile form of 90: the product's is the 16x16x128 one (kDeeppOneTile16).  In the LAB library 90 keeps the 32x32x64 form and 191 is the product's: the kernels the
    // tests compare 90 with bit for bit (the 8-wave kernel 87 / 88, the ring and stream-K kernels) all group K by 64 per MFMA, and outside the exact regime of
    // docs/history.md section 3.1 the grouping shows (random bytes with scale bytes 121 ... 129 at 4096^3: 23 of 16.8 M outputs differ in their last bf16 bit).
    else if constexpr (EBITS == 4) return launch_gemm_deepp<C, false, 17, 0, QAMD_BENCH ? 32 : 0>(p, s);
    else return launch_gemm_deepp8<C>(p, s);
  } else if constexpr (F.family == MXF_HETERO) {
    using CB = GemmCfg<F.tm, F.tn, F.wm, F.wn, EBITS, SPLIT, 0, 2, AFMT>;
    using CT = GemmCfg<F.tm / 2, F.tn / 2, F.wm, F.wn, EBITS, SPLIT, 0, F.depth, AFMT>;
    static_assert(CB::BM == kMxForm<MXV_PERSISTENT>.tm && CB::BN == kMxForm<MXV_PERSISTENT>.tn, "the full rounds run the persistent form");
    return launch_gemm_hetero<CB, CT, 17>(p, s);
  } else if constexpr (F.family == MXF_SKINNY) {
    return launch_mx_skinny(RM, p, s);
  } else if constexpr (F.family == MXF_KSPLIT) {
    // [r6] K split inside the workgroup (gemm_mx_ks.hip.h).  Ring depth by the K stage count: a short K pays for a deep ring's prologue
    // (4096^2 weights, M <= 64: 4.16 us 4-deep, 4.47 us 8-deep), a long one needs the stages in flight (8192^2: 9.4 us 4-deep, 7.4 us 6-deep; profiles/calib_ks_r6*.txt)
    static_assert(KsCfg<F.tm, F.tn, F.depth>::TM == F.tm && KsCfg<F.tm, F.tn, F.depth>::TN == F.tn && F.depth == 4, "the K-split configuration is the row's");
    return cdiv(p.K, 256) > 24 ? launch_gemm_ks<F.tm, F.tn, 6>(p, s) : launch_gemm_ks<F.tm, F.tn, F.depth>(p, s);
  } else if constexpr (F.family == MXF_OS) {
    // [r6] tiles on wave-owned K stages (gemm_mx_os.hip.h): one shot up to 16 stages (12 for the 64-row tile: two m-tiles per stage owner), wave-owned rings beyond
    static_assert(OsCfg<1, F.tn, EBITS, F.tm, AFMT>::TM == F.tm && OsCfg<1, F.tn, EBITS, F.tm, AFMT>::TN == F.tn, "the wave-owned configuration is the row's");
    return launch_gemm_os<RM, F.tn, EBITS, F.tm, AFMT>(p, s);
  } else {
    // [r6] decode form: 16 x (16 / 32 / 48 / 56 / 64) tiles on the 16x16x128 MFMA
    static_assert(F.family == MXF_DECODE && Os16Cfg<1, EBITS, AFMT, F.tn>::TM == F.tm && Os16Cfg<1, EBITS, AFMT, F.tn>::TN == F.tn, "the decode configuration is the row's");
    return launch_gemm_os16<EBITS, AFMT, RM, F.tn>(p, s);
  }
}
// The ONE product dispatcher: variant v of MX_FORMS for the op.  A (form, op) pair the row's mask does not list is an error, as is a number without a row (MXFP8 with
// an e5m2 A operand -- qutlass_amd_matmul_mxf8_bf16_{tn,nn}_fmt -- has the forms the auto rules can pick, nothing else).  One flat chain of comparisons: a switch.
template <int I, int EBITS, int AFMT, bool RM>
inline bool try_mx_row(int v, const GemmParams& p, hipStream_t s, int& rc) {
  if constexpr (MX_FORMS[I].product && (MX_FORMS[I].ops & mx_op(EBITS, AFMT, RM)) != 0) {
    if (v == MX_FORMS[I].variant) { rc = launch_mx_row<I, EBITS, AFMT, RM>(p, s); return true; }
  }
  return false;
}
template <int EBITS, int AFMT, bool RM, int... I>
int launch_mx_form(int v, const GemmParams& p, hipStream_t s, const char* name, std::integer_sequence<int, I...>) {
  int rc = 0;
  if ((try_mx_row<I, EBITS, AFMT, RM>(v, p, s, rc) || ...)) return rc;
  if (AFMT == 1) return fail(QAMD_ERR_INVALID, "%s: gemm_variant %d has no e5m2-operand instantiation", name, v);
  return fail(QAMD_ERR_INVALID, "%s: unknown gemm_variant %d", name, v);
}

#if QAMD_BENCH
// the numbers MX_FORMS does not own (blocked scales, e2m1 / e4m3 A)
template <int EBITS>
int dispatch_lab_variant(int v, const GemmParams& p, hipStream_t s, const char* name) {
  constexpr bool SPLIT = EBITS == 8;
  switch (v) {
    case 273: return launch_gemm<GemmCfg<128, 128, 2, 2, EBITS, SPLIT, 128, 3>, 9>(p, s);   // lab: 73 with the next stage's reads packed into the first MFMAs (ABL_READS_FIRST)
    case 272: return launch_gemm<GemmCfg<64, 128, 2, 2, EBITS, SPLIT, 128, 3>, 9>(p, s);
    case 270: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 128, 3>, 9>(p, s);
    case 224 + 1000: return launch_gemm<GemmCfg<128, 128, 2, 2, EBITS, SPLIT, 128, 2>, 9>(p, s);   //      24 (2-deep, two workgroups per CU) likewise
    case 373: return launch_gemm<GemmCfg<128, 128, 2, 4, EBITS, SPLIT, 0, 3>, 9>(p, s);    //      128x128 on EIGHT waves of 64x32 (two per SIMD cover each other's stage-top bubble)
    case 374: return launch_gemm<GemmCfg<128, 128, 4, 2, EBITS, SPLIT, 0, 3>, 9>(p, s);    //      ... of 32x64
    case 325: return launch_gemm<GemmCfg<256, 128, 2, 2, EBITS, SPLIT, 0, 3>, 9>(p, s);   //      = product variant 58
    case 326: return launch_gemm<GemmCfg<128, 256, 2, 2, EBITS, SPLIT, 0, 3>, 9>(p, s);   //      128x256 on four waves of 64x128
    case 327: return launch_gemm<GemmCfg<256, 128, 2, 2, EBITS, SPLIT, 0, 2>, 9>(p, s);   //      ... 2-deep
    case 76: return launch_gemm<GemmCfg<128, 128, 2, 2, EBITS, SPLIT, 0, 4>, 9>(p, s);   // lab: 73 with a 4-deep ring (144 KiB of LDS: one workgroup per CU, which 73's regime is anyway)
    case 79: return launch_gemm<GemmCfg<64, 128, 2, 2, EBITS, SPLIT, 0, 4>, 9>(p, s);    //      72 with a 4-deep ring
    case 224: return launch_gemm<GemmCfg<128, 128, 2, 2, EBITS, SPLIT>, 3>(p, s);   // the round-1 simple schedule (2 stages, reads after the barrier, then MFMAs)
    case 225: return launch_gemm<GemmCfg<256, 128, 4, 2, EBITS, SPLIT>, 3>(p, s);
    case 227: return launch_gemm<GemmCfg<128, 64, 2, 2, EBITS, SPLIT>, 3>(p, s);
    case 228: return launch_gemm<GemmCfg<64, 128, 2, 2, EBITS, SPLIT>, 3>(p, s);
    case 229: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT>, 3>(p, s);
    case 170: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 0, 3>, 7>(p, s);    // the round-1 ring schedule (whole-stage reads after the barrier, then the MFMAs)
    case 171: return launch_gemm<GemmCfg<128, 64, 2, 2, EBITS, SPLIT, 0, 3>, 7>(p, s);
    case 172: return launch_gemm<GemmCfg<64, 128, 2, 2, EBITS, SPLIT, 0, 3>, 7>(p, s);
    case 173: return launch_gemm<GemmCfg<128, 128, 2, 2, EBITS, SPLIT, 0, 3>, 7>(p, s);
    case 1: return launch_gemm<GemmCfg<256, 256, 2, 4, EBITS, SPLIT>, 1>(p, s);
    case 2: return launch_gemm<GemmCfg<128, 128, 2, 2, EBITS, SPLIT>, 0>(p, s);
    case 3: return launch_gemm<GemmCfg<256, 128, 4, 2, EBITS, SPLIT>, 0>(p, s);
    case 4: return launch_gemm<GemmCfg<128, 256, 2, 4, EBITS, SPLIT>, 0>(p, s);
    case 5: return launch_gemm<GemmCfg<256, 256, 2, 4, EBITS, SPLIT>, 0>(p, s);
    case 20: return launch_gemm<GemmCfg<256, 256, 2, 4, EBITS, SPLIT>, 3>(p, s);   // simple schedule, 256x256
    case 26: return launch_gemm<GemmCfg<128, 256, 2, 4, EBITS, SPLIT>, 3>(p, s);
    case 74: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 0, 4>, 7>(p, s);
    case 75: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 0, 6>, 7>(p, s);
    case 80: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 1, 3>, 7>(p, s);     //   ring ablations: no DMA
    case 81: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 2, 3>, 7>(p, s);     //   no MFMA
    case 82: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 32, 3>, 7>(p, s);    //   no fragment reads
    case 83: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 34, 3>, 7>(p, s);    //   DMA + barriers only
    case 84: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 35, 3>, 7>(p, s);    //   barriers only
    case 78: return launch_gemm<GemmCfg<64, 64, 2, 2, EBITS, SPLIT, 16, 3>, 7>(p, s);    //   per-wave timeline of workgroup 0
  }
  if constexpr (EBITS == 8) {
    if (v == 89) return launch_gemm_deepp_sk<GemmCfg<256, 256, 2, 2, 8, true>>(p, s);
    if (v == 30) return launch_gemm<GemmCfg<256, 256, 2, 2, 8, true>, 4>(p, s);   // per-tile deep schedule (round 1)
  }
  if constexpr (EBITS == 4) {
    if (v == 89) return launch_gemm_deepp_sk<GemmCfg<256, 256, 2, 2, 4, false>>(p, s);
    if (v == 99) return launch_gemm_hetero<GemmCfg<256, 256, 2, 2, 4, false>, GemmCfg<128, 128, 2, 2, 4, false, 0, 3>, 17>(p, s);
    // [r6] lab: the other tiles / ring depths of the in-workgroup K-split kernel (563 = 64x32, 564 = 64x64; 565 - 567 = 32x32 with a 4 / 8 / 6-deep ring)
    if (v == 563 || v == 564) {
      const bool deep = cdiv(p.K, 256) > 24;
      if (v == 563) return deep ? launch_gemm_ks<64, 32, 6>(p, s) : launch_gemm_ks<64, 32, 4>(p, s);
      return deep ? launch_gemm_ks<64, 64, 6>(p, s) : launch_gemm_ks<64, 64, 4>(p, s);
    }
    if (v == 565) return launch_gemm_ks<32, 32, 4>(p, s);
    if (v == 566) return launch_gemm_ks<32, 32, 8>(p, s);
    if (v == 567) return launch_gemm_ks<32, 32, 6>(p, s);
    // [r6] 8-wave persistent schedule (gemm_mx_duo.hip.h): 88 burst retirement, 87 retirement behind the last k-slice, 86 = 88 with stage stamps
    if (v == 88) return launch_gemm_duo<GemmCfg<256, 256, 2, 4, 4, false>, 17, 0>(p, s);
    if (v == 87) return launch_gemm_duo<GemmCfg<256, 256, 2, 4, 4, false>, 17, 1>(p, s);
    if (v == 86) return launch_gemm_duo<GemmCfg<256, 256, 2, 4, 4, false>, 17, 0, true>(p, s);
    if (v == 298) return launch_gemm_hetero<GemmCfg<256, 256, 2, 2, 4, false>, GemmCfg<128, 128, 2, 2, 4, false, 128, 4>, 17>(p, s);   // residual tiles with ABL_READS_FIRST
    // 90 with the one-tile form forced (grid == tile count and an even stage count; any other launch runs as 90): 190 = 32x32x64 MFMAs, 191 = 16x16x128 (gemm_mx_deepp16.hip.h)
    if (v == 190) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 32>(p, s);
    if (v == 191) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 16>(p, s);
    // 191 with the K loop's form forced (gemm_mx_deepp16.hip.h): 192 = the loop before the KL_ forms existed, 193 = KL_SCALES, 194 = KL_DMA, 195 = both, 196 = both + KL_SPREAD, 197 = KL_DMA + KL_SPREAD
    if (v == 192) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 160>(p, s);
    if (v == 193) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 160 + KL_SCALES>(p, s);
    if (v == 194) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 160 + KL_DMA>(p, s);
    if (v == 195) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 160 + (KL_SCALES | KL_DMA)>(p, s);
    if (v == 196) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 160 + (KL_SCALES | KL_DMA | KL_SPREAD)>(p, s);
    if (v == 197) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 0, 160 + (KL_DMA | KL_SPREAD)>(p, s);
    if (v == 91) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, true, 17>(p, s);   //   + phase timestamps of workgroup 0 (qutlass_amd_debug_set_trace_buffer)
    if (v == 92) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 2>(p, s);       //   output stores nt
    if (v == 93) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 16>(p, s);      //   sc1
    if (v == 94) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 0>(p, s);       //   default (write-back) policy
    if (v == 95) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 19>(p, s);      //   sc0 sc1 nt
    if (v == 96) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 1>(p, s);       //   sc0
    // timing experiments that change the result (gemm_mx_deepp.hip.h LAB): 97 = no alpha multiply, 197 = half of the stores one stage early, 297 = both
    if (v == 97) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 1>(p, s);
    if (v == 197) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 2>(p, s);
    if (v == 297) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 3>(p, s);
    if (v == 397) return launch_gemm_deepp<GemmCfg<256, 256, 2, 2, 4, false>, false, 17, 4>(p, s);   //   half of the tile is never stored (accumulators kept alive)
    switch (v) {
      case 6: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false>, 2>(p, s);
      case 7: return launch_gemm<GemmCfg<128, 128, 2, 2, 4, false>, 2>(p, s);
      case 8: return launch_gemm<GemmCfg<256, 128, 4, 2, 4, false>, 2>(p, s);
      case 9: return launch_gemm<GemmCfg<128, 256, 2, 4, 4, false>, 2>(p, s);
      case 30: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false>, 4>(p, s);      // deep schedule: 4 waves x 128x128, one tile per workgroup
      case 31: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 8>, 4>(p, s);   //   no epilogue
      case 32: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 9>, 4>(p, s);   //   no DMA, no epilogue
      case 33: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 10>, 4>(p, s);  //   no MFMA, no epilogue
      case 34: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 40>, 4>(p, s);  //   no reads, no epilogue
      case 40: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false>, 5>(p, s);      // regstage schedule: 4 waves x 128x128, copy through registers
      case 41: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 8>, 5>(p, s);   //   no epilogue
      case 42: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 9>, 5>(p, s);   //   no copy, no epilogue
      case 43: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 10>, 5>(p, s);  //   no MFMA, no epilogue
      case 50: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, 64>, 3>(p, s);      // clock probes of 20 / 30 / 40 and their no-epilogue / no-copy ablations
      case 51: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 64>, 4>(p, s);
      case 52: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 64>, 5>(p, s);
      case 53: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 72>, 5>(p, s);
      case 54: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 73>, 5>(p, s);
      case 55: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 74>, 5>(p, s);
      case 56: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 104>, 5>(p, s);
      case 35: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 16>, 4>(p, s);  //   trace
      case 36: return launch_gemm<GemmCfg<256, 256, 2, 2, 4, false, 17>, 4>(p, s);  //   trace, no DMA
      case 21: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, 8>, 3>(p, s);   //   no epilogue
      case 22: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, 9>, 3>(p, s);   //   no DMA, no epilogue
      case 23: return launch_gemm<GemmCfg<256, 256, 2, 4, 4, false, 10>, 3>(p, s);  //   no MFMA, no epilogue
    }
  }
  if constexpr (EBITS == 4 && !SPLIT) {
    const int rc = dispatch_ablation_mx4(v, p, s);
    if (rc >= 0) return rc;
  }
  return fail(QAMD_ERR_INVALID, "%s: unknown gemm_variant %d", name, v);
}
#endif

template <int EBITS, int AFMT, bool RM>
int dispatch_variant(int v, const GemmParams& p, hipStream_t s, const char* name) {
#if QAMD_BENCH
  if constexpr (AFMT == 0 && !RM) {
    if (p.pp_flags & 4096) {   // lab: "pp_flags" bit 12 = the round-1 ring / simple schedules wherever their pipelined successors are picked
      const MxFormRow* f = mx_form(v);
      if (f && f->family == MXF_RING) v += 100;
      else if (f && f->family == MXF_PIPELINED && f->depth == 2) v += 200;   // (the simple schedule is 2-deep: the 3-deep 256x128 form has no round-1 twin)
    }
    if (!mx_form(v)) return dispatch_lab_variant<EBITS>(v, p, s, name);
  }
#endif
  return launch_mx_form<EBITS, AFMT, RM>(v, p, s, name, std::make_integer_sequence<int, MX_NFORMS>());
}

// the e5m2-operand MXFP8 kernels ride with the NVFP4 unit: balances the parallel build
int launch_nn_fused_a5(const GemmParams& p, hipStream_t s, bool per_tile)
#if QAMD_DEF(4)
{
#if QAMD_BENCH
  if (per_tile) return launch_gemm<GemmCfg<256, 256, 2, 2, 8, true, 0, 2, 1>, 6>(p, s);
#endif
  (void)per_tile;
  return launch_gemm_deepp8<GemmCfg<256, 256, 2, 2, 8, true, 0, 2, 1>, true>(p, s);
}
#else
;
#endif

// fp4 / fp8 / fp8 with an e5m2 A are emitted in units 2 / 3 / 4; the row-major-scale op's forms are small and stay with its entry (unit 1)
#if QAMD_TU != 0
#if QAMD_TU == 2
template int dispatch_variant<4, 0, false>(int, const GemmParams&, hipStream_t, const char*);
#else
extern template int dispatch_variant<4, 0, false>(int, const GemmParams&, hipStream_t, const char*);
#endif
#if QAMD_TU == 3
template int dispatch_variant<8, 0, false>(int, const GemmParams&, hipStream_t, const char*);
#if QAMD_BENCH
template int launch_gemm<GemmCfg<256, 256, 2, 2, 8, true>, 6>(GemmParams, hipStream_t);   // lab: per-tile kernel on the (K, M) operand (round 1)
#endif
#else
extern template int dispatch_variant<8, 0, false>(int, const GemmParams&, hipStream_t, const char*);
#if QAMD_BENCH
extern template int launch_gemm<GemmCfg<256, 256, 2, 2, 8, true>, 6>(GemmParams, hipStream_t);
#endif
#endif
#if QAMD_TU == 4
template int dispatch_variant<8, 1, false>(int, const GemmParams&, hipStream_t, const char*);
#else
extern template int dispatch_variant<8, 1, false>(int, const GemmParams&, hipStream_t, const char*);
#endif
#endif

// NVFP4 launches live in their own unit
#if QAMD_DEF(4)
int launch_nvf4_host(const NvLaunch& l, const NvGemmParams& p, hipStream_t s) { return launch_nvf4_gemm(l, p, s) == hipSuccess ? 0 : 1; }
int launch_nvf4_grouped_host(const NvGroupedParams& q, hipStream_t s, int form) { return launch_nvf4_grouped(q, s, form) == hipSuccess ? 0 : 1; }
#else
int launch_nvf4_host(const NvLaunch& l, const NvGemmParams& p, hipStream_t s);
int launch_nvf4_grouped_host(const NvGroupedParams& q, hipStream_t s, int form);
#endif

#if QAMD_DEF(1)
// Small-output regime: ring schedule (one workgroup per CU with several stages in flight beats the 2-stage simple schedule
// whenever the tiles do not fill the chip twice), plus split-K over grid.y when 64x64 tiles leave CUs idle and K is long
// enough to pay for the second pass (>= 32 stages: fp4 K >= 8192).  One function so that the launcher and qutlass_amd_gemm_splitk_workspace_bytes
// agree.  Measured: profiles/native_r1_ring.log.
struct SmallPlan { int variant; int splits; };   // variant 0: not this regime
// split-K scratch: [splits][M][N] fp32 partials (lab library: then, 256-byte aligned, one 64-bit arrival slot per output tile
// for the fused-reduction experiment)
inline int64_t splitk_partial_bytes(int64_t M, int64_t N, int splits) { return (int64_t)splits * M * N * 4; }
inline int64_t splitk_ctr_offset(int64_t M, int64_t N, int splits) { return (splitk_partial_bytes(M, N, splits) + 255) / 256 * 256; }
inline int64_t splitk_ws_bytes(int variant, int64_t M, int64_t N, int splits) {
#if QAMD_BENCH
  const MxFormRow* f = mx_form(variant);   // a ring form (only those split); a number without a row: the smallest ring tile, which has the most arrival slots
  if (!f) f = &kMxForm<MXV_RING64>;
  return splitk_ctr_offset(M, N, splits) + cdiv(M, f->tm) * cdiv(N, f->tn) * 8;
#else
  (void)variant;
  return splitk_partial_bytes(M, N, splits);
#endif
}
// the round-1/2 rule: thresholds on the tile counts (fitted on sweeps of the in-stream C++ harness, profiles/native_r1_ring.log, native_r2_tilesplit.log)
template <int EBITS>
SmallPlan plan_small_rule(int64_t M, int64_t N, int64_t K, int64_t cus, bool may_split) {
  const int64_t T64 = mx_tiles<MXV_RING64>(M, N), T128 = mx_tiles<MXV_RING128>(M, N);
  if (T64 <= cus) {
    const int64_t KT = cdiv(K * EBITS / 8, 128);
    int64_t S = 1;
    if (may_split && T64 < cus && KT >= opt_splitk_min_kt()) {                          // shorter K: the reduce pass costs more than it saves
      const int64_t wg = opt_splitk_wg() > 0 ? opt_splitk_wg() : cus;
      S = std::min<int64_t>(std::min<int64_t>(8, wg / T64), KT / 8);   // up to one workgroup per CU, >= 8 stages per split
      if (S < 1) S = 1;
      const int64_t per = cdiv(KT, S);
      S = cdiv(KT, per);                                                // every split non-empty
      // a two-way split (more than 64 tiles) halves the K loop at best and pays a second launch + the reduce pass (~3.5 us): it
      // needs ~48 stages to win (M = 128, N = 4096: K = 8192 7.6 us unsplit vs 9.8 us split; K = 14336 17.3 vs 14.0 us;
      // profiles/native_r2_tilesplit.log)
      if (S == 2 && KT < 48) S = 1;
    }
    return {MXV_RING64, (int)S};
  }
  if (T64 <= 2 * cus) return {N >= M ? MXV_RING64x128 : MXV_RING128x64, 1};
  if (M > 64 && N > 64 && T128 <= cus) return {MXV_RING128, 1};
  return {0, 1};
}

// [r3] ... corrected by a fitted cost model where that rule leaves a long K to too few, too small tiles: it only ever splits 64x64 tiles, so 96 x 5120 x 25600
// ran 160 tiles of 64x64 unsplit (27.5 us; MXFP8 50.3) where 40 tiles of 128x128 in 4 K ranges take 19.5 (30.4).  tools/calib_mx_small.py timed the ring schedule
// on 64x64 / 64x128 / 128x128 tiles with 1 / 2 / 4 / 8 K ranges on 132 shapes per format (profiles/calib_mx_small_r3.txt); least squares on log time (rms 14 % /
// 18 %, measurements >= 13 us only -- below that the Python caller of the calibration is the bound) give, per tile kernel,
//     a + g b kt / 16 [+ r0 + (S + 1) M N 4 bytes / bw for the reduce pass]      kt = 128-byte K stages per workgroup, g = 1 while workgroups <= CUs, else
//                                                                                ceil(workgroups / CUs) e
// The model is a CORRECTION, not the rule: it replaces the rule's choice only where its own prediction for that choice is more than 8 % above its best candidate
// and the best candidate takes >= 12 us (K ranges of >= 4 stages).  Against the calibration: 23 of 264 shapes change, MXFP4 96 / 128 x 8192 x 28672 32.4 / 34.1 ->
// 28.2 / 30.5 us, x 5120 x 25600 27.5 / 28.0 -> 19.5 / 21.1; MXFP8 192 / 256 x 4096 x 14336 30.9 / 31.5 -> 23.0 / 25.3, 96 ... 384 x 5120 x 25600 50 ... 68 -> 30 ... 54,
// 96 ... 256 x 8192 x 28672 59 ... 84 -> 44 ... 70; three shapes lose 2 - 4 % (MXFP8 16 / 32 x 8192 x 8192, MXFP4 64 x 8192 x 28672).
template <int EBITS>
SmallPlan plan_small(int64_t M, int64_t N, int64_t K, int64_t cus, bool may_split) {
  const SmallPlan cur = plan_small_rule<EBITS>(M, N, K, cus, may_split);
  static constexpr MxFormRow CAND[3] = {kMxForm<MXV_RING64>, kMxForm<MXV_RING64x128>, kMxForm<MXV_RING128>};      // (MXV_RING128x64: M > N, not calibrated)
  int ccur = -1;
  for (int c = 0; c < 3; ++c)
    if (cur.variant == CAND[c].variant) ccur = c;
  if (ccur < 0) return cur;
  //                                   64x64  64x128 128x128
  static constexpr double A4[3] = {6.07, 6.04, 6.30}, B4[3] = {3.41, 4.80, 6.58}, E4[3] = {0.99, 1.2, 1.2};
  static constexpr double A8[3] = {3.31, 3.79, 2.91}, B8[3] = {3.87, 4.83, 6.41}, E8[3] = {0.90, 1.2, 1.2};
  const double* A = EBITS == 4 ? A4 : A8;
  const double* B = EBITS == 4 ? B4 : B8;
  const double* E = EBITS == 4 ? E4 : E8;
  const double r0 = EBITS == 4 ? 1.39 : 3.86, bw = EBITS == 4 ? 2.63e6 : 2.79e6;
  const int64_t KT = cdiv(K * EBITS / 8, 128);
  auto price = [&](int c, int S, int* s2) {
    const int64_t per = cdiv(KT, S), S2 = cdiv(KT, per);
    const double n = (double)(cdiv(M, CAND[c].tm) * cdiv(N, CAND[c].tn) * S2) / (double)cus;
    double t = A[c] + (n <= 1.0 ? 1.0 : std::ceil(n) * E[c]) * B[c] * (double)per / 16.0;
    if (S2 > 1) t += r0 + (double)(S2 + 1) * (double)M * (double)N * 4.0 / bw;
    *s2 = (int)S2;
    return t;
  };
  int s2;
  const double t_cur = price(ccur, cur.splits, &s2);
  SmallPlan best = cur;
  double t_best = t_cur;
  for (int c = 0; c < 3; ++c)
    for (int S = 1; S <= (may_split && N % 4 == 0 ? 8 : 1); S *= 2) {
      if (S > 1 && cdiv(KT, S) < 4) continue;
      const double t = price(c, S, &s2);
      if (S > 1 && s2 < 2) continue;
      if (t < t_best) { t_best = t; best = {CAND[c].variant, s2}; }
    }
  SmallPlan res = (t_best >= 12.0 && t_best < 0.92 * t_cur) ? best : cur;
  // A long K (>= 96 stages) on 64x128 tiles, single pass: 128x128 tiles in two K ranges while those still fit one per CU -- the guard above leaves these alone (the fit
  // is coarse there), the GPU-only measurement does not: all ten such shapes of the calibration grid gain 8 ... 25 % (MXFP8 384 / 512 x 4096 x 14336 38.6 / 43.0 -> 32.1 /
  // 36.1 us, MXFP4 256 x 8192 x 28672 46.1 -> 42.2, 384 x 5120 x 25600 41.0 -> 36.2), every shape with fewer stages ties or loses
  // (profiles/calib_mx_small_r3_graph_m192_1024.txt, profiles/instream_mx_plan_check_r3.txt)
  if (may_split && N % 4 == 0 && res.variant == MXV_RING64x128 && res.splits == 1 && KT >= 96 && 2 * mx_tiles<MXV_RING128>(M, N) <= cus) res = {MXV_RING128, 2};
  return res;
}

// [r6] When does the in-workgroup K-split kernel (gemm_mx_ks.hip.h, one 32x32 tile per workgroup of four waves) take an MXFP4 shape?  Measured against the plans below on
// M = 1 ... 256 x 14 (N, K) (tools/calib_ks.py, profiles/calib_ks_r6g.txt; GPU-only timing, both sides with caller scratch):
//   * the tiles must fit one per CU (two workgroups on a CU share its LDS-DMA path: +40 ... +100 %), and
//   * with a long K (> 24 stages of 256) they must also fill more than half the chip: below that the split-K plans, which spread K over more CUs, are ahead
//     (N = 4096, K = 14336: M <= 16 8.1-9.1 us split against 9.2-9.4; M = 64 11.4 against 9.8).
// Where it applies it is 11 ... 30 % faster (N = K = 4096: M <= 64 4.9-5.3 -> 4.1-4.5 us; 8192^2: M <= 32 8.8-11.1 -> 7.4-7.8 us), M = 1 ... 8 included (the LDS-free
// split-K kernel: 4.55-4.92 us at N = K = 4096).  32x64 tiles: only where 32x32 tiles just overflow the chip and 32x64 nearly fill it (N = 14336: -6 %).
// Returns the variant (a wave-owned, decode or K-split row of MX_FORMS) or 0.
inline int ks_plan(int64_t M, int64_t N, int64_t K, int64_t cus) {
  const int64_t KT = cdiv(K, 256);
  const int64_t T32 = mx_tiles<MXV_KS32>(M, N);
  // [r6] K <= 4096: the tile's whole K extent fits the LDS -- the one-shot kernel (gemm_mx_os.hip.h), no ring and no barrier in the K walk: N = K = 4096, M = 1 ... 64
  // 4.05-4.39 -> 3.34-3.67 us, N = K = 2048 3.15-3.26 -> 2.62-2.77 (profiles/calib_os_r6q.txt); its wave-owned-ring form for longer K and 16 columns per workgroup where os_plan says so
  // (4096 x 8192, M <= 32: 5.8-7.1 -> 5.5-5.7 us); past one tile per CU the ring plans below keep the shape
  if (M <= 16) {   // [r6] the decode form with wider column tiles (os16_wide_plan)
    if (const int v = os16_wide_plan(4, N, K, cus)) return v;
  }
  if (const int tn = os_plan(M, N, K, cus)) {
    // [r6] decode form (gemm_mx_os16_kernel, 16x16 tiles on the 16x16x128 MFMA) wherever those fit one per CU: a third fewer bytes through each CU's LDS-DMA path
    // (N = K = 4096, M <= 16: 3.25-3.31 -> 2.86-2.92 us; K = 8192 5.0-5.2 -> 3.7-4.1; K = 14336 6.8-7.0 -> 6.1-6.5; two per CU (N = 8192) lose 9 %; profiles/calib_os16_r7.txt)
    if (mx_tiles<MXV_D16>(M, N) <= cus) return MXV_D16;
    return tn == 16 ? MXV_OS16 : MXV_OS32;
  }
  if (os64_plan(M, N, K, cus)) return MXV_OS64;   // [r6] 64x32 tiles on wave-owned K stages where 32x32 tiles overflow the chip
  if (T32 <= cus && (KT <= 24 || (2 * T32 > cus && KT <= 64))) return MXV_KS32;   // (K > 16384 was not calibrated, and a split-K plan on larger tiles moves fewer bytes per CU there)
  const int64_t T64 = mx_tiles<MXV_KS32x64>(M, N);
  if (M <= 32 && T32 > cus && T64 <= cus && 8 * T64 >= 7 * cus && KT <= 24) return MXV_KS32x64;
  return 0;
}

// ---- the MX GEMM plan: pure host functions of the shape, the caller's scratch and the CU count, shared by the launchers, the workspace query and the debug entries

// The kernels address an operand through 32-bit buffer-descriptor offsets (< 2 GiB); the reference's CUTLASS kernels use 64-bit strides.  A larger operand runs as
// ranges of whole gran-row / gran-column tiles with rebased operand / scale / D pointers: column ranges of B (e.g. a 262400 x 16384 fp4 weight), each writing its
// columns of the same D (row stride N) with A shared, and inside each of them row ranges of A (large batch x long K, e.g. 262144 x 16384 fp4) with B shared.  Every
// output element is computed by exactly one launch, in the same K order.  f(r0, c0, m, n) runs once per range; returns the first non-zero code.
template <class F>
int for_each_range(const char* name, int64_t M, int64_t N, int64_t rowbytes, int gran, F&& f) {
  const int64_t lim = ((1ll << 31) - 1) / rowbytes / gran * gran;
  const bool split_n = N * rowbytes >= (1ll << 31), split_m = M * rowbytes >= (1ll << 31);
  if (split_n && lim < gran) return fail(QAMD_ERR_INVALID, "%s: K too large for a %d-column range of B to stay below 2 GiB", name, gran);
  if (split_m && lim < gran) return fail(QAMD_ERR_INVALID, "%s: K too large for a %d-row range of A to stay below 2 GiB", name, gran);
  const int64_t cols = split_n ? lim : N, rows = split_m ? lim : M;
  for (int64_t c0 = 0; c0 < N; c0 += cols)
    for (int64_t r0 = 0; r0 < M; r0 += rows)
      if (int rc = f(r0, c0, std::min(rows, M - r0), std::min(cols, N - c0))) return rc;
  return QAMD_OK;
}

// One launch of a range: `variant` (an MxVariant, or a lab number) over columns [c0, c0 + n) of the range, K in `splits` ranges (> 1: fp32 partials in the
// caller's scratch, then the reduce pass).  A range takes at most two launches (the lab's two-launch experiment, "pp_flags" bit 13).
// ws: split-K scratch of the range's split form, what the caller's scratch must hold for the split to be taken (0: none)
struct MxLaunch { int variant; int64_t c0, n; int splits; };
struct MxPlan {
  int n = 0; MxLaunch l[2]; int64_t ws = 0;
  MxPlan& add(int variant, int64_t c0, int64_t n_cols, int splits = 1) { l[n++] = {variant, c0, n_cols, splits}; return *this; }
};

// a_fmt (MXFP8 only): QAMD_FP8_E4M3 / QAMD_FP8_E5M2 element format of A; ldd: row stride of D (the whole output's N); avail: bytes of the caller's scratch (0: none)
template <int EBITS>
MxPlan mx_plan(int a_fmt, int64_t M, int64_t N, int64_t K, int64_t ldd, int64_t avail, int cus) {
  MxPlan r;
  const int pp = opt_pp_flags();
  int variant = opt_gemm_variant();
  if (variant >= 61 && variant <= 66) variant = 0;   // these select the NN operand path only (matmul_mxf8_bf16_nn)
  // ring schedule + optional split-K (needs caller scratch; "pp_flags" bit 7 turns split-K off, bit 8 the ring rule)
  // the plan with K ranges needs the caller's scratch; without it (or with too little) the best single-pass plan
  auto can_split = [&](int v, int splits) { return splits > 1 && avail >= splitk_ws_bytes(v, M, N, splits) && !(pp & 128); };
  SmallPlan pl = plan_small<EBITS>(M, N, K, cus, true);
  if (pl.variant && pl.splits > 1) r.ws = splitk_ws_bytes(pl.variant, M, N, pl.splits);
  if (pl.variant && pl.splits > 1 && !can_split(pl.variant, pl.splits)) pl = plan_small<EBITS>(M, N, K, cus, false);
  auto ring = [&](int v, int splits) -> MxPlan& {
    const int64_t KT = cdiv(K * EBITS / 8, 128);   // every split non-empty (a forced count may not divide the K stages)
    splits = (int)std::min<int64_t>(std::max(splits, 1), std::min<int64_t>(KT, 8));
    splits = (int)cdiv(KT, cdiv(KT, splits));
    return r.add(v, 0, N, can_split(v, splits) ? splits : 1);
  };
  if (variant == 77) return ring(MXV_RING64, pl.variant == MXV_RING64 ? pl.splits : 1);   // lab: 64x64 ring (+ split-K) whatever M
  if (opt_splitk_force() > 0 && mx_form(variant) && mx_form(variant)->family == MXF_RING) return ring(variant, opt_splitk_force());   // lab: forced tile x forced split
  // small batch (M <= 32): weight-bandwidth bound.  With fewer than 128 64-row tiles (N < 8192) the split-K kernel without
  // LDS staging wins (gemm_mx_skinny.hip.h: N = K = 4096, M = 16: 5.9 us vs 7.1 us for the ring kernel on 64 CUs); from
  // 128 tiles on, the 64x64 ring kernel streams the weight through full-line LDS-DMA and wins (N = 14336, K = 4096: 6.9 us
  // vs 9.7 us; N = 57344, K = 8192: 36 us vs 58-74 us), as does ring + split-K over caller scratch for a long K
  // (N = 4096, K = 14336, M = 16: 11.6 us vs 14.8 us).  profiles/native_r1_skinny_shapes.log, native_r1_ring.log
  // [r3] re-measured GPU-only (HIP-graph replays, tools/calib_mx_small.py with CALIB_MS=1,4,8,16,24,32; profiles/calib_mx_decode_graph_r3.txt): the split-K kernel's time
  // grows with M (N = K = 4096: 4.65 us at M = 1, 5.4 at 16, 6.1 at 32) while the 3-deep ring stays at 5.0 -- it keeps M <= 8 (now including N = 8192: 8.9 us against
  // the ring's 10.8 at K = 8192) and M <= 24 only against small weights (N <= 2048: 3.7 against 3.9 us)
  // [r6] small batches against a weight that fills the chip with 32x32 tiles: the in-workgroup K-split kernel (gemm_mx_ks.hip.h; ks_plan above)
  // [r6] MXFP8 small batches (e4m3 and e5m2 A): the wave-owned kernel where os8_plan says so
  if (variant == 0 && !(pp & 256)) {
    if (const int kv = EBITS == 4 ? ks_plan(M, N, K, cus) : os8_plan(M, N, K, cus)) { r.ws = 0; return r.add(kv, 0, N); }
  }
  const bool split = pl.variant && can_split(pl.variant, pl.splits);
  const bool skinny_auto = variant == 0 && !split && ((M <= 8 && cdiv(N, 64) <= cus / 2) || (M <= 24 && cdiv(N, 64) <= cus / 8));
  if (EBITS == 4 && (variant == MXV_SKINNY || (variant >= 44 && variant <= 49) || skinny_auto)) return r.add(variant ? variant : MXV_SKINNY, 0, N);
  if (variant == 0 && !(pp & 256) && pl.variant) return ring(pl.variant, pl.splits);
  if (variant == 0) {
    // auto (measured, profiles/native_r1_schedules.log, profiles/bench_sweep_*.txt): the largest tile that still gives
    // every CU work -- 256x256 ("deep" schedule, 4 waves of 128x128), then 128x128, 128x64 / 64x128, 64x64 (simple
    // schedule, several workgroups per CU).  (fp4 with M <= 32 went to the split-K kernel above.)
    const int64_t want = cus * 3 / 4;   // 3/4 of the CUs
    // no point in tiles taller than the problem; 64x64 until 64x128 tiles fill the chip 1.5 times (weight-bandwidth
    // bound: N = 28672, K = 4096, M = 32: 12.6 us with 448 tiles of 64x64 vs 14.3 us with 224 of 64x128)
    if (M <= 64) variant = (mx_tiles<MXV_P64x128>(M, N) >= cus * 3 / 2) ? MXV_P64x128 : MXV_P64;
    else if (N <= 64) variant = (mx_tiles<MXV_P128x64>(M, N) >= want) ? MXV_P128x64 : MXV_P64;
    // [r3] at most 128 rows against a wide weight (more 128x128 tiles than CUs): the 256-row persistent tile would be half empty -- 128x128 tiles, two workgroups
    // per CU (96 x 57344 x 8192: 52.4 -> 42.7 us, 128 x 51200 x 5120: 32.7 -> 26.8, MXFP8 96 x 57344 x 8192 113.5 -> 100.3; profiles/calib_mx_small_r3.txt)
    else if (M <= 128 && mx_tiles<MXV_P128>(M, N) >= want) variant = MXV_P128;
    // [r3] ... or more than HALF of them with K >= 8 stages: the smaller tiles then no longer fit one round (128x128: two per CU, 256x128: one per CU --
    // both hold exactly cus / 2 tiles' worth of 256x256 output), and a second, part-filled round costs more than idle CUs do:
    // 2560 x 4096 x 4096 (160 tiles) 34.6 -> 28.8 us, 1536 x 6144 x 4096 33.2 -> 28.3, 2048 x 5120 x 5120 42.2 -> 35.3, MXFP8 2560 x 4096 x 4096
    // 49.3 -> 39.4, K = 14336 likewise (146.9 -> 120.9); at exactly half (2048 x 4096: 128 tiles) the small tiles tie or win
    // (tools/calib_tiles.py, profiles/calib_tiles_r3.txt; found by tools/dip_scan.py: a LARGER batch ran faster)
    else if (mx_tiles<MXV_PERSISTENT>(M, N) >= want || (2 * mx_tiles<MXV_PERSISTENT>(M, N) > cus && cdiv(K * EBITS / 8, 128) >= 8)) {
      // the persistent deep schedule (one workgroup per CU walks the tiles, epilogue folded into the last K stage), fp4 and
      // fp8; its epilogue addresses a tile with 32-bit byte offsets, so absurdly wide outputs stay with 256x128 simple tiles
      const int big = ldd < (1ll << 22) ? MXV_PERSISTENT : MXV_P256x128_W8;
      variant = big;
      // Wave quantisation: T tiles on `cus` CUs run ceil(T / cus) rounds, the last one part-filled (4096 x 5120: 320 tiles =
      // 1.25 rounds).  [r3] The residual tiles run as 128x128 quarter tiles on extra workgroups of the SAME launch
      // (gemm_mx_hetero_kernel: dispatched CU by CU as the persistent workgroups retire) whenever the cost model says so;
      // otherwise ONE persistent launch with balanced rounds (deepp_grid).
      constexpr MxFormRow BIG = kMxForm<MXV_PERSISTENT>;
      const int64_t tm = cdiv(M, BIG.tm), tn = cdiv(N, BIG.tn), T = tm * tn;
      bool hetero_ok = big == MXV_PERSISTENT && !(pp & 64);   // (lab, "pp_flags" bit 6: balanced rounds only)
#if QAMD_BENCH
      // lab, "pp_flags" bit 13: the round-1/2 form of the same idea INSTEAD -- the trailing tile columns as a SECOND launch of smaller
      // tiles (kept for the A/B in profiles/native_r3_heterobench.log)
      const int64_t full = (T / cus) * cus, main_cols = (tm > 0) ? full / tm : 0;
      const bool two_launch = (pp & 8192) != 0;
      if (two_launch && hetero_ok && full >= cus && full < 3 * cus && main_cols >= 1 && main_cols < tn && (T - main_cols * tm) <= 80) {
        const int64_t n1 = main_cols * BIG.tn, Nt = N - n1;
        const int vt = (mx_tiles<MXV_P256x128_W8>(M, Nt) >= want) ? MXV_P256x128_W8 : (mx_tiles<MXV_P128>(M, Nt) >= want) ? MXV_P128 : (mx_tiles<MXV_P128x64>(M, Nt) >= want) ? MXV_P128x64 : MXV_P64;
        return r.add(big, 0, n1).add(vt, n1, Nt);
      }
      if (two_launch) hetero_ok = false;
#endif
      if (hetero_ok && hetero_wins(T, cus)) variant = MXV_HETERO;
    }
    else if (mx_tiles<MXV_P128>(M, N) >= want) {
      // [r3] half-chip outputs (fewer than `want` tiles of 256x256): with a long K (>= 32 stages) the 256x128 tile on four waves wins 5-6 %
      // over 128x128 tiles on two workgroups per CU; with K = 4096 the two tie (22.97 vs 22.95 us at 2048 x 4096 x 4096) and 128x128 stays
      const int64_t KTs = cdiv(K * EBITS / 8, 128);
      // (MXFP8 likewise: 2048 x 4096 x 4096 34.9 -> 32.7 us, x 8192 63.2 -> 57.1 us; K = 2048 = 16 stages: -2 %, stays)
      variant = (M >= 256 && KTs >= 32 && mx_tiles<MXV_P256x128>(M, N) >= want) ? MXV_P256x128 : MXV_P128;
      // [r3] ... and, at the same K, whenever the 128x128 grid no longer fits one tile per CU while the 256x128 grid still does: the CUs that hold
      // two 128x128 tiles set the kernel's time.  MXFP8 768 x 6144 x 4096 28.3 -> 23.5 us, 1024 x 5120 x 5120 36.9 -> 29.6, 1024 x 5120 x 25600
      // 145.3 -> 120.8; MXFP4 1024 x 5120 x 25600 83.5 -> 75.2.  Not below 32 stages: MXFP4 2048 x 4096 x 4096 23.6 against 26.6 on the 256x128 tile
      // (profiles/calib_tiles_r3.txt)
      if (M >= 256 && KTs >= 32 && mx_tiles<MXV_P128>(M, N) > cus && mx_tiles<MXV_P256x128>(M, N) <= cus) variant = MXV_P256x128;
    }
    else if (mx_tiles<MXV_P128x64>(M, N) >= want || mx_tiles<MXV_P64x128>(M, N) >= want) variant = (N >= M) ? MXV_P128x64 : MXV_P64x128;
    else variant = MXV_P64;
  }
  if (variant == 89) {   // (lab: forced stream-K; falls back to the persistent kernel when the shape has nothing to cut or the scratch is missing)
    const int64_t T = mx_tiles<MXV_PERSISTENT>(M, N), KTe = (cdiv(K * EBITS / 8, 128) + 1) / 2 * 2;
    const bool ok = a_fmt == 0 && avail >= sk_ws_bytes(cus) && T % cus != 0 && T > cus && KTe >= 8 && (K * EBITS / 8) % 256 == 0 && ldd < (1ll << 22);
    if (!ok) variant = MXV_PERSISTENT;
  }
  return r.add(variant, 0, N);
}

// matmul_ada_mxf4_bf16_tn (row-major scales): the form of the kernel with row-major scale fetch, a row of MX_FORMS with MXOP_ADA -- the LDS-free split-K
// kernel, the 64x64 ring (lab: 178 = its round-1 schedule), the wave-owned kernel with 32x32 / 32x16 / 64x32 tiles, its decode form
// with 16 / 32 / 48 / 56 / 64 columns per workgroup.  Never split-K: the op has no scratch argument.
inline int ada_plan(int64_t M, int64_t N, int64_t K, int cus) {
  // Same regimes as matmul_mxf4_bf16_tn: the LDS-free split-K kernel while the weight has fewer than 128 64-row tiles;
  // from 128 tiles on (N >= 8192) the 64x64 ring kernel with row-major scale fetch streams the weight through full-line
  // LDS-DMA (M = 16: N = 14336, K = 4096 9.7 -> 6.9 us; N = 57344, K = 8192 62.6 -> 39.9 us), and any M > 32 goes there
  // too ("gemm_variant" 60 / 70 force either).
  const int forced = opt_gemm_variant();
  const int64_t T64 = cdiv(N, 64);   // (no split-K here -- the op has no scratch argument -- so a long K on few tiles stays with the split-K kernel:
                                     //  8 x 8192 x 28672: 27.9 us vs 34.2 us on 128 workgroups of the ring kernel)
  const bool ring = forced == MXV_RING64 || (forced != MXV_SKINNY && (M > 32 || T64 >= cus || (T64 >= cus / 2 && K < 16384)));
  // [r6] K <= 4096 and at most one 32x32 tile per CU: the one-shot kernel with row-major scale pieces (gemm_mx_os.hip.h; "gemm_variant" 568 forces it where it fits)
  const int os_tn = forced == 0 ? os_plan(M, N, K, cus, true) : 0;
  const bool os16 = forced == MXV_OS16 || os_tn == 16;   // 16 columns per workgroup
  // [r6] ... its decode form (16x16 tiles on the 16x16x128 MFMA) where those fit one per CU (matmul_mxf4_bf16_tn's rule, ks_plan)
  const MxFormRow* ff = mx_form(forced);
  if (ff && ff->family == MXF_DECODE) return forced;
  if (os_tn != 0 && mx_tiles<MXV_D16>(M, N) <= cus) return MXV_D16;
  if (forced == 0 && M <= 16) {
    if (const int v = os16_wide_plan(4, N, K, cus)) return v;   // (wider column tiles: matmul_mxf4_bf16_tn's rule)
  }
  const bool os64 = forced == MXV_OS64 || (forced == 0 && os_tn == 0 && os64_plan(M, N, K, cus, true));   // 64x32 tiles where the 32-row tiles overflow the chip (os64_plan)
  const bool oneshot = (ff && ff->family == MXF_OS) ? mx_tiles<MXV_OS32>(M, N) <= 4 * cus : (os_tn != 0 || os64);
  if (oneshot) return os64 ? MXV_OS64 : os16 ? MXV_OS16 : MXV_OS32;
  if (ring) return forced == 178 ? 178 : MXV_RING64;
  return MXV_SKINNY;
}

// ---- the executor.  The operands of one MX GEMM: scales in the to_blocked layout (128-row blocks of ceil(K / 128) 512-byte pieces: the TN and NN ops) or row-major (rows, K / 32)
// (rm: matmul_ada_mxf4_bf16_tn); ldd: row stride of D in elements
// group: K elements per scale (32: the MX formats, 16: NVFP4)
struct MxArgs { const void *A, *B, *A_sf, *B_sf; const float* alpha; void* D; int64_t K, ldd; int ebits; bool rm; int group = 32; };
// the operand, scale and output fields of rows [r0, r0 + m) x columns [c0, c0 + n) of the output (with blocked scales r0 and c0 are multiples of 128); P: GemmParams / NvGemmParams
template <class P>
inline P operand_params(const MxArgs& x, int64_t r0, int64_t c0, int64_t m, int64_t n) {
  const int64_t rowbytes = x.K * x.ebits / 8, KB = x.K / x.group, CB = cdiv(KB, 4);
  auto sf_offset = [&](int64_t row) { return x.rm ? row * KB : (row / 128) * CB * 512; };
  auto sf_bytes = [&](int64_t rows) { return (uint32_t)(x.rm ? rows * KB : cdiv(rows, 128) * CB * 512); };
  P p{};
  p.A = (const uint8_t*)x.A + r0 * rowbytes; p.B = (const uint8_t*)x.B + c0 * rowbytes;
  p.SFA = (const uint8_t*)x.A_sf + sf_offset(r0); p.SFB = (const uint8_t*)x.B_sf + sf_offset(c0);
  p.alpha = x.alpha; p.D = (uint16_t*)x.D + r0 * x.ldd + c0; p.M = (int)m; p.N = (int)n; p.K = (int)x.K; p.ldd = (int)x.ldd;
  p.a_bytes = (uint32_t)(m * rowbytes); p.b_bytes = (uint32_t)(n * rowbytes);
  p.sfa_bytes = sf_bytes(m); p.sfb_bytes = sf_bytes(n);
  p.dbg = opt_dbg();
  p.splits = 1;
  return p;
}
inline GemmParams mx_params(const MxArgs& x, int64_t r0, int64_t c0, int64_t m, int64_t n) {
  GemmParams p = operand_params<GemmParams>(x, r0, c0, m, n);
  p.pp_shift = opt_pp_shift(); p.pp_flags = opt_pp_flags();
  return p;
}
inline NvGemmParams nv_params(const MxArgs& x, int64_t r0, int64_t c0, int64_t m, int64_t n) {
  NvGemmParams p = operand_params<NvGemmParams>(x, r0, c0, m, n);
  p.sk_tag = next_launch_tag();
  return p;
}
inline SkinnyParams skinny_params(const GemmParams& p) {
  SkinnyParams q;
  q.A = p.A; q.B = p.B; q.SFA = p.SFA; q.SFB = p.SFB; q.alpha = p.alpha; q.D = p.D; q.M = p.M; q.N = p.N; q.K = p.K;
  q.a_bytes = p.a_bytes; q.b_bytes = p.b_bytes; q.sfa_bytes = p.sfa_bytes; q.sfb_bytes = p.sfb_bytes; q.ldd = p.ldd;
  return q;
}

int launch_mx_skinny(bool rm, const GemmParams& p, hipStream_t s) {
  constexpr MxFormRow F = kMxForm<MXV_SKINNY>;   // wm waves; depth segments per wave per trip: 32 b128 loads in flight per wave
  if (rm) launch_skinny<false, F.wm, F.depth, false>(skinny_params(p), s);
  else launch_skinny<true, F.wm, F.depth, false>(skinny_params(p), s);
  return check_launch("gemm_mx_skinny_kernel");
}

// the second launch of a split: sum the `splits` K ranges of fp32 partials in ws in fixed z order, alpha, bf16 (deterministic; gemm_mx.hip.h)
inline int splitk_reduce(const char* name, int splits, const void* ws, uint16_t* D, const float* alpha, int M, int N, int ldd, hipStream_t s) {
  const int64_t quads = (int64_t)M * (N / 4);
  const int grid = (int)std::min<int64_t>(cdiv(quads, 256), 2048);
  switch (splits) {
#define QAMD_RED(S_) case S_: hipLaunchKernelGGL(splitk_reduce_kernel<S_>, dim3(grid), dim3(256), 0, s, (const float*)ws, D, alpha, M, N, ldd); break;
    QAMD_RED(2) QAMD_RED(3) QAMD_RED(4) QAMD_RED(5) QAMD_RED(6) QAMD_RED(7) QAMD_RED(8)
#undef QAMD_RED
    default: return fail(QAMD_ERR_INVALID, "%s: unsupported split count %d", name, splits);
  }
  return check_launch("splitk_reduce_kernel");
}

// one planned launch of matmul_mx{f4,f8}_bf16_tn, then the reduce pass of a split
template <int EBITS>
int mx_launch(const char* name, const MxLaunch& l, GemmParams p, void* ws, int a_fmt, hipStream_t s) {
  // one place decides which instantiation family a variant number is looked up in
  auto dispatch = [&](int v) -> int {
    if (EBITS == 8 && a_fmt == 1) return dispatch_variant<8, 1, false>(v, p, s, name);
    return dispatch_variant<EBITS, 0, false>(v, p, s, name);
  };
#if QAMD_BENCH
  if (EBITS == 4 && l.variant >= 44 && l.variant <= 49) {   // lab-only shapes of the split-K kernel (waves, segments per trip, chunk mapping)
    const SkinnyParams q = skinny_params(p);
    switch (l.variant) {
      case 44: launch_skinny<true, 8, 2, true>(q, s); break;
      case 45: launch_skinny<true, 4, 2, false>(q, s); break;
      case 46: launch_skinny<true, 4, 2, true>(q, s); break;
      case 47: launch_skinny<true, 8, 2, false>(q, s); break;
      case 48: launch_skinny<true, 8, 1, true>(q, s); break;
      case 49: launch_skinny<true, 4, 4, true>(q, s); break;
    }
    return check_launch("gemm_mx_skinny_kernel");
  }
  if (l.variant == 89) {   // lab: stream-K over the caller's scratch (the persistent kernel when that is not 16-byte aligned)
    if ((uintptr_t)ws % 16) return dispatch(MXV_PERSISTENT);
    const int cus = chip_cus();
    p.sk_tiles = (int)(cus + cdiv(p.M, 256) * cdiv(p.N, 256) % cus);
    p.ws = (float*)ws;
    p.ctr = (unsigned long long*)((char*)ws + (int64_t)cus * SK_PART_BYTES);
    p.tag = next_launch_tag();
    return dispatch(89);
  }
#endif
  if (l.splits == 1) return dispatch(l.variant);
  p.ws = (float*)ws; p.splits = l.splits;
#if QAMD_BENCH
  if (p.pp_flags & 512) {   // lab: ONE launch, the last split to arrive for a tile reduces it (gemm_mx.hip.h epilogue_splitk_fused);
                            // measured slower than the reduce kernel below, see there
    p.ctr = (unsigned long long*)((char*)ws + splitk_ctr_offset(p.M, p.N, l.splits));
    p.tag = (next_launch_tag() & ((1ull << 56) - 1)) << 8;
    return dispatch(l.variant);
  }
#endif
  if (int rc = dispatch(l.variant)) return rc;
  return splitk_reduce(name, l.splits, ws, p.D, p.alpha, p.M, p.N, p.ldd, s);
}

// the argument checks of the plain TN GEMMs: K >= kmin and a multiple of kalign; mn_got: the M / N message names the values (the MX ops)
inline int gemm_check(const char* name, int kmin, int kalign, bool mn_got, const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha,
                      const void* D, int64_t M, int64_t N, int64_t K) {
  if (!A || !B || !A_sf || !B_sf || !alpha || !D) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  // [r5] operands are fetched as 16-byte LDS-DMA pieces and the output leaves as 16-byte stores (the reference's CUTLASS kernels ask for 128-bit alignment as well, via TMA)
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)A_sf | (uintptr_t)B_sf | (uintptr_t)D) % 16)
    return fail(QAMD_ERR_INVALID, "%s: A, B, the scale operands and D must be 16-byte aligned", name);
  if (M <= 0 || N <= 0)
    return mn_got ? fail(QAMD_ERR_INVALID, "%s: M and N must be positive (got M=%lld N=%lld)", name, (long long)M, (long long)N)
                  : fail(QAMD_ERR_INVALID, "%s: M and N must be positive", name);
  if (K < kmin || K % kalign) return fail(QAMD_ERR_INVALID, "%s: K must be a positive multiple of %d (got %lld)", name, kalign, (long long)K);
  if (N % 8) return fail(QAMD_ERR_INVALID, "%s: N must be a multiple of 8 (got %lld)", name, (long long)N);
  if (M * N >= (1ll << 40) || M >= (1ll << 31) || N >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: an output of 2^40 elements is not supported", name);
  return QAMD_OK;
}
// ... of matmul_mx{f4,f8}_bf16_tn (ebits 4 / 8)
inline int mx_check(const char* name, int ebits, const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, const void* D,
                    int64_t M, int64_t N, int64_t K) {
  return gemm_check(name, 32, ebits == 4 ? 128 : 32, true, A, B, A_sf, B_sf, alpha, D, M, N, K);
}

// matmul_nvf4_bf16_tn: f(r0, c0, m, n, launch) for the planned launch of every range.  A ranged call runs without scratch (avail: bytes of the caller's scratch, 0: none).
template <class F>
int nv_for_each_launch(const char* name, int64_t M, int64_t N, int64_t K, int64_t avail, int cus, F&& f) {
  return for_each_range(name, M, N, K / 2, 256, [&](int64_t r0, int64_t c0, int64_t m, int64_t n) -> int {
    return f(r0, c0, m, n, qamd::nvf4_launch_plan(opt_nvf4_variant(), m, n, K, cus, (m == M && n == N) ? avail : 0, opt_deepp_grid()));   // (the lab's "deepp_grid": the forced persistent kernel, variant 42)
  });
}

// EBITS: 4 = MXFP4, 8 = MXFP8 (TN); a_fmt (MXFP8 only): QAMD_FP8_E4M3 / QAMD_FP8_E5M2 element format of A
template <int EBITS>
int gemm_mx(const char* name, const void* A, const void* B, const void* A_sf, const void* B_sf,
            const float* alpha, void* D, int64_t M, int64_t N, int64_t K, void* stream, void* ws = nullptr, int64_t ws_bytes = 0, int a_fmt = 0) {
  if (int rc = mx_check(name, EBITS, A, B, A_sf, B_sf, alpha, D, M, N, K)) return rc;
  const MxArgs x{A, B, A_sf, B_sf, alpha, D, K, N, EBITS, false};
  return for_each_range(name, M, N, K * EBITS / 8, 256, [&](int64_t r0, int64_t c0, int64_t m, int64_t n) -> int {
    const MxPlan pl = mx_plan<EBITS>(a_fmt, m, n, K, N, ws ? ws_bytes : 0, chip_cus());
    for (int i = 0; i < pl.n; ++i)
      if (int rc = mx_launch<EBITS>(name, pl.l[i], mx_params(x, r0, c0 + pl.l[i].c0, m, pl.l[i].n), ws, a_fmt, (hipStream_t)stream)) return rc;
    return QAMD_OK;
  });
}

// debug entries: plan(m, n) of every range; out[3 i .. 3 i + 2] = {variant, N of the launch, K splits} of launch i (the first min(cap, 8)); returns the launch count
template <class P>
int debug_plan(const char* name, int64_t M, int64_t N, int64_t rowbytes, int gran, int* out, int cap, P&& plan) {
  int cnt = 0;
  const int rc = for_each_range(name, M, N, rowbytes, gran, [&](int64_t, int64_t, int64_t m, int64_t n) {
    const MxPlan pl = plan(m, n);
    for (int i = 0; i < pl.n; ++i, ++cnt)
      if (cnt < 8 && cnt < cap) { out[3 * cnt] = pl.l[i].variant; out[3 * cnt + 1] = (int)pl.l[i].n; out[3 * cnt + 2] = pl.l[i].splits; }
    return QAMD_OK;
  });
  return rc == QAMD_OK ? cnt : -1;
}

#endif   // QAMD_DEF(1)

// One rotation switch for the rotate + quantize family.  KIND picks the __global__ wrapper (quantize.hip.h): the plain quantizer, the gated one (act = silu(gate) * up
// computed in the tile loads) or the gathering one (the tile loads go through a row index).  BLK: scales written in the to_blocked() layout.
// The _GSCALE kinds are the gated and the gathering quantizer with one global scale per expert (quantize.hip.h, GSCALE): NV abs-max with flat scales and nothing else.
enum QuantKind { QK_PLAIN, QK_GATED, QK_GATHER, QK_GATED_GSCALE, QK_GATHER_GSCALE };

// FMT: QF_E2M1, or QF_E4M3 / QF_E5M2 for the MXFP8 quantizers (MX abs-max; plain, gated or gathering) -- their own three __global__ wrappers --, or QF_E2M3 for the
// MXFP6 quantizers (plain or gathering, flat scales) -- their own two.
template <int KIND, int R, bool NV, int METHOD, bool MASK, bool BLK, int FMT = QF_E2M1>
int launch_quant(const QuantParams& p, hipStream_t s, int grid) {
  static_assert((KIND != QK_GATED_GSCALE && KIND != QK_GATHER_GSCALE) || (NV && METHOD == METHOD_ABSMAX && !MASK && !BLK), "per-expert global scales: NV abs-max, flat scales");
  static_assert(FMT == QF_E2M1 || (KIND == QK_PLAIN || KIND == QK_GATED || KIND == QK_GATHER), "MXFP8: plain, gated or gathering");
  static_assert(FMT != QF_E2M3 || (!BLK && (KIND == QK_PLAIN || KIND == QK_GATHER)), "MXFP6: plain or gathering, flat scales");
  if constexpr (FMT == QF_E2M3 && KIND == QK_GATHER) {
    hipLaunchKernelGGL((fused_gather_quantize_mxf6_kernel<R>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_gather_quantize_mxf6_kernel");
  } else if constexpr (FMT == QF_E2M3) {
    hipLaunchKernelGGL((fused_quantize_mxf6_kernel<R>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_quantize_mxf6_kernel");
  } else if constexpr (FMT != QF_E2M1 && KIND == QK_GATED) {
    hipLaunchKernelGGL((fused_silu_mul_quantize_mxf8_kernel<R, FMT, BLK>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_silu_mul_quantize_mxf8_kernel");
  } else if constexpr (FMT != QF_E2M1 && KIND == QK_GATHER) {
    hipLaunchKernelGGL((fused_gather_quantize_mxf8_kernel<R, FMT>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_gather_quantize_mxf8_kernel");
  } else if constexpr (FMT != QF_E2M1) {
    hipLaunchKernelGGL((fused_quantize_mxf8_kernel<R, FMT, BLK>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_quantize_mxf8_kernel");
  } else if constexpr (KIND == QK_GATED_GSCALE) {
    hipLaunchKernelGGL((fused_silu_mul_quantize_gscale_kernel<R>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_silu_mul_quantize_gscale_kernel");
  } else if constexpr (KIND == QK_GATHER_GSCALE) {
    hipLaunchKernelGGL((fused_gather_quantize_gscale_kernel<R>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_gather_quantize_gscale_kernel");
  } else if constexpr (KIND == QK_GATED) {
    hipLaunchKernelGGL((fused_silu_mul_quantize_kernel<R, NV, METHOD, BLK>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_silu_mul_quantize_kernel");
  } else if constexpr (KIND == QK_GATHER) {
    hipLaunchKernelGGL((fused_gather_quantize_kernel<R, NV, METHOD>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_gather_quantize_kernel");
  } else {
#if QAMD_BENCH
    // lab only, and deliberately on the plain kernels only: the software e2m1 encoder exists to be compared with the hardware convert, and the plain kernels are where
    // that comparison is made -- the gated and the gathering wrappers are instantiated with the hardware convert alone
    if (!opt_hw_fp4()) hipLaunchKernelGGL((fused_quantize_kernel<R, NV, METHOD, MASK, false, BLK>), dim3(grid), dim3(256), 0, s, p);
    else
#endif
    hipLaunchKernelGGL((fused_quantize_kernel<R, NV, METHOD, MASK, true, BLK>), dim3(grid), dim3(256), 0, s, p);
    return check_launch("fused_quantize_kernel");
  }
}

template <int KIND, bool NV, int METHOD, bool MASK, bool BLK, int FMT = QF_E2M1>
int dispatch_quant(int rot, const QuantParams& p, hipStream_t s, int grid, const char* name) {
  static_assert(!MASK || (KIND == QK_PLAIN && !NV && METHOD == METHOD_QUEST), "the clip mask exists for the plain MX quest quantizer only");
  static_assert(FMT == QF_E2M1 || (!NV && METHOD == METHOD_ABSMAX && !MASK), "MXFP8: MX scales, abs-max, no clip mask");
  static_assert(!BLK || (KIND != QK_GATHER && KIND != QK_GATED_GSCALE && KIND != QK_GATHER_GSCALE), "the gathering and the grouped-scale quantizers write flat scales only");
  switch (rot) {
    case 16:
      if constexpr (NV) return launch_quant<KIND, 16, NV, METHOD, false, BLK>(p, s, grid);
      break;
    case 32: return launch_quant<KIND, 32, NV, METHOD, MASK, BLK, FMT>(p, s, grid);
    case 64:
      if constexpr (!MASK) return launch_quant<KIND, 64, NV, METHOD, false, BLK, FMT>(p, s, grid);
      break;
    case 128:
      if constexpr (!MASK) return launch_quant<KIND, 128, NV, METHOD, false, BLK, FMT>(p, s, grid);
      break;
  }
  if (MASK) return fail(QAMD_ERR_INVALID, "%s: Unsupported rotation size %d; expected 32.", name, rot);
  return fail(QAMD_ERR_INVALID, "%s: Unsupported rotation size %d; expected %s32, 64, or 128.", name, rot, NV ? "16, " : "");
}

// every instantiation select_quant() can reach, and no other: defined in unit 5 (build.py gives that unit the VGPR-form MFMA flag), declared elsewhere
#if QAMD_TU != 0
#if QAMD_TU == 5
#define QAMD_QUANT_INST(...) template int dispatch_quant<__VA_ARGS__>(int, const QuantParams&, hipStream_t, int, const char*);
#else
#define QAMD_QUANT_INST(...) extern template int dispatch_quant<__VA_ARGS__>(int, const QuantParams&, hipStream_t, int, const char*);
#endif
#define QAMD_QUANT_FORMATS(KIND_, BLK_) \
  QAMD_QUANT_INST(KIND_, false, METHOD_QUEST, false, BLK_) QAMD_QUANT_INST(KIND_, false, METHOD_ABSMAX, false, BLK_) \
  QAMD_QUANT_INST(KIND_, true, METHOD_QUEST, false, BLK_) QAMD_QUANT_INST(KIND_, true, METHOD_ABSMAX, false, BLK_)
QAMD_QUANT_FORMATS(QK_PLAIN, false)
QAMD_QUANT_FORMATS(QK_PLAIN, true)
QAMD_QUANT_INST(QK_PLAIN, false, METHOD_QUEST, true, false)
QAMD_QUANT_INST(QK_PLAIN, false, METHOD_QUEST, true, true)
QAMD_QUANT_FORMATS(QK_GATED, false)
QAMD_QUANT_FORMATS(QK_GATED, true)
QAMD_QUANT_FORMATS(QK_GATHER, false)
QAMD_QUANT_INST(QK_GATED_GSCALE, true, METHOD_ABSMAX, false, false)
QAMD_QUANT_INST(QK_GATHER_GSCALE, true, METHOD_ABSMAX, false, false)
// MXFP8 (x R = 32, 64, 128 each): plain flat and blocked x e4m3, e5m2; gathering x e4m3, e5m2; gated flat and blocked x e4m3 (a forward activation has no use for e5m2)
QAMD_QUANT_INST(QK_PLAIN, false, METHOD_ABSMAX, false, false, QF_E4M3) QAMD_QUANT_INST(QK_PLAIN, false, METHOD_ABSMAX, false, false, QF_E5M2)
QAMD_QUANT_INST(QK_PLAIN, false, METHOD_ABSMAX, false, true, QF_E4M3) QAMD_QUANT_INST(QK_PLAIN, false, METHOD_ABSMAX, false, true, QF_E5M2)
QAMD_QUANT_INST(QK_GATHER, false, METHOD_ABSMAX, false, false, QF_E4M3) QAMD_QUANT_INST(QK_GATHER, false, METHOD_ABSMAX, false, false, QF_E5M2)
QAMD_QUANT_INST(QK_GATED, false, METHOD_ABSMAX, false, false, QF_E4M3) QAMD_QUANT_INST(QK_GATED, false, METHOD_ABSMAX, false, true, QF_E4M3)
// MXFP6 (x R = 32, 64, 128 each): plain and gathering, flat scales
QAMD_QUANT_INST(QK_PLAIN, false, METHOD_ABSMAX, false, false, QF_E2M3) QAMD_QUANT_INST(QK_GATHER, false, METHOD_ABSMAX, false, false, QF_E2M3)
#undef QAMD_QUANT_FORMATS
#undef QAMD_QUANT_INST
#endif

// backward_t_bf16 / backward_qt_bf16 kernels live in unit 5 with the other rotation quantizers (MFMA results straight in VGPRs: a
// v_accvgpr_read per accumulator register is 32 more VALU issues per tile).  Launches what stream_launch_plan planned (quartet_bwd.hip.h: STREAM_FORMS): one arm per
// (form, op, e2m1 encoder), each naming one instantiation; the software encoder (!hw) is lab-only.  A form this build holds no kernel for is an error.
int launch_bwd_quant(const char* name, const BwdTParams& p, bool qt, bool hw, const StreamLaunch& l, hipStream_t s);
#if QAMD_DEF(5)
int launch_bwd_quant(const char* name, const BwdTParams& p, bool qt, bool hw, const StreamLaunch& l, hipStream_t s) {
  auto go = [&](auto kern, const char* what) { hipLaunchKernelGGL(kern, dim3((unsigned)l.grid), dim3(l.threads), 0, s, p); return check_launch(what); };
  constexpr auto arm = [](int form, bool qt_, bool hw_) { return form * 4 + qt_ * 2 + hw_; };   constexpr bool T = false, QT = true, SW = false, HW = true;
  switch (arm(l.form, qt, hw)) {
    case arm(BWD_ROUND3, T, HW): return go(bwd_quant_t_kernel<false, true>, "bwd_quant_t_kernel");   case arm(BWD_ROUND3, QT, HW): return go(bwd_quant_t_kernel<true, true>, "bwd_quant_t_kernel");
    case arm(BWD_WAVE8, T, HW): return go(bwd_quant_tw_kernel<false, true, 8>, "bwd_quant_tw_kernel");
    case arm(BWD_WAVE4, QT, HW): return go(bwd_quant_tw_kernel<true, true, 4>, "bwd_quant_tw_kernel");
    case arm(QT_RING, QT, HW): return go(bwd_qt_ring_kernel<true, 4, 3, false>, "bwd_qt_ring_kernel");
#if QAMD_BENCH   // the other op's unit size, [r6] BWD_WAVE2 (latency against write efficiency at small inputs), the software encoder, the whole-line lab forms
    case arm(BWD_WAVE8, QT, HW): return go(bwd_quant_tw_kernel<true, true, 8>, "bwd_quant_tw_kernel");
    case arm(BWD_WAVE4, T, HW): return go(bwd_quant_tw_kernel<false, true, 4>, "bwd_quant_tw_kernel");
    case arm(BWD_WAVE2, T, HW): return go(bwd_quant_tw_kernel<false, true, 2>, "bwd_quant_tw_kernel");   case arm(BWD_WAVE2, QT, HW): return go(bwd_quant_tw_kernel<true, true, 2>, "bwd_quant_tw_kernel");
    case arm(BWD_ROUND3, T, SW): return go(bwd_quant_t_kernel<false, false>, "bwd_quant_t_kernel");   case arm(BWD_ROUND3, QT, SW): return go(bwd_quant_t_kernel<true, false>, "bwd_quant_t_kernel");
    case arm(BWD_WAVE8, T, SW): return go(bwd_quant_tw_kernel<false, false, 8>, "bwd_quant_tw_kernel");   case arm(BWD_WAVE8, QT, SW): return go(bwd_quant_tw_kernel<true, false, 8>, "bwd_quant_tw_kernel");
    case arm(BWD_WAVE4, T, SW): return go(bwd_quant_tw_kernel<false, false, 4>, "bwd_quant_tw_kernel");   case arm(BWD_WAVE4, QT, SW): return go(bwd_quant_tw_kernel<true, false, 4>, "bwd_quant_tw_kernel");
    case arm(QT_RING, QT, SW): return go(bwd_qt_ring_kernel<false, 4, 3, false>, "bwd_qt_ring_kernel");
    case arm(QT_PANEL, QT, SW): return go(bwd_qt_panel_kernel<false>, "bwd_qt_panel_kernel");   case arm(QT_PANEL, QT, HW): return go(bwd_qt_panel_kernel<true>, "bwd_qt_panel_kernel");
    case arm(QT_RING8_XR, QT, HW): return go(bwd_qt_ring_kernel<true, 8, 4, true>, "bwd_qt_ring_kernel");   case arm(QT_RING8, QT, HW): return go(bwd_qt_ring_kernel<true, 8, 4, false>, "bwd_qt_ring_kernel");
    case arm(QT_RING4_XR, QT, HW): return go(bwd_qt_ring_kernel<true, 4, 3, true>, "bwd_qt_ring_kernel");
#endif
  }
  return fail(QAMD_ERR_INVALID, "%s: this build holds no kernel for form %d%s", name, l.form, hw ? "" : " with the software encoder");
}
#endif

// The clamped-SwiGLU kernels and moe_combine's bias form (quantize.hip.h) live in unit 5 with the other quantizers: the fused arm for R = 32 / 64 x method x
// bias, its e4m3 form for R = 32 / 64 x bias, the streaming activation with and without a bias, the combine.  The C entries (unit 1) have checked everything; these only pick the instantiation.
int launch_swiglu_oai_quant(int rot, int method, bool bias, const QuantParams& p, hipStream_t s, int grid);
int launch_swiglu_oai_quant_mxf8(int rot, bool bias, const QuantParams& p, hipStream_t s, int grid);   // (the e4m3 form: abs-max only)
int launch_swiglu_oai_stream(const SwigluOaiParams& p, const RowStreamLaunch& l, hipStream_t s);
int launch_moe_combine_bias(const MoeCombineBiasParams& p, const RowStreamLaunch& l, hipStream_t s);
#if QAMD_DEF(5)
int launch_swiglu_oai_quant(int rot, int method, bool bias, const QuantParams& p, hipStream_t s, int grid) {
  auto go = [&](auto r_, auto m_) {
    using RT = decltype(r_); using M = decltype(m_);
    if (bias) hipLaunchKernelGGL((fused_swiglu_oai_quantize_kernel<RT::value, M::value, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fused_swiglu_oai_quantize_kernel<RT::value, M::value, false>), dim3(grid), dim3(256), 0, s, p);
  };
  using Quest = std::integral_constant<int, METHOD_QUEST>; using AbsMax = std::integral_constant<int, METHOD_ABSMAX>;
  using R32 = std::integral_constant<int, 32>; using R64 = std::integral_constant<int, 64>;
  if (rot == 32) { if (method == QAMD_METHOD_QUEST) go(R32{}, Quest{}); else go(R32{}, AbsMax{}); }
  else { if (method == QAMD_METHOD_QUEST) go(R64{}, Quest{}); else go(R64{}, AbsMax{}); }
  return check_launch("fused_swiglu_oai_quantize_kernel");
}
int launch_swiglu_oai_quant_mxf8(int rot, bool bias, const QuantParams& p, hipStream_t s, int grid) {
  if (rot == 32) {
    if (bias) hipLaunchKernelGGL((fused_swiglu_oai_quantize_mxf8_kernel<32, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fused_swiglu_oai_quantize_mxf8_kernel<32, false>), dim3(grid), dim3(256), 0, s, p);
  } else {
    if (bias) hipLaunchKernelGGL((fused_swiglu_oai_quantize_mxf8_kernel<64, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((fused_swiglu_oai_quantize_mxf8_kernel<64, false>), dim3(grid), dim3(256), 0, s, p);
  }
  return check_launch("fused_swiglu_oai_quantize_mxf8_kernel");
}
int launch_swiglu_oai_stream(const SwigluOaiParams& p, const RowStreamLaunch& l, hipStream_t s) {
  if (p.bias) hipLaunchKernelGGL(swiglu_oai_mul_bf16_kernel<true>, dim3(l.grid), dim3(l.threads), 0, s, p);
  else hipLaunchKernelGGL(swiglu_oai_mul_bf16_kernel<false>, dim3(l.grid), dim3(l.threads), 0, s, p);
  return check_launch("swiglu_oai_mul_bf16_kernel");
}
int launch_moe_combine_bias(const MoeCombineBiasParams& p, const RowStreamLaunch& l, hipStream_t s) {
  hipLaunchKernelGGL(moe_combine_bias_bf16_kernel<0>, dim3(l.grid), dim3(l.threads), 0, s, p);
  return check_launch("moe_combine_bias_bf16_kernel");
}
#endif

#if QAMD_DEF(1)
int quant_grid(int ntiles, int rot) {
  // 4 waves per workgroup, one 32-row tile per wave per trip.  Small rotations are pure streaming: as many waves as
  // fit (8 workgroups per CU; 8192^2 NV runs at 6.26 TB/s).  R = 128 tiles are 8 KiB with 32 MFMAs each: fewer, longer
  // waves let the software pipeline (next tile's loads in flight during this tile's MFMAs) overlap (13.2 vs 14.6 us).
  // ([r4] One 12-wave workgroup per CU sharing one H image -- three waves per SIMD instead of two -- measured slower: 4096^2 8.9 -> 10.8 us warm.)
  int per_cu = opt_quant_wg_per_cu();
  if (per_cu <= 0) per_cu = rot >= 128 ? 2 : (rot >= 64 ? 4 : 8);
  int g = (ntiles + 3) / 4;
  const int cap = chip_cus() * per_cu;
  return g < 1 ? 1 : (g > cap ? cap : g);
}

// blocked-scale quantizers: the kernel also zero-fills the padding of the blocked layout (up to 127 rows x all column tiles); a one-row
// input would leave that to a single workgroup (M = 1, K = 4096: 14.4 us for the 2-launch linear layer against 9.1 us with 3 launches)
int blocked_pad_grid(int grid, int sf_rows, int sf_cols) {
  const int64_t prow = cdiv(sf_rows, 128) * 128, cb = cdiv(sf_cols, 4);
  const int64_t stores = (prow - sf_rows) * cb + (int64_t)sf_rows * (cb * 4 - sf_cols);
  const int64_t want = std::min<int64_t>(cdiv(stores, 256), chip_cus());
  return (int)std::max<int64_t>(grid, want);
}

// ---- the rotate + quantize family (plain, gated, gathering; MX and NV): every check and the launch set-up written once; each C entry calls them in its own order ----
inline int quant_check_rot(const char* name, const QuantFormat& f, int rot, bool mask = false) {
  if (f.has_rot(rot)) return QAMD_OK;   // (a mask with R = 64 / 128 passes here and is refused by dispatch_quant, after the entry's other checks)
  return fail(QAMD_ERR_INVALID, "%s: Unsupported rotation size %d; expected %s.", name, rot, mask ? "32" : f.rots);
}

inline int quant_check_method(const char* name, int method) {
  if (method == QAMD_METHOD_QUEST || method == QAMD_METHOD_ABSMAX) return QAMD_OK;
  return fail(QAMD_ERR_INVALID, "%s: invalid method %d", name, method);
}

// the MXFP8 entries have no method (abs-max is the only one): the code format stands in its place in every chain.  fmt is the C ABI's (the GEMMs' _fmt convention);
// the kernels' FMT is fmt + 1.  e4m3_only: the gated form.
inline int quant_check_how(const char* name, const QuantFormat& f, int method, int fmt, bool e4m3_only = false) {
  if (!f.fp8) return quant_check_method(name, method);
  if (f.fp6) return QAMD_OK;   // MXFP6: one code format, abs-max only -- nothing to choose
  if (fmt == QAMD_FP8_E4M3 || (fmt == QAMD_FP8_E5M2 && !e4m3_only)) return QAMD_OK;
  return fail(QAMD_ERR_INVALID, "%s: invalid fmt %d; expected %s", name, fmt, e4m3_only ? "0 (e4m3)" : "0 (e4m3) or 1 (e5m2)");
}

// (rot >= 64 stages H with 16-byte vector loads, quantize.hip.h: an offset view of a larger tensor may be 2-byte aligned only -- rejected rather than left to
//  the device's unaligned-access mode; torch allocations are 256-byte aligned)
inline int quant_check_h(const char* name, int rot, const void* h) {
  if (rot < 64 || (uintptr_t)h % 16 == 0) return QAMD_OK;
  return fail(QAMD_ERR_INVALID, "%s: the rotation matrix must be 16-byte aligned for rotation sizes >= 64", name);
}

inline int quant_rp(int rot) { return rot < 32 ? 32 : rot; }   // a tile is 32 rows of max(R, 32) elements: the unit of ntiles and of every row length

// numel elements in rows of k (k is read for blocked scales only); src_row / src_n: the gather index.  Fills ntiles, sf_rows, sf_cols and the index; returns the grid.
inline int quant_fill(QuantParams& p, const QuantFormat& f, int rot, int64_t numel, int64_t k, bool blocked, const int32_t* src_row = nullptr, int64_t src_n = 0) {
  p.numel = numel;
  p.ntiles = (int)cdiv(numel, (int64_t)quant_rp(rot) * 32);
  p.sf_rows = blocked ? (int)(numel / k) : 0; p.sf_cols = blocked ? (int)(k / f.group) : 0;
  p.src_row = src_row; p.src_n = (int)src_n;
  const int grid = quant_grid(p.ntiles, rot);
  return blocked ? blocked_pad_grid(grid, p.sf_rows, p.sf_cols) : grid;
}

// per-expert global scales (the *_nv_grouped entries): offs (e) = the grouped GEMMs' cumulative END rows, read by the kernel; the entry's global scale then has e floats
struct QuantGroups {
  const int32_t* offs;
  int64_t e;
};
static_assert(qamd::QUANT_MAX_E == qamd::GRP_MAX_E, "the quantizers take as many experts as the grouped GEMMs");

// the two checks a grouped entry adds behind its sibling's chain (a null offs joins the sibling's null-pointer check)
inline int quant_check_groups(const char* name, const QuantGroups& g) {
  if (g.e < 1 || g.e > qamd::QUANT_MAX_E) return fail(QAMD_ERR_INVALID, "%s: E must be in [1, %d] (got %lld)", name, qamd::QUANT_MAX_E, (long long)g.e);
  if ((uintptr_t)g.offs % 4) return fail(QAMD_ERR_INVALID, "%s: offs must be 4-byte aligned", name);
  return QAMD_OK;
}

// runtime (nv, method, mask, blocked) -> the dispatch_quant instantiation; the callers have checked method, and that a mask comes with MX + quest only
// fmt8: -1, or the C ABI's fmt of an MXFP8 entry (checked by quant_check_how): MX abs-max with e4m3 / e5m2 codes
template <int KIND>
int select_quant(bool nv, int method, bool mask, bool blocked, int rot, const QuantParams& p, hipStream_t s, int grid, const char* name, int fmt8 = -1) {
  if (fmt8 == QF_E2M3 - 1) {   // MXFP6 (the entries pass the kernels' FMT - 1, as the MXFP8 ones do): plain or gathering, flat scales
    if constexpr (KIND == QK_PLAIN || KIND == QK_GATHER) return dispatch_quant<KIND, false, METHOD_ABSMAX, false, false, QF_E2M3>(rot, p, s, grid, name);
    else return fail(QAMD_ERR_INVALID, "%s: no MXFP6 form", name);
  }
  if (fmt8 >= 0) {
    auto go8 = [&](auto fmt_) {
      using F = decltype(fmt_);
      if constexpr (KIND != QK_GATHER)
        if (blocked) return dispatch_quant<KIND, false, METHOD_ABSMAX, false, true, F::value>(rot, p, s, grid, name);
      return dispatch_quant<KIND, false, METHOD_ABSMAX, false, false, F::value>(rot, p, s, grid, name);
    };
    if constexpr (KIND != QK_GATED)
      if (fmt8 == QAMD_FP8_E5M2) return go8(std::integral_constant<int, QF_E5M2>{});
    return go8(std::integral_constant<int, QF_E4M3>{});
  }
  auto go = [&](auto nv_, auto method_, auto mask_) {
    using NV = decltype(nv_); using M = decltype(method_); using K = decltype(mask_);
    if constexpr (KIND != QK_GATHER)
      if (blocked) return dispatch_quant<KIND, NV::value, M::value, K::value, true>(rot, p, s, grid, name);
    return dispatch_quant<KIND, NV::value, M::value, K::value, false>(rot, p, s, grid, name);
  };
  using Quest = std::integral_constant<int, METHOD_QUEST>; using AbsMax = std::integral_constant<int, METHOD_ABSMAX>;
  if constexpr (KIND == QK_PLAIN)
    if (mask) return go(std::false_type{}, Quest{}, std::true_type{});
  if (nv) return method == QAMD_METHOD_QUEST ? go(std::true_type{}, Quest{}, std::false_type{}) : go(std::true_type{}, AbsMax{}, std::false_type{});
  return method == QAMD_METHOD_QUEST ? go(std::false_type{}, Quest{}, std::false_type{}) : go(std::false_type{}, AbsMax{}, std::false_type{});
}

// the grouped-scale form of KIND (QK_GATED / QK_GATHER), NV with flat scales.  Quest never reads a global scale (quantize.hip.h, the NV Quest arm): it runs the
// single-scale kernel; abs-max runs the GSCALE kernel over p.offs / p.E.
template <int KIND>
int select_quant_grouped(int method, int rot, QuantParams& p, const QuantGroups& g, hipStream_t s, int grid, const char* name) {
  if (method == QAMD_METHOD_QUEST) return select_quant<KIND>(true, method, false, false, rot, p, s, grid, name);
  p.offs = g.offs; p.E = (int)g.e;
  return dispatch_quant<KIND == QK_GATED ? QK_GATED_GSCALE : QK_GATHER_GSCALE, true, METHOD_ABSMAX, false, false>(rot, p, s, grid, name);
}

#endif   // QAMD_DEF(1)

}  // namespace qamd_host

using namespace qamd_host;

#if QAMD_DEF(1)
// the library is built with -fvisibility=hidden: only the C ABI below is exported
#pragma GCC visibility push(default)
extern "C" {

int qutlass_amd_matmul_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K, void* stream) {
  return gemm_mx<4>("matmul_mxf4_bf16_tn", A, B, A_sf, B_sf, alpha, D, M, N, K, stream);
}

// the split-K scratch of the plan with unlimited scratch
int64_t qutlass_amd_gemm_splitk_workspace_bytes(int ebits, int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || (ebits != 4 && ebits != 8)) return 0;
  const int cus = chip_cus();
  int64_t need = (ebits == 4 ? mx_plan<4>(0, M, N, K, N, INT64_MAX, cus) : mx_plan<8>(0, M, N, K, N, INT64_MAX, cus)).ws;
#if QAMD_BENCH
  if (opt_gemm_variant() == 89) need = std::max<int64_t>(need, sk_ws_bytes(cus));   // lab: forced stream-K
  if (opt_splitk_force() > 1) need = std::max<int64_t>(need, splitk_ws_bytes(MXV_RING64, M, N, 8));   // lab: room for any forced tile x split
#endif
  return need;
}

int qutlass_amd_matmul_mxf4_bf16_tn_ws(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D,
                                       int64_t M, int64_t N, int64_t K, void* workspace, int64_t workspace_bytes, void* stream) {
  if (workspace && (uintptr_t)workspace % 16) return fail(QAMD_ERR_INVALID, "matmul_mxf4_bf16_tn: the workspace must be 16-byte aligned");   // v4f partials
  return gemm_mx<4>("matmul_mxf4_bf16_tn", A, B, A_sf, B_sf, alpha, D, M, N, K, stream, workspace, workspace_bytes);
}

int qutlass_amd_matmul_mxf8_bf16_tn_ws(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D,
                                       int64_t M, int64_t N, int64_t K, void* workspace, int64_t workspace_bytes, void* stream) {
  if (workspace && (uintptr_t)workspace % 16) return fail(QAMD_ERR_INVALID, "matmul_mxf8_bf16_tn: the workspace must be 16-byte aligned");   // v4f partials
  return gemm_mx<8>("matmul_mxf8_bf16_tn", A, B, A_sf, B_sf, alpha, D, M, N, K, stream, workspace, workspace_bytes);
}

// the argument checks of matmul_ada_mxf4_bf16_tn
static int ada_check(const char* name, const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, const void* D, int64_t M, int64_t N,
                     int64_t K) {
  if (!A || !B || !A_sf || !B_sf || !alpha || !D) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (M <= 0 || N <= 0) return fail(QAMD_ERR_INVALID, "%s: M and N must be positive (got M=%lld N=%lld)", name, (long long)M, (long long)N);
  if (K < 128 || K % 128) return fail(QAMD_ERR_INVALID, "%s: K must be a positive multiple of 128 (got %lld)", name, (long long)K);
  if (N % 8) return fail(QAMD_ERR_INVALID, "%s: N must be a multiple of 8 (got %lld)", name, (long long)N);
  if (M >= (1ll << 31) || N >= (1ll << 31) || M * N >= (1ll << 40)) return fail(QAMD_ERR_INVALID, "%s: an output of 2^40 elements is not supported", name);
  return QAMD_OK;
}

// the plan of each range (ada_plan; operands of >= 2 GiB: ranges of whole 64-row / 64-column tiles) on the row-major-scale kernels
int qutlass_amd_matmul_ada_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                        const float* alpha, void* D, int64_t M, int64_t N, int64_t K, void* stream) {
  const char* name = "matmul_ada_mxf4_bf16_tn";
  if (int rc = ada_check(name, A, B, A_sf, B_sf, alpha, D, M, N, K)) return rc;
  const MxArgs x{A, B, A_sf, B_sf, alpha, D, K, N, 4, true};
  const hipStream_t s = (hipStream_t)stream;
  return for_each_range(name, M, N, K / 2, 64, [&](int64_t r0, int64_t c0, int64_t m, int64_t n) -> int {
    const GemmParams p = mx_params(x, r0, c0, m, n);
    const int v = ada_plan(m, n, K, chip_cus());
#if QAMD_BENCH
    if (v == 178) return launch_gemm<GemmCfg<64, 64, 2, 2, 4, false, 0, 3>, 8>(p, s);   // round-1 ring schedule
#endif
    return dispatch_variant<4, 0, true>(v, p, s, name);
  });
}

int qutlass_amd_grouped_matmul_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                                            const int32_t* offs, void* D, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  constexpr const GroupedFormat& F = GRP_MXF4;
  if (int rc = grouped_check(F, F.name, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E)) return rc;
  if (M == 0) return QAMD_OK;
  GroupedParams q;
  grouped_fill(q, F, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E);
  grouped_mx_defaults(q);
  const int v = grouped_form(F, grouped_plan, M, N, K, E);
  return launch_grouped_mx<GRP_MXF4, GroupedRingCfg>(v, q, (hipStream_t)stream);   // (the ring form: matmul_ada_mxf4_bf16_tn's ring tiles)
}

int qutlass_amd_grouped_matmul_mxf8_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                                            const int32_t* offs, void* D, int64_t M, int64_t N, int64_t K, int64_t E, int a_format, void* stream) {
  constexpr const GroupedFormat& F = GRP_MXF8;
  if (int rc = grouped_check(F, F.name, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E)) return rc;
  if (a_format != QAMD_FP8_E4M3 && a_format != QAMD_FP8_E5M2) return fail(QAMD_ERR_INVALID, "%s: invalid a_format %d", F.name, a_format);
  if (M == 0) return QAMD_OK;
  GroupedParams q;
  grouped_fill(q, F, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E);
  grouped_mx_defaults(q);
  const int v = grouped_form(F, grouped8_plan, M, N, K, E);
  hipStream_t s = (hipStream_t)stream;
  return a_format == QAMD_FP8_E5M2 ? launch_grouped_mx<GRP_MXF8, GroupedRing8Cfg<1>, 1>(v, q, s) : launch_grouped_mx<GRP_MXF8, GroupedRing8Cfg<0>, 0>(v, q, s);
}

int qutlass_amd_grouped_matmul_mxf8_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                                                 const int32_t* offs, void* D, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  constexpr const GroupedFormat& F = GRP_MXF8_MXF4;
  if (int rc = grouped_check(F, F.name, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E)) return rc;
  if (M == 0) return QAMD_OK;
  GroupedParams q;
  grouped_fill(q, F, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E);
  grouped_mx_defaults(q);
  return launch_grouped_w4a8(grouped_form(F, grouped_w4a8_plan, M, N, K, E), q, (hipStream_t)stream);
}

// W4A6: A (M, 3K/4) packed e2m3 codes, everything else as W4A8
int qutlass_amd_grouped_matmul_mxf6_mxf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                                                 const int32_t* offs, void* D, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  constexpr const GroupedFormat& F = GRP_MXF6_MXF4;
  if (int rc = grouped_check(F, F.name, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E)) return rc;
  if ((uintptr_t)A % 16) return fail(QAMD_ERR_INVALID, "%s: A must be 16-byte aligned", F.name);   // 16-byte LDS-DMA chunks at a 3K/4-byte row pitch
  if (M == 0) return QAMD_OK;
  GroupedParams q;
  grouped_fill(q, F, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E);
  grouped_mx_defaults(q);
  return launch_grouped_w4a6(grouped_form(F, grouped_w4a6_plan, M, N, K, E), q, (hipStream_t)stream);
}

// W4A16: A (M, K) bf16 without scales; src_row (M,) int32 or null -- with it A is the unsorted (T, K) tokens and sorted row r reads A[src_row[r]]
int qutlass_amd_grouped_matmul_bf16_mxf4_bf16_tn(const void* A, const void* B, const void* B_sf, const float* alpha, int64_t n_alpha, const int32_t* offs,
                                                 const int32_t* src_row, int64_t T, void* D, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  constexpr const GroupedFormat& F = GRP_BF16_MXF4;
  if (int rc = grouped_check(F, F.name, A, B, /* no A scales */ A, B_sf, alpha, n_alpha, offs, D, M, N, K, E)) return rc;
  if (src_row) {   // the descriptor spans all of A: T rows of 2 K bytes
    if (T < 0) return fail(QAMD_ERR_INVALID, "%s: T must be >= 0 (got %lld)", F.name, (long long)T);
    if (T >= ((1ll << 31) - 1) / F.row_bytes(K) + 1) return fail(QAMD_ERR_INVALID, "%s: the gathered token matrix (T * 2K bytes, T=%lld K=%lld) must stay below 2 GiB", F.name, (long long)T, (long long)K);
  }
  if (M == 0) return QAMD_OK;
  W4A16Params q;
  grouped_fill(q, F, A, B, nullptr, B_sf, alpha, n_alpha, offs, D, M, N, K, E);
  q.sfa_bytes = 0;
  grouped_mx_defaults(q);
  q.src_row = src_row; q.T = src_row ? (int)T : 0;
  return launch_grouped_w4a16(grouped_form(F, grouped_w4a16_plan, M, N, K, E), q, (hipStream_t)stream);
}

// ---- grouped NVFP4 GEMM (gemm_nvf4.hip.h, gemm_nvf4_os.hip.h; the kernels live in the NVFP4 unit: launch_nvf4_grouped) -----------------------------------------------
// Forms: 598 = 32x32 tiles of the wave-owned kernel, 599 = its 64x32 tiles, 600 = 64x64 tiles, 601 = 128x128 tiles of gemm_nvf4_kernel with row-major scale fetch.
// Measured on the decode and prefill shapes of Qwen3-30B-A3B and Mixtral-8x7B and on token counts between them (profiles/calib_grouped_nvf4_r7.txt; these are not the MX
// thresholds).  NVFP4 is bound by dequantisation instructions per MFMA, so the larger tile wins as soon as the groups fill it: at a mean of 64 rows per group and
// beyond 601 leads (Qwen3 gate/up, 64 rows: 90.6 us against 111.8 for 600; Mixtral gate/up, 1024 rows: 1823 against 2791), at 48 rows and below 600 does (Qwen3 gate/up,
// 48 rows: 84.1 against 94.2; 4 rows: 70.9 against 82.7 and 84.2 for 598; Qwen3 down, K = 768, 4 rows: 44.1 against 50.3 and 105.7 for 598).  The wave-owned kernel
// leads only where few 64x64 tiles would each walk a long K: at most 16 rows per group and K >= 8192 (Mixtral down, K = 14336, 16 rows: 598 takes 69.6 / 83.1 us
// uniform / skewed against 82.8 / 115.5 for 600; cut to K = 8192: 48.6 / 58.6 against 49.5 / 68.8; cut to K = 6144 the two cross, 42.7 / 49.7 against 38.1 / 53.0,
// and at K = 4096 600 leads, Mixtral gate/up 166.0 / 181.6 against 215.3 / 238.4); at 32 rows per group 600 leads at every K measured.  599 never leads.
// N and the CU count are arguments so that a rule re-taken from more measurements can use them.
inline int grouped_nv_plan(int64_t M, int64_t N, int64_t K, int64_t E, int cus) {
  (void)N; (void)cus;
  if (M <= 16 * E && K >= 8192) return 598;
  return M <= 48 * E ? 600 : 601;
}

int qutlass_amd_grouped_matmul_nvf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, int64_t n_alpha,
                                            const int32_t* offs, void* D, int64_t M, int64_t N, int64_t K, int64_t E, void* stream) {
  constexpr const GroupedFormat& F = GRP_NVF4;
  if (int rc = grouped_check(F, F.name, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E)) return rc;
  if (M == 0) return QAMD_OK;
  const int v = grouped_form(F, grouped_nv_plan, M, N, K, E);
  qamd::NvGroupedParams q{};
  grouped_fill(q, F, A, B, A_sf, B_sf, alpha, n_alpha, offs, D, M, N, K, E);
  if (launch_nvf4_grouped_host(q, (hipStream_t)stream, v)) return fail(QAMD_ERR_INVALID, "%s: unknown form %d", F.name, v);
  return check_launch(F.name);
}

int qutlass_amd_matmul_mxf8_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K, void* stream) {
  return gemm_mx<8>("matmul_mxf8_bf16_tn", A, B, A_sf, B_sf, alpha, D, M, N, K, stream);
}

// one rule for the launcher and the workspace query: the persistent kernel on the (K, M) operand wherever the TN op would
// pick the persistent 256x256 kernel for the whole problem (mx_plan auto rule); everything smaller goes through the
// byte-transpose pre-pass and the TN dispatch with its smaller tiles / split-K
// (operands of >= 2 GiB also take the pre-pass: the in-place path walks the (K, M) operand with 32-bit offsets k * M + m, which only a
//  per-K-chunk descriptor could extend; the (M, K) copy in the workspace then runs as row ranges of the TN dispatch, gemm_mx)
static bool mxf8_nn_is_fused(int64_t M, int64_t N, int64_t K) {
  return M > 64 && N > 64 && N < (1ll << 22) && cdiv(M, 256) * cdiv(N, 256) >= chip_cus() * 3 / 4 && M * K < (1ll << 31) && N * K < (1ll << 31);
}

int64_t qutlass_amd_mxf8_nn_workspace_bytes(int64_t M, int64_t K) { return (M > 0 && K > 0) ? M * K : 0; }
int64_t qutlass_amd_mxf8_nn_workspace_bytes_for(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return (opt_gemm_variant() == 0 && mxf8_nn_is_fused(M, N, K)) ? 0 : M * K;
}

static int mxf8_nn_impl(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D, int64_t M, int64_t N,
                        int64_t K, int a_fmt, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "matmul_mxf8_bf16_nn";
  if (!A) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (M <= 0 || N <= 0) return fail(QAMD_ERR_INVALID, "%s: M and N must be positive (got M=%lld N=%lld)", name, (long long)M, (long long)N);
  if (K < 32 || K % 32) return fail(QAMD_ERR_INVALID, "%s: K must be a positive multiple of 32 (got %lld)", name, (long long)K);
  if (M % 16) return fail(QAMD_ERR_INVALID, "%s: M must be a multiple of 16 for the (K, M) operand (got %lld)", name, (long long)M);
  if (M >= (1ll << 31) || K >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: tensor too large", name);
  // large problems: the persistent kernel reads A^T directly (no pre-pass, no workspace).  Lab library only: "gemm_variant"
  // 63 forces it, 61 forces the per-tile fused kernel of round 1 (dword reads + v_perm byte transposes), 62 the pre-pass
  const int forced = opt_gemm_variant();
  const bool fused = (M * K < (1ll << 31) && N * K < (1ll << 31)) && (forced == 61 || (forced >= 63 && forced <= 66) || (forced == 0 && mxf8_nn_is_fused(M, N, K)));
  if (!fused) {
    if (!workspace) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
    if (workspace_bytes < M * K) return fail(QAMD_ERR_INVALID, "%s: workspace too small (%lld < %lld bytes)", name, (long long)workspace_bytes, (long long)(M * K));
  }
  if (fused) {
    if (!B || !A_sf || !B_sf || !alpha || !D) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
    if (N % 8) return fail(QAMD_ERR_INVALID, "%s: N must be a multiple of 8 (got %lld)", name, (long long)N);
    const GemmParams p = mx_params({A, B, A_sf, B_sf, alpha, D, K, N, 8, false}, 0, 0, M, N);   // (A is (K, M): M * K bytes all the same)
    if (a_fmt == 1) return launch_nn_fused_a5(p, (hipStream_t)stream, forced == 61);
#if QAMD_BENCH
    if (forced == 61) return launch_gemm<GemmCfg<256, 256, 2, 2, 8, true>, 6>(p, (hipStream_t)stream);
    // timing-only ablations (wrong results): 64 = A fetched with the TN addresses, 65 = A fragments read the TN way, 66 = both
    if (forced == 64) return launch_gemm_deepp8<GemmCfg<256, 256, 2, 2, 8, true>, true, 1>(p, (hipStream_t)stream);
    if (forced == 65) return launch_gemm_deepp8<GemmCfg<256, 256, 2, 2, 8, true>, true, 2>(p, (hipStream_t)stream);
    if (forced == 66) return launch_gemm_deepp8<GemmCfg<256, 256, 2, 2, 8, true>, true, 3>(p, (hipStream_t)stream);
#endif
    return launch_gemm_deepp8<GemmCfg<256, 256, 2, 2, 8, true>, true>(p, (hipStream_t)stream);
  }
  TransposeParams t;
  t.in = (const uint8_t*)A; t.out = (uint8_t*)workspace; t.K = (int)K; t.M = (int)M;
  hipLaunchKernelGGL(transpose_u8_kernel<>, dim3((unsigned)cdiv(M, 128), (unsigned)cdiv(K, 128)), dim3(256), 0, (hipStream_t)stream, t);
  if (int rc = check_launch("transpose_u8_kernel")) return rc;
  return gemm_mx<8>(name, workspace, B, A_sf, B_sf, alpha, D, M, N, K, stream, nullptr, 0, a_fmt);
}

int qutlass_amd_matmul_mxf8_bf16_nn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  return mxf8_nn_impl(A, B, A_sf, B_sf, alpha, D, M, N, K, QAMD_FP8_E4M3, workspace, workspace_bytes, stream);
}

static int check_fp8_formats(const char* name, int a_format, int b_format) {
  if (a_format != QAMD_FP8_E4M3 && a_format != QAMD_FP8_E5M2) return fail(QAMD_ERR_INVALID, "%s: invalid a_format %d", name, a_format);
  if (b_format != QAMD_FP8_E4M3) return fail(QAMD_ERR_INVALID, "%s: b_format must be QAMD_FP8_E4M3 (got %d)", name, b_format);
  return QAMD_OK;
}

int qutlass_amd_matmul_mxf8_bf16_tn_fmt(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D, int64_t M,
                                        int64_t N, int64_t K, int a_format, int b_format, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_fp8_formats("matmul_mxf8_bf16_tn", a_format, b_format)) return rc;
  return gemm_mx<8>("matmul_mxf8_bf16_tn", A, B, A_sf, B_sf, alpha, D, M, N, K, stream, workspace, workspace_bytes, a_format);
}

int qutlass_amd_matmul_mxf8_bf16_nn_fmt(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D, int64_t M,
                                        int64_t N, int64_t K, int a_format, int b_format, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_fp8_formats("matmul_mxf8_bf16_nn", a_format, b_format)) return rc;
  return mxf8_nn_impl(A, B, A_sf, B_sf, alpha, D, M, N, K, a_format, workspace, workspace_bytes, stream);
}

// matmul_nvf4_bf16_tn: the plan of each range (gemm_nvf4.hip.h nvf4_launch_plan; operands of >= 2 GiB: ranges of whole 256-row / 256-column tiles, as gemm_mx), its
// launch, then the reduce pass of a split.  ws: caller scratch (null: none)
static int nvf4_impl(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D, int64_t M, int64_t N,
                     int64_t K, void* stream, void* ws = nullptr, int64_t ws_bytes = 0) {
  const char* name = "matmul_nvf4_bf16_tn";
  if (int rc = gemm_check(name, 16, 32, false, A, B, A_sf, B_sf, alpha, D, M, N, K)) return rc;
  const MxArgs x{A, B, A_sf, B_sf, alpha, D, K, N, 4, false, 16};
  const hipStream_t s = (hipStream_t)stream;
  return nv_for_each_launch(name, M, N, K, ws ? ws_bytes : 0, chip_cus(), [&](int64_t r0, int64_t c0, int64_t m, int64_t n, const qamd::NvLaunch& l) -> int {
    NvGemmParams p = nv_params(x, r0, c0, m, n);
    if (l.ws > 0) p.ws = (float*)ws;
    if (launch_nvf4_host(l, p, s)) return fail(QAMD_ERR_INVALID, "%s: unknown nvf4_variant %d", name, opt_nvf4_variant());
    if (int rc = check_launch(name)) return rc;
    return l.splits > 1 ? splitk_reduce(name, l.splits, ws, p.D, alpha, p.M, p.N, p.ldd, s) : QAMD_OK;
  });
}

int qutlass_amd_matmul_nvf4_bf16_tn(const void* A, const void* B, const void* A_sf, const void* B_sf,
                                    const float* alpha, void* D, int64_t M, int64_t N, int64_t K, void* stream) {
  return nvf4_impl(A, B, A_sf, B_sf, alpha, D, M, N, K, stream);
}

// [r3] the scratch of the plan with unlimited scratch: bytes for the fp32 partials ws[splits][M][N] of the planned split, 0 when the shape does not split
// (256x256 tiles run the persistent kernel in balanced whole-tile rounds: no scratch; its stream-K form is lab-only, gemm_nvf4_pk.hip.h)
int64_t qutlass_amd_nvf4_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K < 32 || N % 4 || N * (K / 2) >= (1ll << 31) || M * (K / 2) >= (1ll << 31)) return 0;
#if QAMD_BENCH
  if (opt_nvf4_variant() >= 100) return 8 * M * N * 4;   // lab: room for any forced split
  if (opt_nvf4_variant() >= 42 && opt_nvf4_variant() <= 45) return qamd::nvpk_ws_bytes(chip_cus());   // lab: forced persistent kernel
#endif
  return qamd::nvf4_launch_plan(0, M, N, K, chip_cus(), INT64_MAX).ws;
}

int qutlass_amd_matmul_nvf4_bf16_tn_ws(const void* A, const void* B, const void* A_sf, const void* B_sf, const float* alpha, void* D, int64_t M,
                                       int64_t N, int64_t K, void* workspace, int64_t workspace_bytes, void* stream) {
  if (workspace_bytes < 0 || (workspace_bytes > 0 && !workspace)) return fail(QAMD_ERR_INVALID, "matmul_nvf4_bf16_tn: invalid workspace");
  if ((uintptr_t)workspace % 16) return fail(QAMD_ERR_INVALID, "matmul_nvf4_bf16_tn: the workspace must be 16-byte aligned");
  return nvf4_impl(A, B, A_sf, B_sf, alpha, D, M, N, K, stream, workspace, workspace_bytes);
}

// k: logical 2-D shape of x (rows of k elements) for the blocked-scale variants; k == 0: flat scales (the reference's contract).  MX: global_scale null; NV: out_mask null.
// MXFP8 (f.fp8): out_e2m1 takes numel code bytes, fmt8 is the entry's fmt and method is not read.
static int fused_quantize_impl(const char* name, const QuantFormat& f, const void* x, const void* h, int rot, int64_t numel, int64_t k, int method,
                               const float* global_scale, void* out_e2m1, void* out_sf, void* out_mask, void* stream, int fmt8 = -1) {
  if (!x || !h || !out_e2m1 || !out_sf || (f.nv && !global_scale)) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (int rc = quant_check_rot(name, f, rot, out_mask != nullptr)) return rc;
  if (numel <= 0 || numel % rot) return fail(QAMD_ERR_INVALID, "%s: A must be divisible by %d", name, rot);
  if (numel * 2 >= (1ll << 32)) return fail(QAMD_ERR_INVALID, "%s: more than 2^31 elements is not supported", name);
  if (int rc = quant_check_how(name, f, method, fmt8)) return rc;
  if (out_mask && method != QAMD_METHOD_QUEST) return fail(QAMD_ERR_INVALID, "%s: the clip mask is only defined for method quest", name);
  if (k && (k % quant_rp(rot) || numel % k))
    return fail(QAMD_ERR_INVALID, "%s: the row length %lld must be a multiple of %s%d and divide numel", name, (long long)k, f.row_unit, quant_rp(rot));
  if (int rc = quant_check_h(name, rot, h)) return rc;
  QuantParams p;
  p.x = (const uint16_t*)x; p.h = (const uint16_t*)h; p.out = (uint8_t*)out_e2m1; p.out_sf = (uint8_t*)out_sf;
  p.out_mask = (uint32_t*)out_mask; p.global_scale = global_scale;
  const int grid = quant_fill(p, f, rot, numel, k, k != 0);
  return select_quant<QK_PLAIN>(f.nv, method, out_mask != nullptr, k != 0, rot, p, (hipStream_t)stream, grid, name, f.fp8 ? fmt8 : -1);
}

int qutlass_amd_fused_quantize_mx(const void* x, const void* h, int rot, int64_t numel, int method,
                                  void* out_e2m1, void* out_e8m0, void* out_mask, void* stream) {
  return fused_quantize_impl("fusedQuantizeMx", kQuantMx, x, h, rot, numel, 0, method, nullptr, out_e2m1, out_e8m0, out_mask, stream);
}

int qutlass_amd_fused_quantize_nv(const void* x, const void* h, int rot, int64_t numel, int method,
                                  const float* global_scale, void* out_e2m1, void* out_e4m3, void* stream) {
  return fused_quantize_impl("fusedQuantizeNv", kQuantNv, x, h, rot, numel, 0, method, global_scale, out_e2m1, out_e4m3, nullptr, stream);
}

static int blocked_shape_check(const char* name, int64_t rows, int64_t k) {
  if (rows <= 0 || k <= 0 || rows >= (1ll << 31) || k >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: bad shape (%lld, %lld)", name, (long long)rows, (long long)k);
  return QAMD_OK;
}

int qutlass_amd_fused_quantize_mx_blocked(const void* x, const void* h, int rot, int64_t rows, int64_t k, int method,
                                          void* out_e2m1, void* out_e8m0_blocked, void* out_mask, void* stream) {
  if (int rc = blocked_shape_check("fusedQuantizeMxBlocked", rows, k)) return rc;
  return fused_quantize_impl("fusedQuantizeMxBlocked", kQuantMx, x, h, rot, rows * k, k, method, nullptr, out_e2m1, out_e8m0_blocked, out_mask, stream);
}

int qutlass_amd_fused_quantize_nv_blocked(const void* x, const void* h, int rot, int64_t rows, int64_t k, int method,
                                          const float* global_scale, void* out_e2m1, void* out_e4m3_blocked, void* stream) {
  if (int rc = blocked_shape_check("fusedQuantizeNvBlocked", rows, k)) return rc;
  return fused_quantize_impl("fusedQuantizeNvBlocked", kQuantNv, x, h, rot, rows * k, k, method, global_scale, out_e2m1, out_e4m3_blocked, nullptr, stream);
}

// ---- gated MLP: act = silu(gate) * up of x = (rows, 2 * inter) [gate | up], alone or fused into the rotate + quantize ops ----------------------------------
// The fused kernels read gate and up where the plain quantizer reads its operand (4 B instead of 2 B per element, and no (rows, inter) bf16 round trip through
// memory in between); workgroups per CU as quant_grid's rule for the act tiles (calibrated with the doubled read stream: profiles/calib_gated_quantize_*.txt).
static int gated_common_check(const char* name, const void* x, int64_t rows, int64_t inter, int64_t align) {
  if (rows < 0 || inter <= 0 || rows >= (1ll << 31) || inter >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: bad shape (%lld, 2 * %lld)", name, (long long)rows, (long long)inter);
  if (inter % align) return fail(QAMD_ERR_INVALID, "%s: the gate / up width %lld must be a multiple of %lld", name, (long long)inter, (long long)align);
  if ((uintptr_t)x % 16) return fail(QAMD_ERR_INVALID, "%s: x must be 16-byte aligned", name);
  return QAMD_OK;
}

int qutlass_amd_silu_mul_bf16(const void* x, int64_t rows, int64_t inter, void* out, void* stream) {
  const char* name = "silu_and_mul";
  if (int rc = gated_common_check(name, x, rows, inter, 8)) return rc;
  if ((uintptr_t)out % 16) return fail(QAMD_ERR_INVALID, "%s: out must be 16-byte aligned", name);
  if (rows == 0) return QAMD_OK;
  if (!x || !out) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  SiluMulParams p;
  p.x = (const uint16_t*)x; p.out = (uint16_t*)out; p.chunks = rows * (inter / 8); p.cpr = (uint32_t)(inter / 8);
  const RowStreamLaunch l = row_stream_plan(p.chunks, chip_cus());
  hipLaunchKernelGGL(silu_mul_bf16_kernel<0>, dim3(l.grid), dim3(l.threads), 0, (hipStream_t)stream, p);
  return check_launch("silu_mul_bf16_kernel");
}

static int fused_silu_mul_quantize_impl(const char* name, const QuantFormat& f, const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method,
                                        const float* global_scale, int blocked, void* out_e2m1, void* out_sf, void* stream, const QuantGroups* grp = nullptr,
                                        int fmt8 = -1) {
  if (int rc = quant_check_rot(name, f, rot)) return rc;
  if (int rc = quant_check_how(name, f, method, fmt8, true)) return rc;
  if (int rc = gated_common_check(name, x, rows, inter, quant_rp(rot))) return rc;
  // x is addressed with 32-bit offsets from one buffer descriptor (quantize.hip.h, GATED): no silent wrap beyond it
  if (rows * inter >= (1ll << 29)) return fail(QAMD_ERR_INVALID, "%s: x (rows * 2 * inter * 2 = %lld bytes) must stay below 2 GiB", name, (long long)(rows * inter * 4));
  if (rows == 0) return QAMD_OK;
  if (!x || !h || !out_e2m1 || !out_sf || (f.nv && !global_scale) || (grp && !grp->offs)) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (int rc = quant_check_h(name, rot, h)) return rc;
  if (grp) if (int rc = quant_check_groups(name, *grp)) return rc;
  QuantParams p;
  p.x = (const uint16_t*)x; p.h = (const uint16_t*)h; p.out = (uint8_t*)out_e2m1; p.out_sf = (uint8_t*)out_sf;
  p.out_mask = nullptr; p.global_scale = global_scale; p.inter = (int)inter;
  const int grid = quant_fill(p, f, rot, rows * inter, inter, blocked != 0);
  if (grp) return select_quant_grouped<QK_GATED>(method, rot, p, *grp, (hipStream_t)stream, grid, name);
  return select_quant<QK_GATED>(f.nv, method, false, blocked != 0, rot, p, (hipStream_t)stream, grid, name, f.fp8 ? fmt8 : -1);
}

int qutlass_amd_fused_silu_mul_quantize_mx(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method, int blocked, void* out_e2m1,
                                           void* out_e8m0, void* stream) {
  return fused_silu_mul_quantize_impl(blocked ? "fusedSiluMulQuantizeMxBlocked" : "fusedSiluMulQuantizeMx", kQuantMx, x, h, rot, rows, inter, method, nullptr, blocked,
                                      out_e2m1, out_e8m0, stream);
}

int qutlass_amd_fused_silu_mul_quantize_nv(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method, const float* global_scale, int blocked,
                                           void* out_e2m1, void* out_e4m3, void* stream) {
  return fused_silu_mul_quantize_impl(blocked ? "fusedSiluMulQuantizeNvBlocked" : "fusedSiluMulQuantizeNv", kQuantNv, x, h, rot, rows, inter, method, global_scale,
                                      blocked, out_e2m1, out_e4m3, stream);
}

// ---- MoE dispatch and combine: the two ends of a mixture-of-experts MLP around the grouped GEMMs ---------------------------------------------------------
// Dispatch: fusedQuantize{Mx,Nv}(x.index_select(0, src_row)) in one launch, byte for byte -- the quantizer's tile loads go through the row index (quantize.hip.h,
// GATHER), so the (M, K) bf16 copy of the routed tokens is never written.
static int fused_gather_quantize_impl(const char* name, const QuantFormat& f, const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row,
                                      int64_t m, int method, const float* global_scale, void* out_e2m1, void* out_sf, void* stream, const QuantGroups* grp = nullptr,
                                      int fmt8 = -1) {
  if (int rc = quant_check_rot(name, f, rot)) return rc;
  if (int rc = quant_check_how(name, f, method, fmt8)) return rc;
  if (t < 0 || m < 0 || k <= 0 || t >= (1ll << 31) || m >= (1ll << 31) || k >= (1ll << 31))
    return fail(QAMD_ERR_INVALID, "%s: bad shape (x (%lld, %lld), %lld indices)", name, (long long)t, (long long)k, (long long)m);
  if (k % quant_rp(rot)) return fail(QAMD_ERR_INVALID, "%s: the row length %lld must be a multiple of %d", name, (long long)k, quant_rp(rot));
  if ((uintptr_t)x % 16 || (uintptr_t)src_row % 4) return fail(QAMD_ERR_INVALID, "%s: x must be 16-byte aligned (and src_row 4-byte aligned)", name);
  // x is addressed with 32-bit offsets from one buffer descriptor, and offset 2^31 is the kernel's "zero row" (quantize.hip.h, GATHER): no silent wrap beyond it
  if (t * k >= (1ll << 30)) return fail(QAMD_ERR_INVALID, "%s: x (rows * k * 2 = %lld bytes) must stay below 2 GiB", name, (long long)(t * k * 2));
  if (m * k >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: more than 2^31 elements is not supported", name);
  if (m == 0) return QAMD_OK;
  if ((!x && t > 0) || !h || !src_row || !out_e2m1 || !out_sf || (f.nv && !global_scale) || (grp && !grp->offs)) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (int rc = quant_check_h(name, rot, h)) return rc;
  if (grp) if (int rc = quant_check_groups(name, *grp)) return rc;
  QuantParams p;
  p.x = (const uint16_t*)x; p.h = (const uint16_t*)h; p.out = (uint8_t*)out_e2m1; p.out_sf = (uint8_t*)out_sf;
  p.out_mask = nullptr; p.global_scale = global_scale; p.inter = (int)k;
  const int grid = quant_fill(p, f, rot, m * k, k, false, src_row, t);
  if (grp) return select_quant_grouped<QK_GATHER>(method, rot, p, *grp, (hipStream_t)stream, grid, name);
  return select_quant<QK_GATHER>(f.nv, method, false, false, rot, p, (hipStream_t)stream, grid, name, f.fp8 ? fmt8 : -1);
}

int qutlass_amd_fused_gather_quantize_mx(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int method, void* out_e2m1,
                                         void* out_e8m0, void* stream) {
  return fused_gather_quantize_impl("fusedGatherQuantizeMx", kQuantMx, x, h, rot, t, k, src_row, m, method, nullptr, out_e2m1, out_e8m0, stream);
}

int qutlass_amd_fused_gather_quantize_nv(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int method,
                                         const float* global_scale, void* out_e2m1, void* out_e4m3, void* stream) {
  return fused_gather_quantize_impl("fusedGatherQuantizeNv", kQuantNv, x, h, rot, t, k, src_row, m, method, global_scale, out_e2m1, out_e4m3, stream);
}

// The grouped-scale forms of the two NV quantizers of the MoE chain: one global scale per expert, the expert of a row found from offs by the kernel (quantize.hip.h,
// GSCALE).  Each runs its sibling's chain under its own name (a null offs joins the null-pointer check), then quant_check_groups.
int qutlass_amd_fused_gather_quantize_nv_grouped(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int method,
                                                 const float* global_scales, const int32_t* offs, int64_t e, void* out_e2m1, void* out_e4m3, void* stream) {
  const QuantGroups grp{offs, e};
  return fused_gather_quantize_impl("fusedGatherQuantizeNvGrouped", kQuantNv, x, h, rot, t, k, src_row, m, method, global_scales, out_e2m1, out_e4m3, stream, &grp);
}

int qutlass_amd_fused_silu_mul_quantize_nv_grouped(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method, const float* global_scales,
                                                   const int32_t* offs, int64_t e, void* out_e2m1, void* out_e4m3, void* stream) {
  const QuantGroups grp{offs, e};
  return fused_silu_mul_quantize_impl("fusedSiluMulQuantizeNvGrouped", kQuantNv, x, h, rot, rows, inter, method, global_scales, 0, out_e2m1, out_e4m3, stream, &grp);
}

// ---- MXFP8: the same three forms with e4m3 / e5m2 codes (quantize.hip.h, the FP8 arm): the A operands of matmul_mxf8_bf16_tn and grouped_matmul_mxf8_bf16_tn.
// Each entry runs its MX sibling's chain under its own name, with the fmt check where the sibling checks the method (abs-max is the only method).
int qutlass_amd_fused_quantize_mxf8(const void* x, const void* h, int rot, int64_t numel, int fmt, void* out_fp8, void* out_e8m0, void* stream) {
  return fused_quantize_impl("fusedQuantizeMxf8", kQuantMxf8, x, h, rot, numel, 0, QAMD_METHOD_ABSMAX, nullptr, out_fp8, out_e8m0, nullptr, stream, fmt);
}

int qutlass_amd_fused_quantize_mxf8_blocked(const void* x, const void* h, int rot, int64_t rows, int64_t k, int fmt, void* out_fp8, void* out_e8m0_blocked,
                                            void* stream) {
  if (int rc = blocked_shape_check("fusedQuantizeMxf8Blocked", rows, k)) return rc;
  return fused_quantize_impl("fusedQuantizeMxf8Blocked", kQuantMxf8, x, h, rot, rows * k, k, QAMD_METHOD_ABSMAX, nullptr, out_fp8, out_e8m0_blocked, nullptr, stream, fmt);
}

int qutlass_amd_fused_silu_mul_quantize_mxf8(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int fmt, int blocked, void* out_fp8, void* out_e8m0,
                                             void* stream) {
  return fused_silu_mul_quantize_impl(blocked ? "fusedSiluMulQuantizeMxf8Blocked" : "fusedSiluMulQuantizeMxf8", kQuantMxf8, x, h, rot, rows, inter, QAMD_METHOD_ABSMAX,
                                      nullptr, blocked, out_fp8, out_e8m0, stream, nullptr, fmt);
}

int qutlass_amd_fused_gather_quantize_mxf8(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, int fmt, void* out_fp8,
                                           void* out_e8m0, void* stream) {
  return fused_gather_quantize_impl("fusedGatherQuantizeMxf8", kQuantMxf8, x, h, rot, t, k, src_row, m, QAMD_METHOD_ABSMAX, nullptr, out_fp8, out_e8m0, stream, nullptr,
                                    fmt);
}

// ---- MXFP6: the plain and the gathering form with e2m3 codes, four in three bytes (quantize.hip.h, the FP6 arm): the A operand of grouped_matmul_mxf6_mxf4_bf16_tn.
// Each entry runs its MX sibling's chain under its own name; there is neither a method nor a fmt to check.  out_fp6 takes numel * 3 / 4 bytes.
int qutlass_amd_fused_quantize_mxf6(const void* x, const void* h, int rot, int64_t numel, void* out_fp6, void* out_e8m0, void* stream) {
  return fused_quantize_impl("fusedQuantizeMxf6", kQuantMxf6, x, h, rot, numel, 0, QAMD_METHOD_ABSMAX, nullptr, out_fp6, out_e8m0, nullptr, stream, QF_E2M3 - 1);
}

int qutlass_amd_fused_gather_quantize_mxf6(const void* x, const void* h, int rot, int64_t t, int64_t k, const int32_t* src_row, int64_t m, void* out_fp6,
                                           void* out_e8m0, void* stream) {
  return fused_gather_quantize_impl("fusedGatherQuantizeMxf6", kQuantMxf6, x, h, rot, t, k, src_row, m, QAMD_METHOD_ABSMAX, nullptr, out_fp6, out_e8m0, stream, nullptr,
                                    QF_E2M3 - 1);
}

// ---- gpt-oss: the clamped SwiGLU with per-expert biases (quantize.hip.h, swiglu_oai_mul8), alone and fused into the MXFP4 and the MXFP8 (e4m3) quantizer; moe_combine with the down bias ----
// alpha and limit -> the kernels' constants (SwigluOaiAct).  alpha * log2 e = c_hi + c_lo in fp64, c_hi rounded to 16 significant bits: with the gate's 8 the
// product c_hi * gate is exact in fp32.  Outside [2^-100, 2^100] -- where c_hi or ln 2 * c_lo would leave fp32's normal range -- every element takes the fp64 path.
static int swiglu_oai_act(const char* name, float alpha, float limit, SwigluOaiAct& a) {
  if (!(alpha > 0.f) || !std::isfinite(alpha)) return fail(QAMD_ERR_INVALID, "%s: alpha must be finite and > 0 (got %g)", name, (double)alpha);
  uint32_t lb;
  memcpy(&lb, &limit, 4);
  if (!(limit > 0.f) || !std::isfinite(limit) || (lb & 0xffffu))
    return fail(QAMD_ERR_INVALID, "%s: limit must be > 0, finite and exactly representable in bf16 (got %.9g)", name, (double)limit);
  const double c = (double)alpha * 1.4426950408889634;
  int ex;
  (void)frexp(c, &ex);
  const double q = ldexp(1.0, ex - 16), chi = nearbyint(c / q) * q;
  const bool fast = c >= ldexp(1.0, -100) && c <= ldexp(1.0, 100);
  a.nch = fast ? (float)-chi : 0.f;
  a.klo = fast ? (float)(-0.6931471805599453 * (c - chi)) : 0.f;
  a.alpha = alpha; a.tmax = fast ? 16.0f : -1.0f; a.limit = limit;
  return QAMD_OK;
}

// the checks a per-expert bias adds: e, the alignments, offs where more than one expert could own a row
static int swiglu_oai_check_bias(const char* name, const void* bias, const int32_t* offs, int64_t e) {
  if (e < 1 || e > qamd::QUANT_MAX_E) return fail(QAMD_ERR_INVALID, "%s: E must be in [1, %d] (got %lld)", name, qamd::QUANT_MAX_E, (long long)e);
  if ((uintptr_t)bias % 16) return fail(QAMD_ERR_INVALID, "%s: bias must be 16-byte aligned", name);
  if (!offs && e > 1) return fail(QAMD_ERR_INVALID, "%s: a bias of E = %lld experts needs offs", name, (long long)e);
  if ((uintptr_t)offs % 4) return fail(QAMD_ERR_INVALID, "%s: offs must be 4-byte aligned", name);
  return QAMD_OK;
}

int qutlass_amd_swiglu_oai_mul_bf16(const void* x, int64_t rows, int64_t inter, float alpha, float limit, const void* bias, const int32_t* offs, int64_t e, void* out,
                                    void* stream) {
  const char* name = "swiglu_oai_and_mul";
  SwigluOaiParams p;
  if (int rc = gated_common_check(name, x, rows, inter, 8)) return rc;
  if ((uintptr_t)out % 16) return fail(QAMD_ERR_INVALID, "%s: out must be 16-byte aligned", name);
  if (int rc = swiglu_oai_act(name, alpha, limit, p.act)) return rc;
  if (bias) if (int rc = swiglu_oai_check_bias(name, bias, offs, e)) return rc;
  if (rows == 0) return QAMD_OK;
  if (!x || !out) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  p.x = (const uint16_t*)x; p.out = (uint16_t*)out; p.bias = (const uint16_t*)bias; p.offs = offs; p.E = bias ? (int)e : 0;
  p.chunks = rows * (inter / 8); p.cpr = (uint32_t)(inter / 8);
  return launch_swiglu_oai_stream(p, row_stream_plan(p.chunks, chip_cus()), (hipStream_t)stream);
}

// fusedQuantizeMx(swiglu_oai_and_mul(x, ...), h) -- f.fp8: fusedQuantizeMxf8(swiglu_oai_and_mul(x, ...), h, e4m3) -- in one launch, byte for byte: the gated
// quantizer's chain with the activation's checks; flat scales only.  `how` is the method of the e2m1 entry and the fmt of the e4m3 one (quant_check_how).
static int fused_swiglu_oai_quantize_impl(const char* name, const char* plain, const QuantFormat& f, const void* x, const void* h, int rot, int64_t rows, int64_t inter,
                                          int how, float alpha, float limit, const void* bias, const int32_t* offs, int64_t e, void* out, void* out_e8m0, void* stream) {
  QuantParams p;
  if (rot == 128)
    return fail(QAMD_ERR_INVALID, "%s: rotation size 128 is not supported; expected 32 or 64 (use swiglu_oai_and_mul followed by %s)", name, plain);
  if (rot != 32 && rot != 64) return fail(QAMD_ERR_INVALID, "%s: Unsupported rotation size %d; expected 32 or 64.", name, rot);
  if (!f.fp8) { if (int rc = quant_check_method(name, how)) return rc; }
  else if (how != QAMD_FP8_E4M3) return fail(QAMD_ERR_INVALID, "%s: invalid fmt %d; expected 0 (e4m3): a forward activation is e4m3 only", name, how);
  if (int rc = gated_common_check(name, x, rows, inter, rot)) return rc;
  if (rows * inter >= (1ll << 29)) return fail(QAMD_ERR_INVALID, "%s: x (rows * 2 * inter * 2 = %lld bytes) must stay below 2 GiB", name, (long long)(rows * inter * 4));
  if (int rc = swiglu_oai_act(name, alpha, limit, p.oai)) return rc;
  if (bias) {
    if (int rc = swiglu_oai_check_bias(name, bias, offs, e)) return rc;
    if (e * inter >= (1ll << 29)) return fail(QAMD_ERR_INVALID, "%s: bias (E * 2 * inter * 2 = %lld bytes) must stay below 2 GiB", name, (long long)(e * inter * 4));
  }
  if (rows == 0) return QAMD_OK;
  if (!x || !h || !out || !out_e8m0) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (int rc = quant_check_h(name, rot, h)) return rc;
  p.x = (const uint16_t*)x; p.h = (const uint16_t*)h; p.out = (uint8_t*)out; p.out_sf = (uint8_t*)out_e8m0;
  p.out_mask = nullptr; p.global_scale = nullptr; p.inter = (int)inter;
  p.bias = (const uint16_t*)bias; p.offs = offs; p.E = bias ? (int)e : 0;
  const int grid = quant_fill(p, f, rot, rows * inter, inter, false);
  if (f.fp8) return launch_swiglu_oai_quant_mxf8(rot, bias != nullptr, p, (hipStream_t)stream, grid);
  return launch_swiglu_oai_quant(rot, how, bias != nullptr, p, (hipStream_t)stream, grid);
}

int qutlass_amd_fused_swiglu_oai_quantize_mx(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int method, float alpha, float limit, const void* bias,
                                             const int32_t* offs, int64_t e, void* out_e2m1, void* out_e8m0, void* stream) {
  return fused_swiglu_oai_quantize_impl("fusedSwigluOaiQuantizeMx", "fusedQuantizeMx", kQuantMx, x, h, rot, rows, inter, method, alpha, limit, bias, offs, e, out_e2m1,
                                        out_e8m0, stream);
}

// the W4A8 form: e4m3 codes (one byte per element) for the A operand of grouped_matmul_mxf8_mxf4_bf16_tn; abs-max is the only method, so fmt stands where method does
int qutlass_amd_fused_swiglu_oai_quantize_mxf8(const void* x, const void* h, int rot, int64_t rows, int64_t inter, int fmt, float alpha, float limit, const void* bias,
                                               const int32_t* offs, int64_t e, void* out_fp8, void* out_e8m0, void* stream) {
  return fused_swiglu_oai_quantize_impl("fusedSwigluOaiQuantizeMxf8", "fusedQuantizeMxf8", kQuantMxf8, x, h, rot, rows, inter, fmt, alpha, limit, bias, offs, e, out_fp8,
                                        out_e8m0, stream);
}

// Combine: out[t] = sum_k w[t][k] * y[pos[t][k]] in the order and with the roundings moe_combine_bf16_kernel states (quantize.hip.h); slots outside [0, m) are skipped.
// has_bias: the form with the down projection's per-expert bias added to every gathered row in bf16 (moe_combine_bias_bf16_kernel); else bias, offs and e are not read.
static int combine_impl(bool has_bias, const void* y, int64_t m, int64_t hdim, const int32_t* pos, const float* weights, int64_t t, int64_t topk, const void* bias,
                        const int32_t* offs, int64_t e, void* out, void* stream) {
  const char* name = "moe_combine";
  if (m < 0 || t < 0 || hdim <= 0 || m >= (1ll << 31) || t >= (1ll << 31) || hdim >= (1ll << 31))
    return fail(QAMD_ERR_INVALID, "%s: bad shape (y (%lld, %lld), %lld tokens)", name, (long long)m, (long long)hdim, (long long)t);
  if (hdim % 8) return fail(QAMD_ERR_INVALID, "%s: the row length %lld must be a multiple of 8", name, (long long)hdim);
  if (topk < 1 || topk > 32) return fail(QAMD_ERR_INVALID, "%s: bad shape: topk must be in [1, 32] (got %lld)", name, (long long)topk);
  if (((uintptr_t)y | (uintptr_t)out) % 16) return fail(QAMD_ERR_INVALID, "%s: y and out must be 16-byte aligned", name);
  if (has_bias) if (int rc = swiglu_oai_check_bias(name, bias, offs, e)) return rc;
  if (t == 0) return QAMD_OK;
  if ((!y && m > 0) || !pos || !weights || !out || (has_bias && !bias)) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (m == 0) {   // no row to name: every slot is skipped and every sum is its start, +0 (the kernels read row 0 for a skipped slot, so they want one row)
    if (hipMemsetAsync(out, 0, (size_t)(t * hdim * 2), (hipStream_t)stream) != hipSuccess) return fail(QAMD_ERR_HIP, "%s: hipMemsetAsync failed", name);
    return QAMD_OK;
  }
  MoeCombineBiasParams p;   // (the plain kernel takes its first member)
  p.c.y = (const uint16_t*)y; p.c.pos = pos; p.c.w = weights; p.c.out = (uint16_t*)out;
  p.c.chunks = t * (hdim / 8); p.c.cpr = (uint32_t)(hdim / 8); p.c.m = (uint32_t)m; p.c.topk = (int)topk;
  p.bias = (const uint16_t*)bias; p.offs = offs; p.E = (int)e;
  const RowStreamLaunch l = row_stream_plan(p.c.chunks, chip_cus());
  if (has_bias) return launch_moe_combine_bias(p, l, (hipStream_t)stream);
  hipLaunchKernelGGL(moe_combine_bf16_kernel<0>, dim3(l.grid), dim3(l.threads), 0, (hipStream_t)stream, p.c);
  return check_launch("moe_combine_bf16_kernel");
}
int qutlass_amd_moe_combine_bf16(const void* y, int64_t m, int64_t hdim, const int32_t* pos, const float* weights, int64_t t, int64_t topk, void* out, void* stream) {
  return combine_impl(false, y, m, hdim, pos, weights, t, topk, nullptr, nullptr, 0, out, stream);
}
int qutlass_amd_moe_combine_bias_bf16(const void* y, int64_t m, int64_t hdim, const int32_t* pos, const float* weights, int64_t t, int64_t topk, const void* bias,
                                      const int32_t* offs, int64_t e, void* out, void* stream) {
  return combine_impl(true, y, m, hdim, pos, weights, t, topk, bias, offs, e, out, stream);
}

// ---- MoE routing: the front of the chain (moe_route.hip.h) ---------------------------------------------------------------------------------------------------
// Router logits -> top-k ids (exact: logit descending, expert index ascending) and softmax weights; one wave per token, one launch, no workspace.
// Both routers: topk_check (the checks they share), their own checks and fill, moe_topk_plan (moe_route.hip.h), launch_topk -- one arm per kernel of the family, an error for any other.
extern "C++" {
struct TopkSoftmax { static constexpr const char* what = "moe_topk_softmax_kernel"; template <typename T, int R, bool V> static auto kernel() { return moe_topk_softmax_kernel<T, R, V>; } };
struct TopkGrouped { static constexpr const char* what = "moe_topk_grouped_kernel"; template <typename T, int R, bool V> static auto kernel() { return moe_topk_grouped_kernel<T, R, V>; } };
struct RouteFused { static constexpr const char* what = "moe_route_fused_kernel"; template <typename T, int R, bool V> static auto kernel() { return moe_route_fused_kernel<T, R, V>; } };
struct RouteGroupedFused { static constexpr const char* what = "moe_route_grouped_fused_kernel"; template <typename T, int R, bool V> static auto kernel() { return moe_route_grouped_fused_kernel<T, R, V>; } };
template <typename F, typename... P>   // p: the kernel's arguments -- the router's parameters, and the sort's behind them for the one-launch routing kernels
static int launch_topk(const char* name, int elem_bytes, const MoeTopkLaunch& l, hipStream_t s, const P&... p) {
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, s, p...); return check_launch(F::what); };
  constexpr auto arm = [](int eb, int r, bool v) { return eb * 64 + r * 2 + v; };   constexpr bool V = true, S = false;   using bf16 = uint16_t;   // (V / S: 16-byte vector loads / single columns)
  switch (arm(elem_bytes, l.R, l.loadv)) {
    case arm(2, 8, V): return go(F::template kernel<bf16, 8, V>());     case arm(2, 8, S): return go(F::template kernel<bf16, 8, S>());
    case arm(2, 16, V): return go(F::template kernel<bf16, 16, V>());   case arm(2, 16, S): return go(F::template kernel<bf16, 16, S>());
    case arm(4, 4, V): return go(F::template kernel<float, 4, V>());    case arm(4, 4, S): return go(F::template kernel<float, 4, S>());
    case arm(4, 8, V): return go(F::template kernel<float, 8, V>());    case arm(4, 8, S): return go(F::template kernel<float, 8, S>());
    case arm(4, 16, V): return go(F::template kernel<float, 16, V>());  case arm(4, 16, S): return go(F::template kernel<float, 16, S>());
  }
  return fail(QAMD_ERR_INVALID, "%s: this build holds no kernel for R = %d with %d-byte logits", name, l.R, elem_bytes);
}
template <typename IdT>   // the expert sort (further down): one launch or three, as moe_sort_plan says
static void launch_moe_sort(const MoeSortParams& p, const MoeSortLaunch& l, hipStream_t s) {
  if (l.launches == 1) { hipLaunchKernelGGL((moe_sort_kernel<IdT, 0>), dim3(1), dim3(MOE_SORT_NT), 0, s, p); return; }
  hipLaunchKernelGGL((moe_sort_kernel<IdT, 1>), dim3(l.rows), dim3(MOE_SORT_NT), 0, s, p);
  hipLaunchKernelGGL(moe_sort_scan_kernel<0>, dim3(1), dim3(MOE_SORT_NT), 0, s, p);
  hipLaunchKernelGGL((moe_sort_kernel<IdT, 3>), dim3(l.rows), dim3(MOE_SORT_NT), 0, s, p);
}
}   // extern "C++"
static int topk_check(const char* name, int elem_bytes, int64_t t, int64_t e) {
  if (elem_bytes != 2 && elem_bytes != 4) return fail(QAMD_ERR_INVALID, "%s: logits must be bf16 (elem_bytes 2) or float32 (4), got elem_bytes %d", name, elem_bytes);
  if (t < 0 || t >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: bad shape (%lld tokens)", name, (long long)t);
  if (e < 1 || e > 1024) return fail(QAMD_ERR_INVALID, "%s: bad shape: the number of experts must be in [1, 1024] (got %lld)", name, (long long)e);
  return QAMD_OK;
}

// The softmax router's checks and kernel parameters: what qutlass_amd_moe_topk_softmax and qutlass_amd_moe_route_fused both do with these arguments (t == 0 passes with p not filled).
static int topk_softmax_args(const char* name, const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int renormalize, float* weights, int32_t* ids, MoeTopkParams& p) {
  if (int rc = topk_check(name, elem_bytes, t, e)) return rc;
  if (topk < 1 || topk > 32 || topk > e) return fail(QAMD_ERR_INVALID, "%s: bad shape: topk must be in [1, min(E, 32)] (got %lld for E = %lld)", name, (long long)topk, (long long)e);
  if ((uintptr_t)logits % elem_bytes || (uintptr_t)weights % 4 || (uintptr_t)ids % 4) return fail(QAMD_ERR_INVALID, "%s: logits, weights and ids must be aligned to their element size", name);
  if (t == 0) return QAMD_OK;
  if (!logits || !weights || !ids) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  p.logits = logits; p.weights = weights; p.ids = ids; p.t = t; p.e = (int)e; p.topk = (int)topk; p.renorm = renormalize ? 1 : 0;
  return QAMD_OK;
}

int qutlass_amd_moe_topk_softmax(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int renormalize, float* weights, int32_t* ids, void* stream) {
  const char* name = "moe_topk_softmax";
  MoeTopkParams p;
  if (int rc = topk_softmax_args(name, logits, elem_bytes, t, e, topk, renormalize, weights, ids, p)) return rc;
  if (t == 0) return QAMD_OK;
  return launch_topk<TopkSoftmax>(name, elem_bytes, moe_topk_plan(elem_bytes, e, t, (uintptr_t)logits % 16 == 0, chip_cus()), (hipStream_t)stream, p);
}

// Grouped top-k (DeepSeek-V2 / V3, Kimi-K2 routers): scores, a selection bias, a top-k inside the best groups; the same launch shape as moe_topk_softmax.
// Its checks and kernel parameters, for qutlass_amd_moe_topk_grouped and qutlass_amd_moe_route_grouped_fused (t == 0 passes with p not filled).
static int topk_grouped_args(const char* name, const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int64_t n_group, int64_t topk_group, int scoring,
                             const float* bias, int renormalize, float routed_scaling_factor, float* weights, int32_t* ids, float* scores, MoeGroupedParams& p) {
  if (int rc = topk_check(name, elem_bytes, t, e)) return rc;
  if (n_group < 1 || n_group > 64) return fail(QAMD_ERR_INVALID, "%s: bad shape: n_group must be in [1, 64] (got %lld)", name, (long long)n_group);
  if (e % n_group != 0) return fail(QAMD_ERR_INVALID, "%s: bad shape: n_group must divide E (got n_group = %lld for E = %lld)", name, (long long)n_group, (long long)e);
  if (topk_group < 1 || topk_group > n_group)
    return fail(QAMD_ERR_INVALID, "%s: bad shape: topk_group must be in [1, n_group] (got %lld for n_group = %lld)", name, (long long)topk_group, (long long)n_group);
  if (topk < 1 || topk > 32 || topk > topk_group * (e / n_group))
    return fail(QAMD_ERR_INVALID, "%s: bad shape: topk must be in [1, min(32, topk_group * E / n_group)] (got %lld for E = %lld, n_group = %lld, topk_group = %lld)", name,
                (long long)topk, (long long)e, (long long)n_group, (long long)topk_group);
  if (scoring != QAMD_MOE_SCORING_SIGMOID && scoring != QAMD_MOE_SCORING_SOFTMAX)
    return fail(QAMD_ERR_INVALID, "%s: scoring must be QAMD_MOE_SCORING_SIGMOID (0) or QAMD_MOE_SCORING_SOFTMAX (1), got %d", name, scoring);
  if ((uintptr_t)logits % elem_bytes || ((uintptr_t)bias | (uintptr_t)weights | (uintptr_t)ids | (uintptr_t)scores) % 4)
    return fail(QAMD_ERR_INVALID, "%s: logits, bias, weights, ids and scores must be aligned to their element size", name);
  if (t == 0) return QAMD_OK;
  if (!logits || !weights || !ids) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  p.logits = logits; p.bias = bias; p.weights = weights; p.ids = ids; p.scores = scores; p.t = t; p.e = (int)e; p.topk = (int)topk; p.renorm = renormalize ? 1 : 0;
  p.sigmoid = scoring == QAMD_MOE_SCORING_SIGMOID; p.n_group = (int)n_group; p.topk_group = (int)topk_group; p.s = (int)(e / n_group);
  p.lg_l = 0;
  while ((n_group << (p.lg_l + 1)) <= 64) ++p.lg_l;   // L lanes per group in the group stage
  p.magic = (uint32_t)(((1ll << 22) + p.s - 1) / p.s);
  p.scale = routed_scaling_factor;
  return QAMD_OK;
}

int qutlass_amd_moe_topk_grouped(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int64_t n_group, int64_t topk_group, int scoring,
                                 const float* bias, int renormalize, float routed_scaling_factor, float* weights, int32_t* ids, float* scores, void* stream) {
  const char* name = "moe_topk_grouped";
  MoeGroupedParams p;
  if (int rc = topk_grouped_args(name, logits, elem_bytes, t, e, topk, n_group, topk_group, scoring, bias, renormalize, routed_scaling_factor, weights, ids, scores, p)) return rc;
  if (t == 0) return QAMD_OK;
  const bool aligned = (uintptr_t)logits % 16 == 0 && (uintptr_t)scores % 16 == 0;   // the scores, if asked for, are stored as 16-byte vectors too
  return launch_topk<TopkGrouped>(name, elem_bytes, moe_topk_plan(elem_bytes, e, t, aligned, chip_cus()), (hipStream_t)stream, p);
}

// One-launch routing for decode (moe_route.hip.h): either router's checks above, then the sort's for the map and the three results, then ONE launch of one workgroup.
// The sort's half of the checks and of the kernel's parameters (n > 0 slots; the ids are handed over in LDS, so sp.ids stays null).
int64_t qutlass_amd_moe_route_fused_max_tokens(void) { return MOE_ROUTE_FUSED_TOKENS; }

static int route_fused_sort_args(const char* name, int64_t t, int64_t topk, int64_t num_experts, const int32_t* expert_map, int64_t g, int32_t* src_row, int32_t* offs,
                                 int32_t* pos, MoeSortParams& p) {
  if (t > MOE_ROUTE_FUSED_MAX_T)
    return fail(QAMD_ERR_INVALID, "%s: the one-launch routing takes at most %d tokens (got %lld): use the router and qutlass_amd_moe_sort beyond", name, MOE_ROUTE_FUSED_MAX_T, (long long)t);
  if (num_experts < 1 || num_experts > 1024) return fail(QAMD_ERR_INVALID, "%s: bad shape: the number of experts must be in [1, 1024] (got %lld)", name, (long long)num_experts);
  if (g < 0 || g >= (1ll << 31) || (expert_map && g == 0)) return fail(QAMD_ERR_INVALID, "%s: bad shape (expert_map of %lld entries)", name, (long long)g);
  if (((uintptr_t)expert_map | (uintptr_t)src_row | (uintptr_t)offs | (uintptr_t)pos) % 4)
    return fail(QAMD_ERR_INVALID, "%s: expert_map and the results must be aligned to their element size", name);
  if (t == 0) return QAMD_OK;
  if (!src_row || !offs || !pos) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  p.ids = nullptr; p.map = expert_map; p.src_row = src_row; p.offs = offs; p.pos = pos; p.ws = nullptr;
  p.n = t * topk; p.spb = cdiv(p.n, 512) * 512; p.rows = 1; p.g = (int)g; p.e = (int)num_experts; p.topk = (int)topk;
  p.nbits = 0;
  while ((num_experts >> p.nbits) != 0) ++p.nbits;   // keys are 0 .. E
  return QAMD_OK;
}

int qutlass_amd_moe_route_fused(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int renormalize, float* weights, int32_t* ids, int64_t num_experts,
                                const int32_t* expert_map, int64_t g_entries, int32_t* src_row, int32_t* offs, int32_t* pos, void* stream) {
  const char* name = "moe_route_fused";
  MoeTopkParams tp;
  MoeSortParams sp;
  if (int rc = topk_softmax_args(name, logits, elem_bytes, t, e, topk, renormalize, weights, ids, tp)) return rc;
  if (int rc = route_fused_sort_args(name, t, topk, num_experts, expert_map, g_entries, src_row, offs, pos, sp)) return rc;
  if (t == 0) return QAMD_OK;
  return launch_topk<RouteFused>(name, elem_bytes, moe_route_fused_plan(elem_bytes, e, t, (uintptr_t)logits % 16 == 0), (hipStream_t)stream, tp, sp);
}

int qutlass_amd_moe_route_grouped_fused(const void* logits, int elem_bytes, int64_t t, int64_t e, int64_t topk, int64_t n_group, int64_t topk_group, int scoring,
                                        const float* bias, int renormalize, float routed_scaling_factor, float* weights, int32_t* ids, int64_t num_experts,
                                        const int32_t* expert_map, int64_t g_entries, int32_t* src_row, int32_t* offs, int32_t* pos, void* stream) {
  const char* name = "moe_route_grouped_fused";
  MoeGroupedParams tp;
  MoeSortParams sp;
  if (int rc = topk_grouped_args(name, logits, elem_bytes, t, e, topk, n_group, topk_group, scoring, bias, renormalize, routed_scaling_factor, weights, ids, nullptr, tp)) return rc;
  if (int rc = route_fused_sort_args(name, t, topk, num_experts, expert_map, g_entries, src_row, offs, pos, sp)) return rc;
  if (t == 0) return QAMD_OK;
  return launch_topk<RouteGroupedFused>(name, elem_bytes, moe_route_fused_plan(elem_bytes, e, t, (uintptr_t)logits % 16 == 0), (hipStream_t)stream, tp, sp);
}

// Expert sort: moe_sort_plan (moe_route.hip.h) -- the size of the scratch, the entry's check of it, the geometry it fills in and the launches all read that one result.
int64_t qutlass_amd_moe_sort_workspace_bytes(int64_t n, int64_t num_experts) {
  return n >= (1ll << 31) || num_experts < 1 || num_experts > 1024 ? 0 : moe_sort_plan(n, num_experts, opt_moe_sort_one_launch_max()).ws_bytes;
}

int qutlass_amd_moe_sort(const void* topk_ids, int id_bytes, int64_t t, int64_t topk, int64_t num_experts, const int32_t* expert_map, int64_t g, int32_t* src_row,
                         int32_t* offs, int32_t* pos, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "moe_sort";
  if (id_bytes != 4 && id_bytes != 8) return fail(QAMD_ERR_INVALID, "%s: topk_ids must be int32 (id_bytes 4) or int64 (8), got id_bytes %d", name, id_bytes);
  if (t < 0 || topk < 1 || t >= (1ll << 31) || topk >= (1ll << 31) || t * topk >= (1ll << 31))
    return fail(QAMD_ERR_INVALID, "%s: bad shape (topk_ids (%lld, %lld)): topk >= 1 and T * topk < 2^31", name, (long long)t, (long long)topk);
  if (num_experts < 1 || num_experts > 1024) return fail(QAMD_ERR_INVALID, "%s: bad shape: the number of experts must be in [1, 1024] (got %lld)", name, (long long)num_experts);
  if (g < 0 || g >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: bad shape (expert_map of %lld entries)", name, (long long)g);
  if ((uintptr_t)topk_ids % id_bytes || ((uintptr_t)expert_map | (uintptr_t)src_row | (uintptr_t)offs | (uintptr_t)pos | (uintptr_t)workspace) % 4)
    return fail(QAMD_ERR_INVALID, "%s: topk_ids, expert_map, the results and the workspace must be aligned to their element size", name);
  const int64_t n = t * topk;
  const MoeSortLaunch l = moe_sort_plan(n, num_experts, opt_moe_sort_one_launch_max());
  if (l.ws_bytes > 0 && (!workspace || workspace_bytes < l.ws_bytes))
    return fail(QAMD_ERR_INVALID, "%s: %lld slots need a workspace of %lld bytes (qutlass_amd_moe_sort_workspace_bytes), got %lld", name, (long long)n, (long long)l.ws_bytes,
                (long long)(workspace ? workspace_bytes : 0));
  if (n == 0) return QAMD_OK;
  if (!topk_ids || !src_row || !offs || !pos) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  MoeSortParams p;
  p.ids = topk_ids; p.map = expert_map; p.src_row = src_row; p.offs = offs; p.pos = pos; p.ws = l.launches == 3 ? (uint32_t*)workspace : nullptr;
  p.n = n; p.g = (int)g; p.e = (int)num_experts; p.topk = (int)topk; p.spb = l.spb; p.rows = l.rows;
  p.nbits = 0;
  while ((num_experts >> p.nbits) != 0) ++p.nbits;   // keys are 0 .. E
  if (id_bytes == 8) launch_moe_sort<int64_t>(p, l, (hipStream_t)stream); else launch_moe_sort<int32_t>(p, l, (hipStream_t)stream);
  return check_launch("moe_sort_kernel");
}

// How many launches should the activation path y = Q(x h) W^T of one linear layer take (the rule behind qutlass_amd.fused_quantize_matmul_mxf4_bf16_tn;
// reference flow: qutlass/__init__.py:149-180 -> qutlass/utils.py:160-193 -> qutlass/__init__.py:34-76 = three launches)?
//   1  ONE launch, qutlass_amd_fused_quantize_matmul_mxf4_bf16_tn (gemm_mx_fusedq.hip.h: the small-batch GEMM rotates and quantises its own A operand).  It repeats
//      the rotate + quantize chains of its K slices in every workgroup -- ceil(K / 2048) x (1, 2, 4 for M <= 4, 8, 16) chains per wave -- and wins while that stays
//      short: [r6] M <= 4: K <= 4096, M <= 8: K <= 2048 (see below), R = 32, and a weight the small-batch GEMM handles (N < 32 x CUs = 8192 on an MI355X).
//      M = 1 / 8 / 16 at N = K = 4096: 5.0 / 6.0 / 7.6 us against 7.3 / 7.9 / 8.2 us for two launches and 9.0 / 9.5 / 9.9 for three (GEMM alone 4.6 / 4.9 / 5.3);
//      M = 32 or K = 14336 lose (14.2 vs 9.0 us, 12.6 vs 10.7 us).
//   2  TWO launches everywhere else: qutlass_amd_fused_quantize_mx_blocked (scales written in the to_blocked layout) + the GEMM.  The blocked quantizer costs
//      0.2 ... 0.8 us more than the flat one and saves the 1.9 ... 3.2 us to_blocked launch: 2.2 vs 4.5 us at 256 x 4096, 7.3 vs 10.4 at 4096^2, 27.9 vs 31.4 at
//      8192^2, 23.4 vs 26.5 at 4096 x 14336 -- device time, every size measured (profiles/ab_blocked_quant_r3y.txt); with the GEMM behind it: 4096 x 14336 x 4096
//      123.2 vs 124.5 us (profiles/bench_r4c.json).  It never returns 3: the reference's three-launch flow stays available as fusedQuantizeMx + to_blocked + matmul.
// Thresholds scale with the CU count of the current device.  No GPU work.
static int activation_path_plan(int64_t M, int64_t N, int64_t K, int rot, int cus) {
  if (M <= 0 || N <= 0 || K <= 0 || M > 16 || rot != 32 || N >= 32ll * cus || K % 128) return 2;
  // [r6] re-taken after the decode forms made the GEMM of the two-launch path faster (N = K = 4096, M <= 16: 4.6-5.3 -> 2.85-3.0 us; tools/calib_actpath.py,
  // profiles/calib_actpath_r7.txt): two launches now take 5.2-5.7 us at N = K = 4096 where the one-launch kernel takes 5.1 / 5.3 / 6.2 / 8.1 (M = 1 / 4 / 8 / 16), 6.4 against
  // 8.4-8.8 at 4096 x 8192 -- one launch keeps M <= 4 with K <= 4096 (4096 x 6144: a tie) and M <= 8 with K <= 2048 (3.8-4.4 against 4.6-4.9); rounds 3-5: M <= 4: K <= 8192,
  // M <= 8: K <= 6144, M <= 16: K <= 4096
  return K <= (M <= 4 ? 4096 : M <= 8 ? 2048 : 0) ? 1 : 2;
}
int qutlass_amd_activation_path_launches(int64_t M, int64_t N, int64_t K, int rot) { return activation_path_plan(M, N, K, rot, chip_cus()); }

#if QAMD_BENCH
// [r6] lab ("gemm_variant" 580): the hand-off form of the one-launch layer (gemm_mx_os16_fq_kernel: the quantizer's body on the first workgroups, the decode form's K walk
// behind one arrival counter) on a scratch buffer the LAB library allocates once -- an experiment's plumbing, not an API (the product would take caller scratch)
static int fusedq_lab_handoff(const char* name, const void* x, const void* h, int method, const void* B, const void* B_sf, const float* alpha, void* D, int64_t M,
                              int64_t N, int64_t K, int tn, hipStream_t st) {
  static void* scratch = nullptr;
  if (!scratch && hipMalloc(&scratch, 1 << 20) != hipSuccess) return fail(QAMD_ERR_HIP, "%s: lab scratch", name);
  const int64_t CB = cdiv(K / 32, 4);
  FqOsParams P;
  P.q.x = (const uint16_t*)x; P.q.h = (const uint16_t*)h; P.q.out = (uint8_t*)scratch; P.q.out_sf = (uint8_t*)scratch + (256 << 10); P.q.out_mask = nullptr; P.q.global_scale = nullptr;
  P.q.numel = M * K; P.q.ntiles = (int)cdiv(M * K, 1024); P.q.sf_rows = (int)M; P.q.sf_cols = (int)(K / 32);
  GemmParams& g = P.g;
  g.A = (const uint8_t*)scratch; g.B = (const uint8_t*)B; g.SFA = (const uint8_t*)scratch + (256 << 10); g.SFB = (const uint8_t*)B_sf; g.alpha = alpha; g.D = (uint16_t*)D;
  g.M = (int)M; g.N = (int)N; g.K = (int)K; g.ldd = (int)N;
  g.a_bytes = (uint32_t)(M * (K / 2)); g.b_bytes = (uint32_t)(N * (K / 2)); g.sfa_bytes = (uint32_t)(CB * 512); g.sfb_bytes = (uint32_t)(cdiv(N, 128) * CB * 512);
  g.pp_shift = 0; g.pp_flags = 0; g.dbg = nullptr; g.ws = nullptr; g.splits = 1; g.ctr = nullptr; g.tag = 0; g.sk_tiles = 0;
  g.tiles_m = 1; g.tiles_n = (int)cdiv(N, tn); g.raster_magic = 0;
  P.flag = (unsigned long long*)((uint8_t*)scratch + (512 << 10));
  P.tag = (next_launch_tag() & ((1ull << 56) - 1)) << 8;
  P.nq = (int)std::min<int64_t>(cdiv(P.q.ntiles, 4), g.tiles_n);
  const int64_t KT = cdiv(K, 256);
  const dim3 grid(g.tiles_n), block(256);
#define QAMD_FQOS(TN_, SPW_)                                                                                                                     \
  do {                                                                                                                                         \
    if (method == QAMD_METHOD_ABSMAX) hipLaunchKernelGGL((gemm_mx_os16_fq_kernel<Os16Cfg<SPW_, 4, 0, TN_>, METHOD_ABSMAX>), grid, block, 0, st, P); \
    else hipLaunchKernelGGL((gemm_mx_os16_fq_kernel<Os16Cfg<SPW_, 4, 0, TN_>, METHOD_QUEST>), grid, block, 0, st, P);                              \
  } while (0)
  if (tn == 16) { if (KT <= 16) QAMD_FQOS(16, 4); else QAMD_FQOS(16, 8); }
  else if (tn == 32 && KT <= 16) QAMD_FQOS(32, 4);
  else if (tn == 48 && KT <= 16) QAMD_FQOS(48, 4);
  else if (tn == 56 && KT <= 16) QAMD_FQOS(56, 4);
  else return fail(QAMD_ERR_INVALID, "%s: lab variant 580 has no instantiation for this shape", name);
#undef QAMD_FQOS
  return check_launch("gemm_mx_os16_fq_kernel");
}
#endif
// rows per rotation tile: the smallest of 4 / 8 / 16 / 32 that holds the batch (fewer rows = more scale groups per tile = fewer rotate + quantize chains per K segment, gemm_mx_fusedq.hip.h)
static int fusedq_plan(int64_t M) { return M <= 4 ? 4 : M <= 8 ? 8 : M <= 16 ? 16 : 32; }

// decode-time activation path in one launch (gemm_mx_fusedq.hip.h): D = alpha * Q(x . h) (B . SFB)^T for M <= 32
int qutlass_amd_fused_quantize_matmul_mxf4_bf16_tn(const void* x, const void* h, int rot, int method, const void* B, const void* B_sf,
                                                   const float* alpha, void* D, int64_t M, int64_t N, int64_t K, void* stream) {
  const char* name = "fusedQuantizeMatmulMxf4";
  if (!x || !h || !B || !B_sf || !alpha || !D) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (rot != 32) return fail(QAMD_ERR_INVALID, "%s: Unsupported rotation size %d; expected 32.", name, rot);
  if (method != QAMD_METHOD_QUEST && method != QAMD_METHOD_ABSMAX) return fail(QAMD_ERR_INVALID, "%s: invalid method %d", name, method);
  if (M <= 0 || M > 32) return fail(QAMD_ERR_INVALID, "%s: M must be in 1..32 (got %lld); larger batches take fusedQuantizeMxBlocked + matmul_mxf4_bf16_tn", name, (long long)M);
  if (N <= 0 || N % 8) return fail(QAMD_ERR_INVALID, "%s: N must be a positive multiple of 8 (got %lld)", name, (long long)N);
  if (K < 128 || K % 128) return fail(QAMD_ERR_INVALID, "%s: K must be a positive multiple of 128 (got %lld)", name, (long long)K);
  if (N * (K / 2) >= (1ll << 31) || M * K * 2 >= (1ll << 31) || cdiv(N, 32) >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: operand larger than 2 GiB is not supported", name);
#if QAMD_BENCH
  if (const MxFormRow* f = opt_gemm_variant() == 580 && M <= 16 && K <= 8192 ? os16_form(N, chip_cus()) : nullptr) return fusedq_lab_handoff(name, x, h, method, B, B_sf, alpha, D, M, N, K, f->tn, (hipStream_t)stream);
#endif
  FusedQParams p;
  p.x = (const uint16_t*)x; p.h = (const uint16_t*)h; p.B = (const uint8_t*)B; p.SFB = (const uint8_t*)B_sf; p.alpha = alpha; p.D = (uint16_t*)D;
  p.M = (int)M; p.N = (int)N; p.K = (int)K;
  p.x_bytes = (uint32_t)(M * K * 2); p.b_bytes = (uint32_t)(N * (K / 2)); p.sfb_bytes = (uint32_t)(cdiv(N, 128) * cdiv(K / 32, 4) * 512);
  const dim3 grid((unsigned)cdiv(N, 32), 1), block(512);
  hipStream_t s = (hipStream_t)stream;
  auto go = [&](auto meth_, auto hw_) {   // (method, e2m1 encoder: integral constants; the software encoder is lab-only) x the plan's rows per rotation tile
    switch (fusedq_plan(M)) {
      case 4: hipLaunchKernelGGL((gemm_mx_fusedq_kernel<meth_(), hw_(), 4>), grid, block, 0, s, p); break;
      case 8: hipLaunchKernelGGL((gemm_mx_fusedq_kernel<meth_(), hw_(), 8>), grid, block, 0, s, p); break;
      case 16: hipLaunchKernelGGL((gemm_mx_fusedq_kernel<meth_(), hw_(), 16>), grid, block, 0, s, p); break;
      default: hipLaunchKernelGGL((gemm_mx_fusedq_kernel<meth_(), hw_(), 32>), grid, block, 0, s, p);
    }
  };
  using Quest = std::integral_constant<int, METHOD_QUEST>; using AbsMax = std::integral_constant<int, METHOD_ABSMAX>;
#if QAMD_BENCH
  if (!opt_hw_fp4()) { if (method == QAMD_METHOD_ABSMAX) go(AbsMax{}, std::false_type{}); else go(Quest{}, std::false_type{}); } else
#endif
  if (method == QAMD_METHOD_ABSMAX) go(AbsMax{}, std::true_type{}); else go(Quest{}, std::true_type{});
  return check_launch("gemm_mx_fusedq_kernel");
}

// ---- the QAT-backward data-prep ops: check, fill the parameters, stream_launch_plan (quartet_bwd.hip.h: which kernel form, how many workgroups), launch ----
// (bwd_check: backward_t_bf16 / backward_qt_bf16, m_mult 8 / 32; rows_check: the two _rows ops, n a multiple of 128 -- need_n says so -- / 256: every check, in the entries' order)
static int bwd_check(const char* name, int m_mult, bool null_arg, int64_t B, int64_t N, int64_t M) {
  if (null_arg) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (B <= 0 || N <= 0 || M <= 0 || N % 32 || M % m_mult) return fail(QAMD_ERR_INVALID, "%s: need N %% 32 == 0 and M %% %d == 0 (got B=%lld N=%lld M=%lld)", name, m_mult, (long long)B, (long long)N, (long long)M);
  if (B * N * M >= (1ll << 40) || M >= (1ll << 24) || N >= (1ll << 26)) return fail(QAMD_ERR_INVALID, "%s: tensor too large", name);   // 32 input rows / 64 output rows < 2^31 bytes
  if (B * (N / 32) * cdiv(M, 64) >= (1ll << 31) - 65536) return fail(QAMD_ERR_INVALID, "%s: tensor too large", name);   // (BwdTParams::tiles_m: the kernels index tiles in 32 bits)
  return QAMD_OK;
}
static int rows_check(const char* name, int n_mult, const char* need_n, bool null_arg, int64_t m, int64_t m_pad, int64_t n) {
  if (null_arg) return fail(QAMD_ERR_INVALID, "%s: null pointer argument", name);
  if (m <= 0 || n <= 0 || n % n_mult || m_pad < m || m_pad % 128)
    return fail(QAMD_ERR_INVALID, "%s: need m > 0, %s and the output row extent a multiple of 128 >= m (got m=%lld m_pad=%lld n=%lld)", name, need_n, (long long)m, (long long)m_pad, (long long)n);
  if (m_pad >= (1ll << 31) || n >= (1ll << 31) || (m_pad / 128) * (n / 128) >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "%s: tensor too large", name);
  return QAMD_OK;
}

int qutlass_amd_backward_t_bf16(const void* x, const void* h, int64_t B, int64_t N, int64_t M, void* out_e2m1,
                                void* out_e8m0, void* stream) {
  const char* name = "backward_t_bf16";
  if (const int rc = bwd_check(name, 8, !x || !h || !out_e2m1 || !out_e8m0, B, N, M)) return rc;
  BwdTParams p{};
  p.x = (const uint16_t*)x; p.h = (const uint16_t*)h; p.out = (uint8_t*)out_e2m1; p.out_sf = (uint8_t*)out_e8m0;
  p.B = (int)B; p.N = (int)N; p.M = (int)M; p.tiles_m = (int)cdiv(M, 64); p.abl = opt_bwd_variant() >> 4;
  return launch_bwd_quant(name, p, false, opt_hw_fp4(), stream_launch_plan(OP_T, B, N, M, chip_cus(), opt_bwd_variant() & 15, false), (hipStream_t)stream);
}

int qutlass_amd_backward_qt_bf16(const void* x_e2m1, const void* x_e8m0, const void* h, const float* alpha, int64_t B,
                                 int64_t N, int64_t M, void* out_e2m1, void* out_e8m0, void* stream) {
  const char* name = "backward_qt_bf16";
  if (const int rc = bwd_check(name, 32, !x_e2m1 || !x_e8m0 || !h || !alpha || !out_e2m1 || !out_e8m0, B, N, M)) return rc;
  BwdTParams p{};
  p.xq = (const uint8_t*)x_e2m1; p.xs = (const uint8_t*)x_e8m0; p.h = (const uint16_t*)h; p.alpha = alpha;
  p.out = (uint8_t*)out_e2m1; p.out_sf = (uint8_t*)out_e8m0;
  p.B = (int)B; p.N = (int)N; p.M = (int)M; p.tiles_m = (int)cdiv(M, 64); p.abl = opt_bwd_variant() >> 4;
  // (the ring kernel fetches by LDS-DMA: 16-byte pieces of the codes, dword pieces of the scale bytes -- an offset view that breaks either alignment takes the other kernels)
  const int v = opt_bwd_variant() & 15;
  const StreamLaunch l = stream_launch_plan(OP_QT, B, N, M, chip_cus(), v, (uintptr_t)x_e2m1 % 16 == 0 && (uintptr_t)x_e8m0 % 4 == 0);
  if (l.form == SF_NONE) return fail(QAMD_ERR_INVALID, "%s: the %s kernel needs M %% 128 == 0", name, v == QT_PANEL ? "panel" : "ring");   // (lab: a forced whole-line form)
  return launch_bwd_quant(name, p, true, opt_hw_fp4(), l, (hipStream_t)stream);
}

// the square-double and transposer kernels live in this unit; as launch_bwd_quant: one arm per form, each naming one instantiation
static int launch_square_double(const char* name, const SqParams& p, const StreamLaunch& l, hipStream_t s) {
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)l.grid), dim3(l.threads), 0, s, p); return check_launch("bwd_square_double_mxfp8_kernel"); };
  switch (l.form) {
    case SQ_CT1: return go(bwd_square_double_mxfp8_kernel<1, 1>);
    case SQ_CT4: return go(bwd_square_double_mxfp8_kernel<4, 1>);
#if QAMD_BENCH
    case SQ_CT8: return go(bwd_square_double_mxfp8_kernel<4, 2>);   // two tiles per wave
#endif
  }
  return fail(QAMD_ERR_INVALID, "%s: this build holds no kernel for form %d", name, l.form);
}
static int launch_transpose(const char* name, const TrParams& p, const StreamLaunch& l, hipStream_t s) {
  auto go = [&](auto kern, const char* what) { hipLaunchKernelGGL(kern, dim3((unsigned)l.grid), dim3(l.threads), 0, s, p); return check_launch(what); };
  switch (l.form) {
    case TR_ONE_SHOT: return go(mxfp4_transpose_mxfp8_kernel<128, 128>, "mxfp4_transpose_mxfp8_kernel");
#if QAMD_BENCH
    case TR_NC256: return go(mxfp4_transpose_mxfp8_kernel<256>, "mxfp4_transpose_mxfp8_kernel");
    case TR_MR256: return go(mxfp4_transpose_mxfp8_kernel<128, 256>, "mxfp4_transpose_mxfp8_kernel");
    case TR_WAVE4: return go(mxfp4_transpose_mxfp8_tw_kernel<4>, "mxfp4_transpose_mxfp8_tw_kernel");
    case TR_WAVE2: return go(mxfp4_transpose_mxfp8_tw_kernel<2>, "mxfp4_transpose_mxfp8_tw_kernel");
    case TR_PP4: case TR_PP3: case TR_PP2: case TR_PP6: return go(mxfp4_transpose_mxfp8_pp_kernel<128, 128>, "mxfp4_transpose_mxfp8_pp_kernel");   // (one kernel; the forms differ in the grid)
#endif
  }
  return fail(QAMD_ERR_INVALID, "%s: this build holds no kernel for form %d", name, l.form);
}

int qutlass_amd_backward_bf16_square_double_mxfp8_rows(const void* x, int64_t m, int64_t m_pad, int64_t n, void* y, void* row_scales,
                                                       void* col_scales, void* stream) {
  const char* name = "backward_bf16_square_double_mxfp8";
  if (const int rc = rows_check(name, 128, "n a positive multiple of 128", !x || !y || !row_scales || !col_scales, m, m_pad, n)) return rc;
  SqParams p;
  p.x = (const uint16_t*)x; p.y = (uint8_t*)y; p.row_sf = (uint8_t*)row_scales; p.col_sf = (uint8_t*)col_scales;
  p.m = (int)m; p.n = (int)n; p.m_pad = (int)m_pad; p.abl = opt_bwd_variant() >> 4;
  return launch_square_double(name, p, stream_launch_plan(OP_SQ, m_pad, n, 0, chip_cus(), opt_transpose_nc(), false), (hipStream_t)stream);
}

int qutlass_amd_backward_bf16_square_double_mxfp8(const void* x, int64_t m, int64_t n, void* y, void* row_scales,
                                                  void* col_scales, void* stream) {
  if (m > 0 && m % 128) return fail(QAMD_ERR_INVALID, "backward_bf16_square_double_mxfp8: m and n must be positive multiples of 128 (got m=%lld n=%lld)", (long long)m, (long long)n);
  return qutlass_amd_backward_bf16_square_double_mxfp8_rows(x, m, m, n, y, row_scales, col_scales, stream);
}

int qutlass_amd_mxfp4_transpose_mxfp8_rows(const void* x_fp4, const void* scales, int64_t m, int64_t m_pad, int64_t n, void* y,
                                           void* out_e8m0, void* stream) {
  const char* name = "mxfp4_transpose_mxfp8";
  if (const int rc = rows_check(name, 256, "n % 256 == 0", !x_fp4 || !scales || !y || !out_e8m0, m, m_pad, n)) return rc;
  TrParams p;
  p.xq = (const uint8_t*)x_fp4; p.xs = (const uint8_t*)scales; p.y = (uint8_t*)y; p.out_sf = (uint8_t*)out_e8m0;
  p.m = (int)m; p.n = (int)n; p.m_pad = (int)m_pad; p.abl = opt_bwd_variant() >> 4;
  return launch_transpose(name, p, stream_launch_plan(OP_TR, m_pad, n, 0, chip_cus(), opt_transpose_nc(), false), (hipStream_t)stream);
}

int qutlass_amd_mxfp4_transpose_mxfp8(const void* x_fp4, const void* scales, int64_t m, int64_t n, void* y,
                                      void* out_e8m0, void* stream) {
  if (m > 0 && m % 128) return fail(QAMD_ERR_INVALID, "mxfp4_transpose_mxfp8: need m %% 128 == 0 and n %% 256 == 0 (got m=%lld n=%lld)", (long long)m, (long long)n);
  return qutlass_amd_mxfp4_transpose_mxfp8_rows(x_fp4, scales, m, m, n, y, out_e8m0, stream);
}

int qutlass_amd_to_blocked(const void* in, int64_t rows, int64_t cols, void* out, void* stream) {
  if (!in || !out) return fail(QAMD_ERR_INVALID, "to_blocked: null pointer argument");
  if (rows <= 0 || cols <= 0 || rows >= (1ll << 31) || cols >= (1ll << 31))
    return fail(QAMD_ERR_INVALID, "to_blocked: bad shape (%lld, %lld)", (long long)rows, (long long)cols);
  BlockedParams p;
  p.in = (const uint8_t*)in; p.out = (uint8_t*)out; p.rows = (int)rows; p.cols = (int)cols;
  p.RB = (int)cdiv(rows, 128); p.CB = (int)cdiv(cols, 4);
  // columns per workgroup: the widest slab that still gives every CU a workgroup
  int tc = 128;
  while (tc > 16 && (int64_t)p.RB * cdiv(p.CB, tc / 4) < chip_cus()) tc >>= 1;
  const int64_t grid = (int64_t)p.RB * cdiv(p.CB, tc / 4);
  if (grid >= (1ll << 31)) return fail(QAMD_ERR_INVALID, "to_blocked: matrix too large");
  switch (tc) {
    case 128: hipLaunchKernelGGL(to_blocked_kernel<128>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p); break;
    case 64: hipLaunchKernelGGL(to_blocked_kernel<64>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p); break;
    case 32: hipLaunchKernelGGL(to_blocked_kernel<32>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(to_blocked_kernel<16>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p); break;
  }
  return check_launch("to_blocked_kernel");
}

// debug only (not declared in the public header): which kernels would matmul_mx{f4,f8}_bf16_tn(_ws) launch for this shape on a 256-CU part?
// out[3 * i + {0, 1, 2}] = {gemm_variant, N of the launch, K splits} of launch i; returns the number of launches (the split-K
// reduce pass is implied by splits > 1), or -1 when the arguments are rejected.  No GPU is touched.
int qutlass_amd_debug_gemm_plan(int ebits, int64_t M, int64_t N, int64_t K, int64_t workspace_bytes, int* out, int cap) {
  alignas(16) static char dummy[16];
  const char* name = "debug_gemm_plan";
  if ((ebits != 4 && ebits != 8) || mx_check(name, ebits, dummy, dummy, dummy, dummy, (const float*)dummy, dummy, M, N, K)) return -1;
  const int64_t avail = std::max<int64_t>(workspace_bytes, 0);
  return debug_plan(name, M, N, K * ebits / 8, 256, out, cap, [&](int64_t m, int64_t n) {
    return ebits == 4 ? mx_plan<4>(0, m, n, K, N, avail, 256) : mx_plan<8>(0, m, n, K, N, avail, 256);
  });
}

// debug only (not declared in the public header): MX_FORMS, nine ints per row in the order of MxFormRow's fields; writes the first min(cap / 9, rows) rows, returns the row count
int qutlass_amd_debug_mx_forms(int* out, int cap) {
  for (int i = 0; i < MX_NFORMS && 9 * (i + 1) <= cap; ++i) {
    const MxFormRow& f = MX_FORMS[i];
    const int row[9] = {f.variant, f.family, f.tm, f.tn, f.wm, f.wn, f.depth, f.ops, (int)f.product};
    std::copy(row, row + 9, out + 9 * i);
  }
  return MX_NFORMS;
}

// debug only (not declared in the public header): the same for matmul_ada_mxf4_bf16_tn (ada_plan; K splits are always 1)
int qutlass_amd_debug_ada_plan(int64_t M, int64_t N, int64_t K, int* out, int cap) {
  alignas(16) static char dummy[16];
  const char* name = "debug_ada_plan";
  if (ada_check(name, dummy, dummy, dummy, dummy, (const float*)dummy, dummy, M, N, K)) return -1;
  return debug_plan(name, M, N, K / 2, 64, out, cap, [&](int64_t m, int64_t n) { return MxPlan().add(ada_plan(m, n, K, 256), 0, n); });
}

// [r4] debug only (not declared in the public header): the form (quartet_bwd.hip.h StreamForm) the product rules pick on a 256-CU part, no GPU touched.  op 0 / 1: backward_t_bf16 /
// backward_qt_bf16 (a, b, c) = (B, N, M) -> 1, 3 / 1, 2, 5; op 2: backward_bf16_square_double_mxfp8 (a, b) = (m_pad, n) -> column tiles per workgroup (1 or 4)
int qutlass_amd_debug_stream_plan(int op, int64_t a, int64_t b, int64_t c) {
  if (op == OP_T || op == OP_QT) return (a <= 0 || b <= 0 || c <= 0 || b % 32) ? -1 : stream_launch_plan(op, a, b, c, 256, 0, true).form;
  if (op == OP_SQ) return (a <= 0 || b <= 0 || a % 128 || b % 128) ? -1 : stream_launch_plan(op, a, b, 0, 256, 0, false).form;
  return -1;
}

// debug only (not declared in the public header): the whole launch of the four ops (stream_launch_plan, the function their entries run) on a part of `cus` CUs, after the entry's
// own argument checks, no GPU touched.  op 0 / 1: (a, b, c) = (B, N, M); op 2 / 3 = the _rows forms of square-double / the transposer: (a, b, c) = (m_pad, n, m).  variant: the lab's
// "bwd_variant" (low 4 bits) / "transpose_nc", 0 = the product rules; ring_aligned: what backward_qt_bf16 finds of its operands' addresses.  out[0 .. 2] = {form, workgroups,
// threads per workgroup}; returns 1, or -1 for arguments the op rejects and for a form this build holds no kernel for (the product library: any variant but 0).
int qutlass_amd_debug_stream_launch_plan(int op, int64_t a, int64_t b, int64_t c, int cus, int variant, int ring_aligned, int* out) {
  const char* name = "debug_stream_launch_plan";
  if (!out || cus <= 0 || op < OP_T || op > OP_TR || (op <= OP_QT ? bwd_check(name, op == OP_QT ? 32 : 8, false, a, b, c) : rows_check(name, op == OP_SQ ? 128 : 256, "", false, c, a, b))) return -1;
  const StreamLaunch l = stream_launch_plan(op, a, b, c, cus, variant, ring_aligned != 0);
  if (l.form == SF_NONE) return -1;
  out[0] = l.form; out[1] = (int)l.grid; out[2] = l.threads;
  return 1;
}

// debug only (not declared in the public header): the launch plans of the ops around the grouped GEMMs on a part of `cus` CUs -- the functions their entries run -- after the entries'
// own checks of these arguments, no GPU touched.  Returns the number of ints written to out, or -1: an argument the op rejects, no such op, cus <= 0, a null out, cap too small.
//   op 0  row_stream_plan (silu_and_mul, swiglu_oai_and_mul, both moe_combine forms): a = chunks > 0 -> {workgroups, threads};   op 3  fusedq_plan: a = M -> {rows per rotation tile}
//   op 1  moe_topk_plan (both routers): a = elem_bytes, b = E, c = T, plus bit 62 of c when every row's pointers are 16-byte aligned -> {R, vector loads, workgroups, threads}
//   op 5  moe_route_fused_plan (both one-launch routing kernels): op 1's arguments with T <= 64 -> {op 1's R, op 1's vector loads, 1 workgroup, 512 threads}
//   op 2  moe_sort_plan: (a, b, c) = (T * topk, E, the one-launch bound or 0 for the product's) -> {launches, slots per workgroup, rows, workspace bytes};   op 4  activation_path_plan at rot = 32: (M, N, K) -> {launches}
int qutlass_amd_debug_moe_launch_plan(int op, int64_t a, int64_t b, int64_t c, int cus, int* out, int cap) {
  const int64_t t = c & ~(1ll << 62);
  auto put = [&](std::initializer_list<int64_t> v) { return (int)v.size() <= cap ? (std::copy(v.begin(), v.end(), out), (int)v.size()) : -1; };
  if (!out || cus <= 0) return -1;
  if (op == 0 && a > 0) { const RowStreamLaunch l = row_stream_plan(a, cus); return put({l.grid, l.threads}); }
  if (op == 1 && a == (int)a && !topk_check("debug_moe_launch_plan", (int)a, t, b)) { const MoeTopkLaunch l = moe_topk_plan((int)a, b, t, c >> 62 & 1, cus); return put({l.R, l.loadv, l.grid, l.threads}); }
  if (op == 5 && a == (int)a && t <= MOE_ROUTE_FUSED_MAX_T && !topk_check("debug_moe_launch_plan", (int)a, t, b)) { const MoeTopkLaunch l = moe_route_fused_plan((int)a, b, t, c >> 62 & 1); return put({l.R, l.loadv, l.grid, l.threads}); }
  if (op == 2 && a >= 0 && a < (1ll << 31) && b >= 1 && b <= 1024 && c >= 0) { const MoeSortLaunch l = moe_sort_plan(a, b, c); return put({l.launches, l.spb, l.rows, l.ws_bytes}); }
  if (op == 3 && a >= 1 && a <= 32) return put({fusedq_plan(a)});
  return op == 4 ? put({activation_path_plan(a, b, c, 32, cus)}) : -1;
}

// [r4] debug only (not declared in the public header): the grouped-raster decode of the persistent kernels (common.hip.h raster_decode, the SAME function the
// device runs, with the host's raster_magic) for tiles [t0, t0 + n) of a tiles_m x tiles_n grid: out[2 i] = tile row, out[2 i + 1] = tile column.  No GPU touched.
int qutlass_amd_debug_raster_decode(int tiles_m, int tiles_n, int t0, int n, int* out) {
  if (!out || tiles_m <= 0 || tiles_n <= 0 || t0 < 0 || n < 0) return -1;
  const uint32_t magic = qamd::raster_magic(tiles_n);
  for (int i = 0; i < n; ++i) qamd::raster_decode(t0 + i, tiles_m, tiles_n, magic, out[2 * i], out[2 * i + 1]);
  return n;
}

// debug only (not declared in the public header): the tile decode of grouped_matmul_mxf4_bf16_tn (gemm_mx_grouped.hip.h grouped_tile, the SAME lane functions the
// device runs) for workgroups [0, nwg) of TM-row tiles and tiles_n column tiles over host offs[0 .. E): out[4 b .. 4 b + 3] = {expert, first row, rows, column tile} of
// workgroup b ({-1, 0, 0, 0}: no work).  Returns the number of workgroups with work, or -1 when the arguments are rejected.  No GPU touched.
int qutlass_amd_debug_grouped_decode(const int32_t* offs, int E, int M, int TM, int tiles_n, int nwg, int* out) {
  if (!offs || !out || E < 1 || E > qamd::GRP_MAX_E || M < 0 || TM <= 0 || tiles_n <= 0 || nwg < 0) return -1;
  int n = 0;
  for (int b = 0; b < nwg; ++b) {
    qamd::GroupTile t;
    if (qamd::grouped_tile(offs, E, M, TM, tiles_n, b, t)) {
      out[4 * b] = t.g; out[4 * b + 1] = t.row0; out[4 * b + 2] = t.rows; out[4 * b + 3] = t.nt;
      ++n;
    } else {
      out[4 * b] = -1; out[4 * b + 1] = 0; out[4 * b + 2] = 0; out[4 * b + 3] = 0;
    }
  }
  return n;
}

// debug only (not declared in the public header): the expert of operand row m in the grouped-scale quantizers (quantize.hip.h quant_group_of_row, the SAME function
// the two kernels run) over host offs[0 .. E); -1 when the arguments are rejected.  No GPU touched.
int qutlass_amd_debug_group_of_row(const int32_t* offs, int E, int m) {
  if (!offs || E < 1 || E > qamd::QUANT_MAX_E) return -1;
  return qamd::quant_group_of_row(offs, E, m);
}

// debug only (not declared in the public header): the form a grouped op's rule picks on a 256-CU part, after the entry's own argument checks (-1: rejected);
// out[0] (optional) = the workgroups it launches.  No GPU touched.
static int debug_grouped_plan(const GroupedFormat& F, const char* name, GroupedPlan plan, int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  alignas(16) static char dummy[16];
  if (grouped_check(F, name, dummy, dummy, dummy, dummy, (const float*)dummy, 1, (const int32_t*)dummy, dummy, M, N, K, E)) return -1;
  const int v = plan(M, N, K, E, 256);
  if (out) out[0] = M == 0 ? 0 : grouped_grid(F, v, M, N, E);
  return v;
}
// grouped_matmul_mxf4_bf16_tn: 590 = 32x32, 592 = 64x32 tiles of the wave-owned kernel, 593 = the 64x64 ring kernel
int qutlass_amd_debug_grouped_plan(int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  return debug_grouped_plan(GRP_MXF4, "debug_grouped_plan", grouped_plan, M, N, K, E, out);
}
// grouped_matmul_mxf8_bf16_tn: 594 = 32x32 tiles of the wave-owned kernel, 597 = the 64x64 ring kernel
int qutlass_amd_debug_grouped_mxf8_plan(int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  return debug_grouped_plan(GRP_MXF8, "debug_grouped_mxf8_plan", grouped8_plan, M, N, K, E, out);
}
// grouped_matmul_mxf8_mxf4_bf16_tn: 602 = 32x32, 604 = 64x32 tiles of the mixed-width wave-owned kernel
int qutlass_amd_debug_grouped_mxf8_mxf4_plan(int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  return debug_grouped_plan(GRP_MXF8_MXF4, "debug_grouped_mxf8_mxf4_plan", grouped_w4a8_plan, M, N, K, E, out);
}
// grouped_matmul_bf16_mxf4_bf16_tn: 606 = 32x32, 608 = 64x32 tiles of the bf16-token wave-owned kernel
int qutlass_amd_debug_grouped_bf16_mxf4_plan(int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  return debug_grouped_plan(GRP_BF16_MXF4, "debug_grouped_bf16_mxf4_plan", grouped_w4a16_plan, M, N, K, E, out);
}
// grouped_matmul_mxf6_mxf4_bf16_tn: 610 = 32x32, 612 = 64x32 tiles of the 6-bit-token wave-owned kernel
int qutlass_amd_debug_grouped_mxf6_mxf4_plan(int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  return debug_grouped_plan(GRP_MXF6_MXF4, "debug_grouped_mxf6_mxf4_plan", grouped_w4a6_plan, M, N, K, E, out);
}
// grouped_matmul_nvf4_bf16_tn: 598 / 599 = 32x32 / 64x32 tiles of the wave-owned kernel, 600 / 601 = 64x64 / 128x128 tiles of the tile kernel
int qutlass_amd_debug_grouped_nvf4_plan(int64_t M, int64_t N, int64_t K, int64_t E, int64_t* out) {
  return debug_grouped_plan(GRP_NVF4, "debug_grouped_nvf4_plan", grouped_nv_plan, M, N, K, E, out);
}

// debug only (not declared in the public header): what matmul_nvf4_bf16_tn's rule picks for an M x N x K problem (gemm_nvf4.hip.h: nvf4_plan; 256 CUs assumed,
// no GPU touched): the tile configuration (-1 skinny, 0 256x256, 1 128x128, 2 128x64, 3 64x64, 4 256x128), plus 256 x the number of K ranges when may_split
// (= the caller passes a workspace) and the shape splits
int qutlass_amd_debug_nvf4_plan(int64_t M, int64_t N, int64_t K, int may_split) {
  if (M <= 0 || N <= 0 || K <= 0) return -2;
  const qamd::NvPlan pl = qamd::nvf4_plan(M, N, K, 256, may_split != 0);
  return pl.splits > 1 ? pl.cfg + 256 * pl.splits : pl.cfg;
}

// debug only (not declared in the public header): which kernels would matmul_nvf4_bf16_tn(_ws) launch for this shape on a 256-CU part?
// out[6 * i + {0 ... 5}] = {form (gemm_nvf4.hip.h NvForm), columns, rows, K ranges, stages per range, workgroups} of launch i (the first min(cap, 8)); returns the
// number of launches (the reduce pass is implied by K ranges > 1), or -1 when the arguments are rejected.  No GPU is touched.
int qutlass_amd_debug_nvf4_launch_plan(int64_t M, int64_t N, int64_t K, int64_t workspace_bytes, int* out, int cap) {
  alignas(16) static char dummy[16];
  const char* name = "debug_nvf4_launch_plan";
  if (gemm_check(name, 16, 32, false, dummy, dummy, dummy, dummy, (const float*)dummy, dummy, M, N, K)) return -1;
  int cnt = 0;
  const int rc = nv_for_each_launch(name, M, N, K, std::max<int64_t>(workspace_bytes, 0), 256, [&](int64_t, int64_t, int64_t m, int64_t n, const qamd::NvLaunch& l) {
    if (cnt < 8 && cnt < cap) {
      const int v[6] = {l.form, (int)n, (int)m, l.splits, l.kt_per, (int)l.grid};
      std::copy(v, v + 6, out + 6 * cnt);
    }
    ++cnt;
    return QAMD_OK;
  });
  return rc == QAMD_OK ? cnt : -1;
}

// [r4] the persistent NVFP4 kernel's plan on a 256-CU part: out[0] = workgroups, out[1] = tiles in the stream-K region (0: whole tiles only),
// out[2] = K stages per tile; returns 0 when the shape does not run the persistent kernel (tile configuration other than 256x256, K % 256, K < 512)
int qutlass_amd_debug_nvf4_pk_plan(int64_t M, int64_t N, int64_t K, int may_sk, int* out) {
  if (!out || M <= 0 || N <= 0 || K < 32) return 0;
  const qamd::NvPlan pl = qamd::nvf4_plan(M, N, K, 256, may_sk != 0);
  if (pl.cfg != 0 || !qamd::nvpk_shape_ok(M, N, K)) return 0;
  const qamd::NvPkPlan pk = qamd::nvpk_plan(M, N, K, 256, may_sk != 0);   // may_sk: what the LAB's stream-K variant would walk (the product never cuts tiles)
  out[0] = pk.grid; out[1] = pk.sk_tiles; out[2] = (int)(K / 256);
  return 1;
}
// the units workgroup w of `grid` walks over T tiles (the last sk_tiles as a stream of K stages), KT stages per tile: 5 ints per unit
// {tile, first stage, end stage, mode, slot} into out[0 .. 5 cap); returns the number of units (the device kernel runs the same NvPkWalk)
// gran: stage granularity of a range boundary (1: NVFP4 kernel, 2: the MX kernels)
int qutlass_amd_debug_sk_units(int w, int grid, int T, int sk_tiles, int KT, int gran, int* out, int cap) {
  if (!out || grid <= 0 || w < 0 || w >= grid || KT < 2 || sk_tiles < 0 || sk_tiles > T) return -1;
  qamd::SkWalk walk(w, grid, T, sk_tiles, KT, 2, gran);
  int n = 0;
  for (;;) {
    const qamd::SkUnit u = walk.next();
    if (u.mode < 0) break;
    if (n < cap) { out[5 * n] = u.tile; out[5 * n + 1] = u.kb; out[5 * n + 2] = u.ke; out[5 * n + 3] = u.mode; out[5 * n + 4] = u.slot; }
    ++n;
  }
  return n;
}
int qutlass_amd_debug_nvf4_pk_units(int w, int grid, int T, int sk_tiles, int KT, int* out, int cap) { return qutlass_amd_debug_sk_units(w, grid, T, sk_tiles, KT, 1, out, cap); }

#if QAMD_BENCH
// lab library only: device buffer for ABL_TRACE / ABL_CLOCK builds
void qutlass_amd_debug_set_trace_buffer(void* p) { g_dbg.store((uint32_t*)p); }
#endif

const char* qutlass_amd_last_error(void) { return g_err; }
#if QAMD_BENCH
const char* qutlass_amd_version(void) { return "qutlass_amd 0.2.0 (gfx950, lab build)"; }
#else
const char* qutlass_amd_version(void) { return "qutlass_amd 0.2.0 (gfx950)"; }
#endif

// Product library: knows NO key (every call returns -1) -- nothing a caller or another thread does can change which kernel runs or what it computes.
// The lab library accepts the tuning / variant keys its benches use, and "hw_fp4_cvt" (0 = the software e2m1 encoder, bit-identical to the hardware
// convert the product ships: tests/test_gpu_parity.py runs the quantizer goldens under both through the lab build).
int qutlass_amd_set_option(const char* key, int value) {
  if (!key) return -1;
  (void)value;
#if QAMD_BENCH
  if (!strcmp(key, "hw_fp4_cvt")) return g_hw_fp4_cvt.exchange(value);
  if (!strcmp(key, "gemm_variant")) return g_gemm_variant.exchange(value);
  if (!strcmp(key, "nvf4_variant")) return g_nvf4_variant.exchange(value);
  if (!strcmp(key, "transpose_nc")) return g_transpose_nc.exchange(value);
  if (!strcmp(key, "splitk_wg")) return g_splitk_wg.exchange(value);
  if (!strcmp(key, "splitk_min_kt")) return g_splitk_min_kt.exchange(value);
  if (!strcmp(key, "splitk_force")) return g_splitk_force.exchange(value);
  if (!strcmp(key, "deepp_grid")) return g_deepp_grid.exchange(value);
  if (!strcmp(key, "bwd_variant")) return g_bwd_variant.exchange(value);
  if (!strcmp(key, "quant_wg_per_cu")) return g_quant_wg_per_cu.exchange(value);
  if (!strcmp(key, "moe_sort_one_launch_max")) return g_moe_sort_one_launch_max.exchange(value);
  if (!strcmp(key, "pp_shift")) return g_pp_shift.exchange(value);
  if (!strcmp(key, "pp_flags")) return g_pp_flags.exchange(value);
#endif
  return -1;
}

}  // extern "C"
#pragma GCC visibility pop
#endif   // QAMD_DEF(1)
