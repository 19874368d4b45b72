// Does the scaled FP4 MFMA cost fewer joules per flop in its 16x16x128 shape than in its 32x32x64 shape?  (test / bench infrastructure, own main();
// modelled on energy_ubench.hip, which stays as it is.)
// The 4096^3 launch sits at the socket power cap, two thirds of its joules are MFMAs, and every MFMA form priced so far was a 32x32x64 one.  The only older
// figure for the 16x16x128 shape (ubench.hip mode 26) credits half the flops its loop issues and its accumulators get merged by the compiler, so it is no rate.
// This file runs both shapes in ONE process, interleaved, on the same quantised-Gaussian e2m1 codes, every CU busy (256 workgroups x 4 waves, one wave per
// SIMD), socket power sampled through librocm_smi64 (smi_sampler.h) while one kernel runs back to back for ~0.7 s per line:
//   mode 0 (a)  MFMA only: a 128x128 wave tile over K = 256 per iteration (one K stage of the GEMM) = 64 MFMAs of 32x32x64 or 128 of 16x16x128, every
//               MFMA on its own accumulator (256 accumulator registers), fragments and scale operands held in registers;
//   mode 1 (b)  (a) + the fragment reads of that stage: 32 ds_read_b128 per wave and iteration in either shape (16 per 64 MFMAs of 16x16x128 -- the same
//               LDS bytes per MAC), each landing in the registers the NEXT k-slice's MFMAs take;
//   mode 2 (c)  (b) + LDS-DMA: 16 pieces of 1 KiB per wave and iteration (2 KiB per 8 MFMAs of 32x32x64, as ubench mode 4; 64 KiB per workgroup = the
//               GEMM's K stage), source = the workgroup's own 64 KiB (L2 hits);
//   mode 3 (d)  (c) + what each shape has to do for its scale operands in a GEMM's K stage.  32x32x64: 2 ds_read_b128 (a lane's four row dwords per operand are
//               one 16-byte line of the to_blocked image; op_sel picks the byte).  16x16x128: 8 ds_read_b128 and 32 shifts (the lane's scale byte is byte
//               lane >> 4 of the row's dword: the dword shifted right by 8 (lane >> 4), op_sel 0).  This is the whole instruction mix of a K stage.
// Per line: ns per iteration, cycles per MFMA (in-kernel s_memtime around the loop), in-kernel clock (s_memtime / s_memrealtime), TFLOP/s from the MFMAs the
// loop holds (MFMAS x 256 workgroups x 4 waves -- check the count in the ISA, `hipcc -S`: the loop between the two s_memtime holds one stage of 128 MFMAs
// of 16x16x128, or two stages = 128 MFMAs of 32x32x64, each with vdst == srcC and no accumulator copy), socket W, MHz as
// rocm_smi reports it, pJ/flop above the idle socket.  The last lines compare the two shapes per mode against the spread between repeats of one shape.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 energy_ubench16.hip -o energy_ubench16 -lrocm_smi64
//   ./energy_ubench16 [seconds per line = 0.7] [repeats = 2]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "smi_sampler.h"

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP ERROR %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2);} } while (0)

constexpr int WGS = 256, OFF_SC = 128 * 1024, LDS_BYTES = OFF_SC + 4096, SRC_PER_WG = 64 * 1024;

struct Args {
  const uint32_t* codes;   // 64 KiB of e2m1 codes (quantised Gaussian, or zeros): the LDS image the fragments come from
  const uint32_t* scales;  // 1024 dwords of e8m0 bytes
  const char* src;         // DMA source, SRC_PER_WG bytes per workgroup
  uint32_t src_bytes;
  float* out;
  uint64_t* stamps;        // per workgroup: cycles (s_memtime) and 100-MHz ticks (s_memrealtime) around the loop -- read by the host only
  int iters;
};

// LDS image: A = 256 rows x 128 B at 0, B = 256 rows x 128 B at 32 KiB, 16-byte chunk c of row r stored at chunk c ^ ((r >> 1) & 7) -- the GEMM's swizzle.
// Behind the DMA landing area (64 KiB .. 128 KiB) lies a scale image in the to_blocked order of one K stage: per operand (A at 0, B at 2 KiB) and 128-K column
// tile (512 B) the dword of row r sits at (r & 31) * 16 + (r >> 5) * 4, so one ds_read_b128 at (r & 31) * 16 fetches the dwords of rows r, r + 32, r + 64, r + 96.
// The fragment image serves both accesses without a bank conflict (checked on the host below, against the ds_read_b128 lane groups):
//   32x32x64:  lane l reads row 32 t + (l & 31), chunk 4 (l >> 5) + j   for k-slice j = 0..3;
//   16x16x128: lane l reads row 16 t + (l & 15), chunk 4 h + (l >> 4)   for half h = 0, 1 of the stage.
template <int SHAPE, int MODE>
__global__ __launch_bounds__(256) void eu16_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < 64 * 1024 / 4; i += 256) ((uint32_t*)smem)[i] = a.codes[(i + blockIdx.x * 977) & 16383];
  for (int i = tid; i < 1024; i += 256) ((uint32_t*)(smem + OFF_SC))[i] = a.scales[i];
  __syncthreads();
  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.src), 0, a.src_bytes, 0x00020000);
  const int vdma = (int)(blockIdx.x * (uint32_t)SRC_PER_WG + (uint32_t)wave * 16384u + lane * 16);
  auto dma = [&](const int q) __attribute__((always_inline)) {   // piece q of this wave's 16 KiB share of the stage; lands behind the fragment image
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(smem + 65536 + (wave * 16 + q) * 1024), 16, vdma, q * 1024, 0, 0);
  };
  float sink = 0.f;
  uint64_t c0 = 0, c1 = 0, r0 = 0, r1 = 0;

  if constexpr (SHAPE == 32) {
    const int sw = ((lane & 31) >> 1) & 7;
    int base[4];
    for (int j = 0; j < 4; ++j) base[j] = (lane & 31) * 128 + (((4 * (lane >> 5) + j) ^ sw) << 4);
    v16f acc[4][4];
    for (int m = 0; m < 4; ++m) for (int n = 0; n < 4; ++n) for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    v4i fa[4][4], fb[4][4];
    for (int j = 0; j < 4; ++j)
      for (int t = 0; t < 4; ++t) {
        fa[j][t] = *(const v4i*)(smem + base[j] + t * 4096);
        fb[j][t] = *(const v4i*)(smem + 32768 + base[j] + t * 4096);
      }
    // scale dwords: lane group g = lane >> 5 holds K-block 4 g + j in k-slice j, so its dword is the row's dword of column tile g, byte j picked by op_sel.
    // Two sets, as the GEMM keeps them (a stage reads the next stage's while every MFMA of its own still needs the current ones).
    int scb = OFF_SC + (lane >> 5) * 512 + (lane & 31) * 16;
    v4i sa[2], sb[2];
    for (int P = 0; P < 2; ++P) { sa[P] = *(const v4i*)(smem + scb); sb[P] = *(const v4i*)(smem + scb + 2048); }
    auto mf = [&](const int P, const int j, const int m, const int n) __attribute__((always_inline)) {
      const v4i x = fa[j][m], y = fb[j][n];
      const v8i A8 = {x[0], x[1], x[2], x[3], 0, 0, 0, 0}, B8 = {y[0], y[1], y[2], y[3], 0, 0, 0, 0};
      if (j == 0) acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B8, A8, acc[m][n], 4, 4, 0, sb[P][n], 0, sa[P][m]);
      if (j == 1) acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B8, A8, acc[m][n], 4, 4, 1, sb[P][n], 1, sa[P][m]);
      if (j == 2) acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B8, A8, acc[m][n], 4, 4, 2, sb[P][n], 2, sa[P][m]);
      if (j == 3) acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B8, A8, acc[m][n], 4, 4, 3, sb[P][n], 3, sa[P][m]);
    };
    // every operand has arrived before the loop: no wait on these loads is left for the compiler to place inside it
    for (int j = 0; j < 4; ++j) for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(fa[j][t]), "+v"(fb[j][t]));
    for (int P = 0; P < 2; ++P) asm volatile("" : "+v"(sa[P]), "+v"(sb[P]));
    auto stage = [&](const int P) __attribute__((always_inline)) {   // one K stage; P = its parity = its scale set
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(base[j]));   // the reads of a stage are this stage's: nothing is hoisted out of the loop
      asm volatile("" : "+v"(scb));
      fence();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int jn = (j + 1) & 3;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          mf(P, j, i >> 2, i & 3);
          fence();
          if (MODE == 3 && j == 2 && (i == 8 || i == 9)) {   // the next stage's scale dwords: one ds_read_b128 per operand (the GEMM's place for them)
            if (i == 8) sa[P ^ 1] = *(const v4i*)(smem + scb); else sb[P ^ 1] = *(const v4i*)(smem + scb + 2048);
            fence();
          }
          if (MODE >= 1 && i < 8) {   // 8 reads per k-slice, one behind each of its first 8 MFMAs: the next slice's fragments (taken >= 8 MFMAs = 256 cycles later)
            const int k = i;
            if (k < 4) fa[jn][k] = *(const v4i*)(smem + base[jn] + k * 4096);
            else fb[jn][k - 4] = *(const v4i*)(smem + 32768 + base[jn] + (k - 4) * 4096);
            fence();
          }
          if (MODE >= 2 && (i & 3) == 2) { dma(j * 4 + (i >> 2)); fence(); }   // 4 pieces per k-slice: 2 KiB per 8 MFMAs
        }
      }
      if (MODE >= 2) { asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); fence(); }   // two stages of pieces in flight, like the GEMM
    };
    __syncthreads();
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < a.iters; it += 2) { stage(0); stage(1); }   // (iters is even; the loop body holds TWO stages = 128 MFMAs)
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    for (int m = 0; m < 4; ++m) for (int n = 0; n < 4; ++n) for (int r = 0; r < 16; ++r) sink += acc[m][n][r];
  } else {
    const int r16 = lane & 15, kq = lane >> 4, sw = (r16 >> 1) & 7;
    int base[2];
    for (int h = 0; h < 2; ++h) base[h] = r16 * 128 + (((4 * h + kq) ^ sw) << 4);
    v4f acc[8][8];
    for (int m = 0; m < 8; ++m) for (int n = 0; n < 8; ++n) acc[m][n] = v4f{0.f, 0.f, 0.f, 0.f};
    v4i fa[2][8], fb[2][8];
    for (int h = 0; h < 2; ++h)
      for (int t = 0; t < 8; ++t) {
        fa[h][t] = *(const v4i*)(smem + base[h] + t * 2048);
        fb[h][t] = *(const v4i*)(smem + 32768 + base[h] + t * 2048);
      }
    // scale operands: half h is column tile h; one dword per row and 128 K, the lane's byte is byte kq: the dword shifted right by 8 kq, op_sel 0.
    // Rows 16 t + r16 = 32 (t >> 1) + 16 (t & 1) + r16: the read at row 16 p + r16 brings the dwords of t = p, p + 2, p + 4, p + 6 -- two reads per operand and half.
    int scb = OFF_SC + r16 * 16, sh = 8 * kq;
    v4i raw[4];   // A p = 0, A p = 1, B p = 0, B p = 1
    int xa[2][8], xb[2][8];
    for (int h = 0; h < 2; ++h)
      for (int p = 0; p < 2; ++p) {
        const v4i ra = *(const v4i*)(smem + scb + h * 512 + p * 256), rb = *(const v4i*)(smem + scb + 2048 + h * 512 + p * 256);
        for (int k = 0; k < 4; ++k) { xa[h][p + 2 * k] = (int)((unsigned)ra[k] >> sh); xb[h][p + 2 * k] = (int)((unsigned)rb[k] >> sh); }
      }
    for (int h = 0; h < 2; ++h) for (int t = 0; t < 8; ++t) asm volatile("" : "+v"(fa[h][t]), "+v"(fb[h][t]), "+v"(xa[h][t]), "+v"(xb[h][t]));   // (as above)
    __syncthreads();
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < a.iters; ++it) {
#pragma unroll
      for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(base[h]));
      if (MODE == 3) {   // ... and so are its scale reads and shifts: half 0's operands are the ones the previous iteration shifted, not something to recompute here
        asm volatile("" : "+v"(sh), "+v"(scb));
#pragma unroll
        for (int t = 0; t < 8; ++t) asm volatile("" : "+v"(xa[0][t]), "+v"(xb[0][t]));
      }
      fence();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int hn = h ^ 1;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
          const int m = i >> 3, n = i & 7;
          const v4i x = fa[h][m], y = fb[h][n];
          const v8i A8 = {x[0], x[1], x[2], x[3], 0, 0, 0, 0}, B8 = {y[0], y[1], y[2], y[3], 0, 0, 0, 0};
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(B8, A8, acc[m][n], 4, 4, 0, xb[h][n], 0, xa[h][m]);
          fence();
          if (MODE >= 1 && i < 32 && (i & 1) == 1) {   // 16 reads per half, one behind every second of its first 32 MFMAs: the other half's fragments (taken >= 32 MFMAs = 512 cycles later)
            const int k = i >> 1;
            if (k < 8) fa[hn][k] = *(const v4i*)(smem + base[hn] + k * 2048);
            else fb[hn][k - 8] = *(const v4i*)(smem + 32768 + base[hn] + (k - 8) * 2048);
            fence();
          }
          if (MODE == 3 && i >= 32 && i < 40 && (i & 1) == 1) {   // the other half's scale dwords: 4 ds_read_b128 ...
            const int k = (i - 32) >> 1;
            raw[k] = *(const v4i*)(smem + scb + (k >> 1) * 2048 + hn * 512 + (k & 1) * 256);
            fence();
          }
          if (MODE == 3 && i >= 46 && i < 62) {   // ... and 16 shifts, one behind each of 16 MFMAs
            const int k = i - 46, p = (k >> 2) & 1, q = k & 3;   // raw[k >> 2][q] is row tile t = p + 2 q
            if (k < 8) xa[hn][p + 2 * q] = (int)((unsigned)raw[k >> 2][q] >> sh);
            else xb[hn][p + 2 * q] = (int)((unsigned)raw[k >> 2][q] >> sh);
            fence();
          }
          if (MODE >= 2 && (i & 7) == 4) { dma(h * 8 + (i >> 3)); fence(); }   // 8 pieces per half: 2 KiB per 16 MFMAs = per 8 of 32x32x64
        }
      }
      if (MODE >= 2) { asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); fence(); }
    }
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    for (int m = 0; m < 8; ++m) for (int n = 0; n < 8; ++n) for (int r = 0; r < 4; ++r) sink += acc[m][n][r];
  }
  if (MODE >= 2) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sink += ((float*)smem)[16384 + tid];
  }
  if (tid == 0) { a.stamps[2 * blockIdx.x] = c1 - c0; a.stamps[2 * blockIdx.x + 1] = r1 - r0; }
  if (sink == 12345.678f) a.out[blockIdx.x * 256 + tid] = sink;
}

// 64 KiB image of e2m1 codes: N(0,25^2) values, groups of 32, scale = 2^floor(log2(amax)), q = RTNE_e2m1(3 x / scale)  (as energy_ubench.hip)
static std::vector<uint32_t> gaussian_e2m1_image(size_t bytes, uint32_t seed, std::vector<uint8_t>* scales_out) {
  std::mt19937 rng(seed);
  std::normal_distribution<float> nd(0.f, 25.f);
  std::vector<uint8_t> out(bytes);
  const float grid[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  for (size_t g0 = 0; g0 < bytes * 2; g0 += 32) {
    float x[32], amax = 0.f;
    for (int i = 0; i < 32; ++i) { x[i] = nd(rng); amax = std::max(amax, std::fabs(x[i])); }
    const float e = std::floor(std::log2(amax));
    const float sc = std::exp2(e);
    if (scales_out) scales_out->push_back((uint8_t)(127 + (int)e - 2));
    for (int i = 0; i < 32; ++i) {
      const float v = std::fabs(x[i]) / sc * 3.0f;
      int best = 0;
      for (int c = 1; c < 8; ++c) if (std::fabs(v - grid[c]) < std::fabs(v - grid[best]) || (std::fabs(v - grid[c]) == std::fabs(v - grid[best]) && !(c & 1))) best = c;
      const uint8_t code = (uint8_t)(best | (x[i] < 0 ? 8 : 0));
      const size_t el = g0 + i;
      if (el & 1) out[el >> 1] |= (uint8_t)(code << 4); else out[el >> 1] = code;
    }
  }
  std::vector<uint32_t> w(bytes / 4);
  memcpy(w.data(), out.data(), bytes);
  return w;
}

// Worst number of lanes of one ds_read_b128 lane group on one 16-byte slot of the 256-byte bank row (1 = conflict-free), over every read of a stage.
static int worst_bank_multiplicity(int shape) {
  static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  int worst = 0;
  for (int s = 0; s < (shape == 32 ? 4 : 2); ++s)
    for (auto& g : groups) {
      int cnt[16] = {0};
      for (int l : g) {
        const int row = shape == 32 ? (l & 31) : (l & 15), c = shape == 32 ? 4 * (l >> 5) + s : 4 * s + (l >> 4);
        const int addr = row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
        worst = std::max(worst, ++cnt[(addr >> 4) & 15]);
      }
    }
  return worst;
}

static double g_idle_w = 0;
struct Line { int shape, mode; double tflops, pj_dyn, cyc_per_mfma; };
static std::vector<Line> g_lines;

template <int SHAPE, int MODE>
static void run(SmiSampler& smi, const char* data, Args a, double seconds) {
  constexpr int MFMAS = SHAPE == 32 ? 64 : 128;                                     // per wave and iteration
  constexpr double FLOP_MFMA = SHAPE == 32 ? 2.0 * 32 * 32 * 64 : 2.0 * 16 * 16 * 128;
  const double flop_iter = FLOP_MFMA * MFMAS * 4 * WGS;                             // whole chip per iteration
  static const char* names[4] = {"(a) MFMA only", "(b) + 32 ds_read_b128", "(c) + 16 KiB LDS-DMA per wave", SHAPE == 32 ? "(d) (c) + 2 scale reads" : "(d) (c) + 8 scale reads, 32 shifts"};
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&eu16_kernel<SHAPE, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  auto launch = [&] { eu16_kernel<SHAPE, MODE><<<WGS, 256, LDS_BYTES>>>(a); };
  a.iters = 200;   // calibrate iters so that one launch takes ~2 ms
  launch(); launch();
  HIP_OK(hipEventRecord(e0, 0));
  launch();
  HIP_OK(hipEventRecord(e1, 0)); HIP_OK(hipEventSynchronize(e1));
  float ms0; HIP_OK(hipEventElapsedTime(&ms0, e0, e1));
  a.iters = std::max(200, (int)(200 * 2.0 / std::max(ms0, 1e-3f))) & ~1;
  const auto t_begin = std::chrono::steady_clock::now();
  auto el = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
  while (el() < seconds * 0.4) {   // ramp: the power controller settles within ~100 ms
    for (int i = 0; i < 8; ++i) launch();
    HIP_OK(hipDeviceSynchronize());
  }
  const double a_ms = smi.now_ms();
  HIP_OK(hipEventRecord(e0, 0));
  long n = 0;
  while (el() < seconds) {
    for (int i = 0; i < 8; ++i) launch();
    n += 8;
    HIP_OK(hipStreamSynchronize(0));
  }
  HIP_OK(hipEventRecord(e1, 0)); HIP_OK(hipEventSynchronize(e1));
  const double b_ms = smi.now_ms();
  float ms; HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  double w, mhz; int ns;
  smi.mean(a_ms + 20, b_ms, w, mhz, ns);
  std::vector<uint64_t> st(2 * WGS);   // the last launch's stamps: median over workgroups
  HIP_OK(hipMemcpy(st.data(), a.stamps, st.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> cyc(WGS), clk(WGS);
  for (int i = 0; i < WGS; ++i) { cyc[i] = (double)st[2 * i]; clk[i] = st[2 * i + 1] ? (double)st[2 * i] / (double)st[2 * i + 1] * 100.0 : 0.0; }
  std::nth_element(cyc.begin(), cyc.begin() + WGS / 2, cyc.end());
  std::nth_element(clk.begin(), clk.begin() + WGS / 2, clk.end());
  const double cyc_mfma = cyc[WGS / 2] / ((double)a.iters * MFMAS);
  const double ns_iter = ms * 1e6 / ((double)n * a.iters);
  const double tflops = flop_iter / ns_iter * 1e-3, pj = w * ns_iter * 1e3 / flop_iter, pj_dyn = (w - g_idle_w) * ns_iter * 1e3 / flop_iter;
  printf("ENERGY16 %-8s %2dx%2dx%-3d %-30s %4d MFMAs/iter  %8.1f ns/iter  %6.2f cyc/MFMA  %5.0f MHz in-kernel  %6.0f TFLOP/s  %6.0f W  %5.0f MHz smi  %.4f pJ/flop (%.4f above idle)  (%d samples)\n",
         data, SHAPE, SHAPE, SHAPE == 32 ? 64 : 128, names[MODE], MFMAS, ns_iter, cyc_mfma, clk[WGS / 2], tflops, w, mhz, pj, pj_dyn, ns);
  fflush(stdout);
  if (!strcmp(data, "gaussian")) g_lines.push_back({SHAPE, MODE, tflops, pj_dyn, cyc_mfma});
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
}

int main(int argc, char** argv) {
  const double sec = argc > 1 ? atof(argv[1]) : 0.7;
  const int reps = argc > 2 ? std::max(2, atoi(argv[2])) : 2;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, 0));
  printf("DEVICE %s CUs=%d\n", prop.gcnArchName, prop.multiProcessorCount);
  printf("BANKS worst lanes per 16-byte slot within a ds_read_b128 lane group, swizzle c ^ ((row >> 1) & 7): 32-row access %d, 16-row access %d (1 = conflict-free)\n",
         worst_bank_multiplicity(32), worst_bank_multiplicity(16));
  std::vector<uint8_t> sc;
  std::vector<uint32_t> codes = gaussian_e2m1_image(65536, 7, &sc);
  std::vector<uint32_t> scw(1024);
  for (int i = 0; i < 1024; ++i) scw[i] = sc[(4 * i) % sc.size()] | sc[(4 * i + 1) % sc.size()] << 8 | sc[(4 * i + 2) % sc.size()] << 16 | (uint32_t)sc[(4 * i + 3) % sc.size()] << 24;
  uint32_t *d_codes, *d_zero, *d_sc; float* d_out; char *d_src, *d_src0; uint64_t* d_st;
  const size_t SRC = (size_t)WGS * SRC_PER_WG;
  HIP_OK(hipMalloc(&d_codes, 65536)); HIP_OK(hipMalloc(&d_zero, 65536)); HIP_OK(hipMalloc(&d_sc, 4096)); HIP_OK(hipMalloc(&d_out, WGS * 256 * 4));
  HIP_OK(hipMalloc(&d_src, SRC)); HIP_OK(hipMalloc(&d_src0, SRC)); HIP_OK(hipMalloc(&d_st, 2 * WGS * 8));
  HIP_OK(hipMemcpy(d_codes, codes.data(), 65536, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_zero, 0, 65536)); HIP_OK(hipMemset(d_src0, 0, SRC));
  HIP_OK(hipMemcpy(d_sc, scw.data(), 4096, hipMemcpyHostToDevice));
  for (size_t o = 0; o < SRC; o += 65536) HIP_OK(hipMemcpyAsync(d_src + o, d_codes, 65536, hipMemcpyDeviceToDevice, 0));   // Gaussian codes everywhere
  HIP_OK(hipDeviceSynchronize());
  SmiSampler smi;
  smi.start();
  std::this_thread::sleep_for(std::chrono::milliseconds(1500));
  { double mhz; int n; smi.mean(300, smi.now_ms(), g_idle_w, mhz, n); printf("IDLE socket %.0f W (%d samples)\n", g_idle_w, n); }
  const Args g{d_codes, d_sc, d_src, (uint32_t)SRC, d_out, d_st, 0}, z{d_zero, d_sc, d_src0, (uint32_t)SRC, d_out, d_st, 0};
  for (int rep = 0; rep < reps; ++rep) {   // the two shapes interleaved, every line `reps` times
    run<32, 0>(smi, "gaussian", g, sec); run<16, 0>(smi, "gaussian", g, sec);
    run<32, 1>(smi, "gaussian", g, sec); run<16, 1>(smi, "gaussian", g, sec);
    run<32, 2>(smi, "gaussian", g, sec); run<16, 2>(smi, "gaussian", g, sec);
    run<32, 3>(smi, "gaussian", g, sec); run<16, 3>(smi, "gaussian", g, sec);
  }
  // all-zero codes: the chip holds its full clock, so this pair ranks the shapes by cycles only (not the yardstick)
  run<32, 2>(smi, "zeros", z, sec); run<16, 2>(smi, "zeros", z, sec);
  smi.finish();

  // per mode: mean TFLOP/s of each shape, the spread between repeats of one shape, and whether the difference clears three times that spread
  for (int mode = 0; mode < 4; ++mode) {
    double mean[2] = {0, 0}, lo[2] = {1e30, 1e30}, hi[2] = {0, 0}, pj[2] = {0, 0}; int cnt[2] = {0, 0};
    for (auto& l : g_lines) if (l.mode == mode) {
      const int s = l.shape == 16;
      mean[s] += l.tflops; pj[s] += l.pj_dyn; lo[s] = std::min(lo[s], l.tflops); hi[s] = std::max(hi[s], l.tflops); ++cnt[s];
    }
    if (!cnt[0] || !cnt[1]) continue;
    for (int s = 0; s < 2; ++s) { mean[s] /= cnt[s]; pj[s] /= cnt[s]; }
    const double spread = std::max(hi[0] - lo[0], hi[1] - lo[1]), diff = mean[1] - mean[0];
    printf("COMPARE mode %d: 32x32x64 %.0f TFLOP/s (%.4f pJ/flop above idle), 16x16x128 %.0f TFLOP/s (%.4f): %+.2f %%, spread between repeats %.2f %% -> %s\n", mode,
           mean[0], pj[0], mean[1], pj[1], 100 * diff / mean[0], 100 * spread / mean[0],
           diff > 3 * spread ? "16x16x128 FASTER by more than 3 x spread" : diff < -3 * spread ? "16x16x128 SLOWER by more than 3 x spread" : "no difference beyond 3 x spread");
  }
  return 0;
}
