// Gate/up grouped W4A8 GEMM with the activation and the MXFP8 quantizer fused into its epilogue, for gfx950 (extensions: grouped_matmul_mxf8_mxf4_silu_mxf8_tn,
// grouped_matmul_mxf8_mxf4_swiglu_oai_mxf8_tn): MXFP8 tokens (e4m3) against the (E, 2 I, K/2) [gate | up] MXFP4 weights of an expert layer, and what leaves the kernel is
// the down GEMM's A operand -- (M, I) e4m3 codes with one e8m0 scale per 32 -- byte for byte what
//   fusedSiluMulQuantizeMxf8 / fusedSwigluOaiQuantizeMxf8 (grouped_matmul_mxf8_mxf4_bf16_tn(...), identity of 32)
// writes; the (M, 2 I) bf16 tensor between the two launches never exists.
//
// A kernel of its own (gemm_mx_os_w4a8.hip.h keeps its code and its names), built on that header's wave-owned K stages: four waves, wave w owns stages w, w + 4, ...
// of 128 K elements, LDS-DMA pieces, v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = 4 (srcA, the weight fragment, e2m1) and blgp = 0 (srcB, the token fragment, e4m3).
// What differs is the tile: a workgroup owns TM rows x 32 ACTIVATION columns n0 .. n0 + 31 -- the 32 gate rows n0 .. of the weight AND the 32 up rows I + n0 .. that go
// with them -- which is exactly one MX scale group of the output, so the quantizer's row statistic never leaves the workgroup.
//   stage     TM x 128 B of A (pieces of 8 rows, 16-byte chunk ^ ((row >> 1) & 7): the W4A8 kernel's), 64 weight rows x 64 B as FOUR 1 KiB pieces (0, 1: gate rows,
//             2, 3: up rows; chunk ^ ((row >> 2) & 3)), one dword piece of A scales and one of B scales (lanes 0-31: the gate rows', lanes 32-63: the up rows').
//             (TM + 32) x 128 B + 512 B: 8.5 KiB for TM = 32, 12.5 KiB for TM = 64.
//   MFMAs     four per m-tile and stage (two K halves x gate / up) on the same token fragment; accumulators 2 MT 16 registers.
//   slots     SPW per wave, 4 SPW stages per workgroup.  LDS = 4 SPW STAGE (at least the sum's scratch, below); a CU has 160 KiB, two workgroups share it up to 80 KiB:
//               TM = 32:  SPW 1  34 KiB (2 / CU)   2  68 KiB (2 / CU)   3  102 KiB (1 / CU)   4  136 KiB (1 / CU)       one shot up to K = 2048, rings of 4 beyond
//               TM = 64:  SPW 1  64 KiB (2 / CU; the scratch)   2  100 KiB (1 / CU)   3  150 KiB (1 / CU)                 one shot up to K = 1536, rings of 3 beyond
//             so K <= 1024 keeps two 32-row workgroups on a CU and K <= 512 two 64-row ones.  K % 128 == 0: no stage has a short tail, any K runs.
//   sum       [wave][TM][64] fp32 in the freed stage area -- a row is 16 chunks of 4 fp32, 0-7 gate, 8-15 up, chunk ^ (row & 15) --, ((w0 + w1) + w2) + w3, one multiply
//             by alpha[g], one rounding to bf16: the GEMM op's output row, bit for bit (same MFMA sequence per accumulator, same order of the four partial sums).
//   epilogue  thread (row = tid >> 2, c = tid & 3) holds gate and up columns 8 c .. + 7 of its row as packed bf16, adds nothing of its own to the arithmetic: the
//             activation is quantize.hip.h's silu_mul8 / swiglu_oai_mul8<BIAS> (bias chunks of the TILE's expert, one 16-byte load each, requested behind the K loop's last wait).
//             The chain's identity rotation is a bf16 MFMA that accumulates act * 1 + 0 * (the group's other values) onto +0: exact, except that an activation of -0
//             arrives as +0 -- reproduced here.  (A non-finite activation poisons its whole group there, 0 x inf; outside this op's contract, see the Python docstring.)
//             amax over the row's four lanes by two quad-permute DPP moves (no LDS), then the FP8 arm's rule: e8 = 127 if amax == 0 else max(E - 7, 0), codes =
//             fp8_pack4<QF_E4M3>(act * 2^(127 - e8)); one 8-byte code store per thread, one scale byte per row and tile, masked to the group's rows.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"
#include "quantize.hip.h"

namespace qamd {

struct W4A8ActParams : GroupedParams {   // N = 2 I (the weight's rows), tiles_n = I / 32; D is not written
  uint8_t* codes;        // (M, I) e4m3
  uint8_t* out_sf;       // flat (M, I / 32) e8m0
  const uint16_t* bias;  // (E, 2 I) bf16 [gate | up], ACT_OAI_BIAS only
  int inter;             // I
  SwigluOaiAct oai;      // ACT_OAI / ACT_OAI_BIAS
};

template <int SPW_, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 128 elements (RING: any K)
struct OsW4A8ActCfg {
  static constexpr int TM = TM_, TN = 32, ROWA = 128, ROWB = 64, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                                                        // m-tiles of 32 rows
  static constexpr int OFF_B = TM * ROWA, OFF_BU = OFF_B + 32 * ROWB, OFF_S = OFF_BU + 32 * ROWB, OFF_SB = OFF_S + 256, STAGE = OFF_SB + 256;
  static constexpr int NPA = TM / 8, NPB = 4;                                               // A / B pieces per stage
  static constexpr int LPS = NPA + NPB + 2;                                                 // LDS-DMA instructions per stage
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 256;                                                  // cross-wave sum: [wave] TM x 64 fp32
  static constexpr int LDS_BYTES = KTMAX * STAGE > RED ? KTMAX * STAGE : RED;
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
// slots per wave that fit the LDS: 16 stages of 8.5 KiB = 136 KiB, 12 of 12.5 KiB = 150 KiB
constexpr int os_w4a8_act_smax(int TM) { return TM == 32 ? 4 : 3; }

// max over the four lanes of a quad: quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0xB1, 0xf, 0xf, true)));
  return fmaxf(v, __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0x4E, 0xf, 0xf, true)));
}

// This function's fp32 arithmetic is compiled to the single forms (v_add_f32, v_mul_f32): the feature that lets the vectorizer pair independent fp32 operations into
// v_pk_* forms is switched off FOR THIS FUNCTION, in the source, so it holds in every build mode and leaves the unit's other kernels as they were.  The bits are the same
// either way (IEEE add and multiply); what the pairing would save in the epilogue's issue slots is not measured.  `flatten` goes with it: the inliner does not merge a
// callee built with the feature into a caller without it unless told to.
#if defined(__HIP_DEVICE_COMPILE__)
#define QAMD_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops"), flatten))
#else
#define QAMD_NO_PACKED_F32   // (the host pass knows no such feature)
#endif
// RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at most 4 SPW stages, every stage has a slot of its own)
template <class C, int ACT, bool RING = false>
__global__ __launch_bounds__(256) QAMD_NO_PACKED_F32 void gemm_mx_os_w4a8_act_kernel(const W4A8ActParams p) {
  constexpr int SPW = C::SPW, LPS = C::LPS, MT = C::MT;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the kernel's symbol -- as gemm_mx_os_w4a8_kernel)
  // the tile: grouped_setup's view, and the expert itself for the bias row
  GroupTile gt;
  if (!grouped_tile(p.offs, p.E, p.M, C::TM, p.tiles_n, (int)blockIdx.x, gt)) return;   // an m-tile slot past the real tiles: no work
  asm volatile("" :: "s"(p.A), "s"(p.codes), "s"(p.K), "s"(p.b_bytes), "s"(p.alpha));   // all scalar argument loads in one round
  const int grp = uniform(gt.g), gend = uniform(gt.row0 + gt.rows), m0 = uniform(gt.row0), n0 = uniform(gt.nt * 32), I = p.inter;
  const float alpha = p.alpha[p.n_alpha > 1 ? grp : 0];
  const uint8_t* Bg = p.B + (size_t)grp * p.b_bytes;        // 64-bit: the stacked weight may exceed 2 GiB
  const uint8_t* SFBg = p.SFB + (size_t)grp * p.sfb_bytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), i32 = lane & 31, g = lane >> 5;
  const int rowA = p.K, rowB = p.K >> 1, KT = p.K >> 7, KB = p.K >> 5;   // bytes per A / B row, stages, scale bytes per row
  const int er = tid >> 2, ec = tid & 3;                                  // the epilogue's row of the tile and chunk of 8 activation columns

  // ---- LDS-DMA sources: the W4A8 kernel's, with the up rows I weight rows behind the gate rows ---------------------------------------------------
  const uint32_t a_off = (uint32_t)m0 * rowA, b_off = (uint32_t)n0 * rowB;
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A + a_off, (uint32_t)gend * rowA - a_off), rB = make_rsrc(Bg + b_off, p.b_bytes - b_off);
  int vPA[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) vPA[par] = (lane >> 3) * rowA + (((lane & 7) ^ (((lane >> 4) + 4 * par) & 7)) << 4);
  const int vPB = (lane >> 2) * rowB + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
  const int stepA = 8 * rowA, stepB = 16 * rowB, upB = I * rowB;   // (I rowB < one expert's bytes < 2^31)
  const uint32_t sa_off = (uint32_t)m0 * KB, sb_off = (uint32_t)n0 * KB;
  const __amdgpu_buffer_rsrc_t rSA = make_rsrc(p.SFA + sa_off, (uint32_t)gend * KB - sa_off), rSB = make_rsrc(SFBg + sb_off, p.sfb_bytes - sb_off);
  const int vSA = (32 * (MT == 2 ? g : 0) + i32) * KB, vSB = (g * I + i32) * KB;

  auto issue = [&](const int kt, const int slot) __attribute__((always_inline)) {   // stage kt into slot `slot` of this wave (kt >= KT: every piece out of range -> zeros)
    char* st = smem + (wave * SPW + slot) * C::STAGE;
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {
      const int v = ((vPA[qq & 1] + qq * stepA) & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)(st + qq * 1024), 16, v, kt * C::ROWA, 0, 0);
    }
#pragma unroll
    for (int qq = 0; qq < C::NPB; ++qq) {   // 0, 1: gate rows 16 qq ..; 2, 3: up rows
      const int v = ((vPB + (qq & 1) * stepB + (qq >> 1) * upB) & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr_t)(st + C::OFF_B + qq * 1024), 16, v, kt * C::ROWB, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSA, (lds_ptr_t)(st + C::OFF_S), 4, (vSA & ~oob) | ((int)0x80000000 & oob), kt * 4, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSB, (lds_ptr_t)(st + C::OFF_SB), 4, (vSB & ~oob) | ((int)0x80000000 & oob), kt * 4, 0, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
#pragma unroll
  for (int j = 0; j < SPW; ++j) issue(wave + 4 * j, j);

  const int swA = (i32 >> 1) & 7, swB = (i32 >> 2) & 3;
  v16f accg[MT], accu[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accg[t][r] = 0.f; accu[t][r] = 0.f; }
  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };

  // one stage out of slot u; RING: kt_next (>= KT: zeros) is requested into the slot as soon as the reads have returned
  auto consume = [&](const int u, const int kt_next) __attribute__((always_inline)) {
    const char* st = smem + (wave * SPW + u) * C::STAGE;
    v4i fa[MT][4], fbg[2], fbu[2];
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {   // c4 = 2 js + u: A chunk 4 js + 2 u + g (bytes 16 g .. + 15 of K-block 2 js + u)
      const int chunk = 4 * (c4 >> 1) + 2 * (c4 & 1) + g;
      const int off = i32 * C::ROWA + ((chunk ^ swA) << 4);
#pragma unroll
      for (int t = 0; t < MT; ++t) fa[t][c4] = *(const v4i*)(st + t * 32 * C::ROWA + off);
    }
#pragma unroll
    for (int js = 0; js < 2; ++js) {   // B chunk = K-block 2 js + g
      fbg[js] = *(const v4i*)(st + C::OFF_B + i32 * C::ROWB + (((2 * js + g) ^ swB) << 4));
      fbu[js] = *(const v4i*)(st + C::OFF_BU + i32 * C::ROWB + (((2 * js + g) ^ swB) << 4));
    }
    int sa[MT], sbg, sbu;
#pragma unroll
    for (int t = 0; t < MT; ++t) sa[t] = *(const int*)(st + C::OFF_S + (MT == 2 ? (32 * t + i32) * 4 : lane * 4));
    sbg = *(const int*)(st + C::OFF_SB + i32 * 4);
    sbu = *(const int*)(st + C::OFF_SB + (32 + i32) * 4);
    fence();   // every read issued before the first MFMA
    if constexpr (RING) {
      if constexpr (MT == 1)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]), "+v"(fbg[0]), "+v"(fbg[1]), "+v"(fbu[0]), "+v"(fbu[1]), "+v"(sa[0]),
                     "+v"(sbg), "+v"(sbu) :: "memory");   // the slot is free
      else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]), "+v"(fa[MT - 1][0]), "+v"(fa[MT - 1][1]), "+v"(fa[MT - 1][2]),
                     "+v"(fa[MT - 1][3]), "+v"(fbg[0]), "+v"(fbg[1]), "+v"(fbu[0]), "+v"(fbu[1]), "+v"(sa[0]), "+v"(sa[MT - 1]), "+v"(sbg), "+v"(sbu) :: "memory");
      issue(kt_next, u);
      fence();
    }
    // "my" scale byte of K-block 2 js + g down to byte 2 js: op_sel 2 js picks it
#pragma unroll
    for (int t = 0; t < MT; ++t) sa[t] = (int)((unsigned)sa[t] >> (8 * g));
    sbg = (int)((unsigned)sbg >> (8 * g));
    sbu = (int)((unsigned)sbu >> (8 * g));
    // cbsz = format of srcA (the weight fragment): 4 = e2m1; blgp = format of srcB (the token fragment): 0 = e4m3
#pragma unroll
    for (int js = 0; js < 2; ++js) {
      const v8i G8 = {fbg[js][0], fbg[js][1], fbg[js][2], fbg[js][3], 0, 0, 0, 0};
      const v8i U8 = {fbu[js][0], fbu[js][1], fbu[js][2], fbu[js][3], 0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const v4i a = fa[t][2 * js], ah = fa[t][2 * js + 1];
        const v8i A8 = {a[0], a[1], a[2], a[3], ah[0], ah[1], ah[2], ah[3]};
        if (js == 0) {
          accg[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(G8, A8, accg[t], 4, 0, 0, sbg, 0, sa[t]);
          accu[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(U8, A8, accu[t], 4, 0, 0, sbu, 0, sa[t]);
        } else {
          accg[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(G8, A8, accg[t], 4, 0, 2, sbg, 2, sa[t]);
          accu[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(U8, A8, accu[t], 4, 0, 2, sbu, 2, sa[t]);
        }
      }
    }
    fence();
  };
  if constexpr (!RING) {
    static_for<0, SPW>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((SPW - 1 - j) * LPS) : "memory");   // this wave's stage j landed (its later stages may still be in flight)
      fence();
      consume(j, 0);
    });
  } else {
    // the wave's stages kt = wave + 4 j, j = 0, 1, ...: slot j % SPW; behind the wait for stage j exactly the SPW - 1 stages after it are outstanding (the refills
    // past K are zero-fill pieces: the count stays the same to the end)
    for (int kt = wave; kt < KT; kt += 4 * SPW) {
      static_for<0, SPW>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
        if (u == 0 || kt + 4 * u < KT) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((SPW - 1) * LPS) : "memory");
          fence();
          consume(u, kt + 4 * u + 4 * SPW);
        }
      });
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  // the bias chunks, behind the last counted wait (the K loop's vmcnt immediates count LDS-DMA pieces only) and in flight across the sum
  v4i bgate = {0, 0, 0, 0}, bup = {0, 0, 0, 0};
  if constexpr (ACT == ACT_OAI_BIAS) {   // the tile's own expert (well-formed offs: the row's); in range whatever the row
    const uint16_t* b = p.bias + (size_t)grp * (2 * (size_t)I) + n0 + 8 * ec;
    bgate = *(const v4i*)b;
    bup = *(const v4i*)(b + I);
  }
  __builtin_amdgcn_s_barrier();   // every wave's reads of the stage areas are done: they become the sum's scratch
  fence();

  // ---- cross-wave sum: [wave][row][16 chunks of 4 fp32: 0-7 gate, 8-15 up], chunk ^ (row & 15) ------------------------------------------------------
  // acc[4 q + e] = column 8 q + 4 g + e of token row i32: chunk 2 q + g
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      char* rowp = smem + (wave * C::TM + 32 * t + i32) * 256;
      *(v4f*)(rowp + (((2 * q + g) ^ (i32 & 15)) << 4)) = v4f{accg[t][4 * q + 0], accg[t][4 * q + 1], accg[t][4 * q + 2], accg[t][4 * q + 3]};
      *(v4f*)(rowp + (((8 + 2 * q + g) ^ (i32 & 15)) << 4)) = v4f{accu[t][4 * q + 0], accu[t][4 * q + 1], accu[t][4 * q + 2], accu[t][4 * q + 3]};
    }
  __syncthreads();
  if (er >= C::TM) return;   // (TM = 32: the first two waves; whole quads leave, so the DPP moves below stay within live lanes)

  // ---- epilogue: ((w0 + w1) + w2) + w3, one multiply by alpha, one rounding to bf16 -- the GEMM op's output -- then activation and quantizer in registers ----
  v4i yg, yu;
#pragma unroll
  for (int h = 0; h < 2; ++h) {   // chunks 2 ec + h of the gate and of the up half
    v4f sg[4], su[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const char* rowp = smem + (w * C::TM + er) * 256;
      sg[w] = *(const v4f*)(rowp + (((2 * ec + h) ^ (er & 15)) << 4));
      su[w] = *(const v4f*)(rowp + (((8 + 2 * ec + h) ^ (er & 15)) << 4));
    }
    v4f tg, tu;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tg[e] = ((sg[0][e] + sg[1][e]) + sg[2][e]) + sg[3][e];
      tu[e] = ((su[0][e] + su[1][e]) + su[2][e]) + su[3][e];
    }
    yg[2 * h] = (int)pack_bf16x2(tg[0] * alpha, tg[1] * alpha);
    yg[2 * h + 1] = (int)pack_bf16x2(tg[2] * alpha, tg[3] * alpha);
    yu[2 * h] = (int)pack_bf16x2(tu[0] * alpha, tu[1] * alpha);
    yu[2 * h + 1] = (int)pack_bf16x2(tu[2] * alpha, tu[3] * alpha);
  }
  v4i act;
  if constexpr (ACT == ACT_SILU) act = silu_mul8(yg, yu);
  else if constexpr (ACT == ACT_OAI_BIAS) act = swiglu_oai_mul8<true>(yg, yu, bgate, bup, p.oai);
  else act = swiglu_oai_mul8<false>(yg, yu, yg, yu, p.oai);   // (no bias: the last two are not read)

  // the identity rotation of the chain: act * 1 + 0 onto +0 -- the value itself, -0 as +0
  float x[8];
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w = (uint32_t)act[i];
    const uint32_t lo = w << 16, hi = w & 0xffff0000u;
    x[2 * i] = __uint_as_float(lo == 0x80000000u ? 0u : lo);
    x[2 * i + 1] = __uint_as_float(hi == 0x80000000u ? 0u : hi);
    m = fmaxf(m, fmaxf(fabsf(x[2 * i]), fabsf(x[2 * i + 1])));   // v_max_f32 drops NaNs
  }
  m = quad_max(m);
  uint32_t e8;
  const float mul = mxf8_block_scale<QF_E4M3>(m, e8);   // the FP8 arm's rule (quantize.hip.h)
  float t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = x[i] * mul;
  const int row = m0 + er;
  if (row < gend) {
    v2i o;
    o[0] = (int)fp8_pack4<QF_E4M3>(t);
    o[1] = (int)fp8_pack4<QF_E4M3>(t + 4);
    *(v2i*)(p.codes + (size_t)row * I + n0 + 8 * ec) = o;
    if (ec == 0) p.out_sf[(size_t)row * (I >> 5) + gt.nt] = (uint8_t)e8;
  }
#endif
}

}  // namespace qamd
