// Grouped W4A16 GEMM on NVFP4 expert weights for gfx950 (extension: grouped_matmul_bf16_nvf4_bf16_tn): bf16 tokens, unquantised and without scales, against stacked
// NVFP4 weights as a checkpoint stores them -- e2m1 codes (E, N, K/2), one e4m3 scale per 16 elements, row-major (E, N, K/16): the buffer grouped_matmul_nvf4_bf16_tn
// reads --, the per-expert global scale in alpha.  gfx950 has no NVFP4 MFMA: the weights are dequantised to bf16 in registers and meet the tokens on
// v_mfma_f32_32x32x16_bf16.
//
// CONTRACT.  out[r, n] = bf16( alpha[g] * sum_k x[r, k] * w[g, n, k] ) for every row r of group g, w = e2m1(code) * e4m3(scale) HELD AS bf16.
//   * w is exact for EVERY finite scale byte of either sign: an e2m1 magnitude has at most 2 significant bits, an e4m3 value at most 4, the product at most 6 (bf16
//     holds 8), and the magnitudes lie in [2^-10, 2688], all normal bf16.  (The MXFP4 op excludes the scale bytes 0, 1, 253, 254; this op has no such set.)
//   * products of two bf16 are exact in fp32; the sums are fp32 (the MFMA's, then ((w0 + w1) + w2) + w3 across the waves); one fp32 multiply by alpha[g], one rounding.
//   * scale bytes 0x7f / 0xff (the e4m3fn NaN) make EVERY output of that weight row NaN for the rows of that expert; 0x00 / 0x80 give w = 0 (of either sign).
//   * NaN and inf in x propagate as in fp64 arithmetic on the same operands.
//   * K % 128 == 0, N % 8 == 0, E <= 1024, the token matrix and one expert's weight below 2 GiB; rows at or past offs[E - 1] are not written; malformed offs as in the
//     other grouped ops.  GATHER (src_row (M,) int32): A is the unsorted (T, K) tokens, an index outside [0, T) reads an all-zero token and never addresses memory.
//
// A kernel of its own (gemm_mx_os_w4a16.hip.h and gemm_mx_os_w4a16_act.hip.h keep their code and names).  Four waves; wave w owns the 128-element K stages w, w + 4, ...
// and walks them without a barrier; a workgroup owns TM x 32 outputs, TM = 32 (form 620) or 64 (form 621).
//   tokens    through LDS as in the W4A16 kernels: a stage row is 256 B = one LDS bank row, LDS-DMA pieces of 4 rows, physical 16-byte chunk = logical chunk ^ (row & 15)
//             (conflict-free, derived in gemm_mx_os_w4a16.hip.h); GATHER puts src_row[r] * 2 K into the row part of the lane offset, bit 31 for a row past the group or
//             an index outside [0, T).
//   weights   NOT in LDS: in a wave-owned stage every 16-byte code chunk is read by exactly one lane of one wave, so LDS would share nothing.  Lane (i32, g) holds weight
//             row n0 + i32 and K-blocks (32 codes) 2 js + g, js = 0, 1, of the stage: two buffer_load_dwordx4 (js adds 32 B, the stage 64 B) and ONE buffer_load_dwordx2,
//             the row's 8 scale bytes of the stage (the lane uses bytes 2 g, 2 g + 1 of dword js -- not contiguous across js, so no 4-byte load serves it), straight
//             into VGPRs, 10 registers per slot.  They are requested with the stage's token pieces and counted in the same vmcnt sequence: LPS = TM / 4 + 3 loads per
//             stage, all landed behind ONE wait.  Rows past N fall off the descriptors and read zero codes and zero scales.
//   dequant   in registers.  The f32 scale operand of the v_cvt_scalef32_pk_*_fp4 converts contributes its exponent only (profiles/native_r2_cvt_scale_probe.txt), so
//             the e4m3 scale cannot ride in the convert.  Per stage and js ONE v_lshrrev (dword js >> 16 g) and ONE v_cvt_scalef32_pk_f32_fp8 (scale 1.0; OCP e4m3fn:
//             sign honoured, 0x7f / 0xff -> NaN) give the lane's two group scales as fp32 -- no split into exponent and mantissa is needed, because per pair of codes
//                 v_cvt_scalef32_pk_f32_fp4 (scale 1.0)   the two codes as fp32, exact
//                 v_pk_mul_f32 by {s, s}                  exact: at most 6 significant bits, magnitude in [2^-10, 2688]
//                 v_cvt_pk_bf16_f32                       exact for the same reason
//             is exact for all 254 finite bytes x 16 codes BY CONSTRUCTION, and IEEE arithmetic does the two special cases: a zero scale gives code x (+-0) = +-0, a
//             NaN scale gives code x NaN = NaN for every code (0 included), so ALL 16 elements of the group are NaN and x * NaN poisons the weight row's sums for every
//             x -- no select, no OR-ed element.  That is three VALU instructions per two elements where the MXFP4 kernel has one.
//             Dword d of a chunk -- codes k = 32 (2 js + g) + 8 d ... + 7 -- belongs to scale group 2 (2 js + g) + (d >> 1) of the stage: group d >> 1 of the lane's
//             K-block, element d >> 1 of the converted pair.  One MFMA's K = 16 is one lane's 8 codes per g; its A operand is 16-byte chunk 4 (2 js + g) + d of the
//             lane's token row.
//   balance   (a DERIVATION from instruction counts, NOT measured: no counter run separates the two pipes, and it assumes four cycles for every VALU instruction,
//             v_pk_mul_f32 included, and no overlap inside a wave)  per lane and stage: 2 js x 4 d x 4 pairs x 3 = 96 VALU for the fragments + 4 for the scales = 100, of four cycles each = 400 cycles on the wave's SIMD;
//             the MFMAs of the stage are 8 x 32 = 256 cycles (TM = 32) / 16 x 32 = 512 (TM = 64: a weight fragment is converted ONCE and used for both m-tiles).  So
//             the 32-row form would be bounded by the converts (the MFMA pipe idles a third of a stage unless another workgroup's wave on the SIMD fills it), the 64-row form
//             by the MFMAs, with the converts hidden behind them.
//   slots     SPW per wave.  A stage is TM x 256 B of LDS and nothing else, so LDS = 4 SPW TM 256 B; a CU has 160 KiB:
//               TM = 32 (620):  SPW 1  32 KiB (K <= 512; 5 / CU)   2  64 KiB (2 / CU): one shot up to K = 1024, rings of 2 beyond
//               TM = 64 (621):  SPW 1  64 KiB (K <= 512; 2 / CU)   2  128 KiB (1 / CU): one shot up to K = 1024, rings of 2 beyond
//             (the ladder of gemm_mx_os_w4a16_act.hip.h; three or four slots of the 32-row form were not built.)  A ring consumes all its slots every round: the
//             stages past K are zero-fill loads (offset bit 31: zero tokens, zero codes, zero scales), acc + 0 x 0, at most one per wave.
//   sum       [wave][TM][32] fp32 in the freed stage area (a row is 8 chunks of 4 fp32, chunk ^ (row & 7)), ((w0 + w1) + w2) + w3, one multiply by alpha[g], one
//             rounding to bf16; thread (row = tid >> 2, c = tid & 3) stores columns 8 c .. + 7 of its row with ONE 16-byte store, masked to the group's rows and to N.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"
#include "gemm_mx_os_w4a16.hip.h"   // W4A16Params

namespace qamd {

template <int SPW_, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 128 elements (RING: any K)
struct OsNvW4A16Cfg {
  static constexpr int TM = TM_, TN = 32, ROWA = 256, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                           // m-tiles of 32 rows
  static constexpr int STAGE = TM * ROWA;                      // tokens only
  static constexpr int NPA = TM / 4, NLB = 3;                  // A pieces / code and scale register loads per stage
  static constexpr int LPS = NPA + NLB;                        // vector memory instructions per stage
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 128;                     // cross-wave sum: [wave] TM x 32 fp32
  static constexpr int LDS_BYTES = KTMAX * STAGE;
  static_assert(LDS_BYTES >= RED, "the stage area holds the sum's scratch");
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

// the weight side of one stage in registers: 16 B of codes per js, the row's 8 scale bytes of the stage
struct NvW4A16B {
  v4u c[2];
  v2u s;
};

// RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at most 4 SPW stages, every stage has a slot of its own); GATHER: A rows through p.src_row
template <class C, bool RING = false, bool GATHER = false>
__global__ __launch_bounds__(256) void gemm_nvf4_os_w4a16_kernel(const W4A16Params p) {
  constexpr int SPW = C::SPW, LPS = C::LPS, MT = C::MT;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the kernel's symbol -- as gemm_mx_os_w4a16_kernel)
  GroupTile gt;
  if (!grouped_tile(p.offs, p.E, p.M, C::TM, p.tiles_n, (int)blockIdx.x, gt)) return;   // an m-tile slot past the real tiles: no work
  asm volatile("" :: "s"(p.A), "s"(p.D), "s"(p.K), "s"(p.b_bytes), "s"(p.alpha));   // all scalar argument loads in one round
  const int grp = uniform(gt.g), gend = uniform(gt.row0 + gt.rows), m0 = uniform(gt.row0), n0 = uniform(gt.nt * 32);
  const float alpha = p.alpha[p.n_alpha > 1 ? grp : 0];
  const uint8_t* Bg = p.B + (size_t)grp * p.b_bytes;        // 64-bit: the stacked weight may exceed 2 GiB
  const uint8_t* SFBg = p.SFB + (size_t)grp * p.sfb_bytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), i32 = lane & 31, g = lane >> 5;
  const int rowA = p.K << 1, rowB = p.K >> 1, KT = p.K >> 7, KS = p.K >> 4;   // bytes per A / B row, stages, scale bytes per row

  // ---- sources -------------------------------------------------------------------------------------------------------------------------------
  const uint32_t a_off = GATHER ? 0u : (uint32_t)m0 * rowA, b_off = (uint32_t)n0 * rowB, sb_off = (uint32_t)n0 * KS;
  const __amdgpu_buffer_rsrc_t rA = GATHER ? make_rsrc(p.A, (uint32_t)p.T * rowA) : make_rsrc(p.A + a_off, (uint32_t)gend * rowA - a_off);
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(Bg + b_off, p.b_bytes - b_off), rSB = make_rsrc(SFBg + sb_off, p.sfb_bytes - sb_off);
  // A piece qq = rows 4 qq .. + 3; lane -> row 4 qq + (l >> 4), physical chunk l & 15 = logical chunk ^ (4 (qq & 3) | (l >> 4)) (the W4A16 kernel's)
  const int cA = ((lane & 15) ^ (lane >> 4)) << 4;
  int vRA[C::NPA];   // the row part of every piece's offset; GATHER: bit 31 (past every descriptor) for a row past the group's end or an index outside [0, T)
  if constexpr (GATHER) {
    int idx[C::NPA];
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {   // unconditional, in-bounds loads: one round trip, before the K walk
      const int r = m0 + 4 * qq + (lane >> 4);
      idx[qq] = p.src_row[r < gend ? r : m0];
    }
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {
      const int r = m0 + 4 * qq + (lane >> 4);
      const bool ok = r < gend && (unsigned)idx[qq] < (unsigned)p.T;
      vRA[qq] = ok ? idx[qq] * rowA : (int)0x80000000;
    }
  } else {
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) vRA[qq] = (4 * qq + (lane >> 4)) * rowA;
  }
  // weights: the lane's row i32 of the tile (a row past N lies past the descriptor), K-block g of the stage; js adds 32 B, the stage 64 B (codes) / 8 B (scales)
  const int vB = i32 * rowB + 16 * g, vS = i32 * KS;

  auto issue_a = [&](const int kt, const int slot) __attribute__((always_inline)) {   // the tokens of stage kt into slot `slot` of this wave (kt >= KT: zeros)
    char* st = smem + (wave * SPW + slot) * C::STAGE;
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {
      const int v = ((vRA[qq] + (cA ^ (64 * (qq & 3)))) & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)(st + qq * 1024), 16, v, kt * C::ROWA, 0, 0);
    }
  };
  auto issue_b = [&](const int kt, NvW4A16B& w) __attribute__((always_inline)) {      // the weights of stage kt into registers (kt >= KT: zeros)
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
    const int hi = (int)0x80000000 & oob;
#pragma unroll
    for (int js = 0; js < 2; ++js) w.c[js] = __builtin_amdgcn_raw_buffer_load_b128(rB, ((vB + 32 * js) & ~oob) | hi, kt * 64, 0);
    w.s = __builtin_amdgcn_raw_buffer_load_b64(rSB, (vS & ~oob) | hi, kt * 8, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
  NvW4A16B wb[SPW];
  static_for<0, SPW>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    issue_a(wave + 4 * j, j);
    issue_b(wave + 4 * j, wb[j]);
  });

  const int swA = i32 & 15;
  v16f acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };

  // one stage out of slot u; RING: kt_next (>= KT: zeros) is requested into the slot
  auto consume = [&](auto uc, const int kt_next) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
    const char* st = smem + (wave * SPW + u) * C::STAGE;
    v4i fa[MT][8];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {   // c8 = 4 js + d: A chunk 4 (2 js + g) + d (elements 8 d .. + 7 of K-block 2 js + g)
      const int chunk = 4 * (2 * (c8 >> 2) + g) + (c8 & 3);
      const int off = i32 * C::ROWA + ((chunk ^ swA) << 4);
#pragma unroll
      for (int t = 0; t < MT; ++t) fa[t][c8] = *(const v4i*)(st + t * 32 * C::ROWA + off);
    }
    fence();   // every read issued before the first convert
    if constexpr (RING) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]), "+v"(fa[0][4]), "+v"(fa[0][5]), "+v"(fa[0][6]), "+v"(fa[0][7])
                   :: "memory");   // the slot is free
      if constexpr (MT == 2)
        asm volatile("" : "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fa[1][2]), "+v"(fa[1][3]), "+v"(fa[1][4]), "+v"(fa[1][5]), "+v"(fa[1][6]), "+v"(fa[1][7]) :: "memory");
      issue_a(kt_next, u);
      fence();
    }
    const NvW4A16B w = wb[u];
#pragma unroll
    for (int js = 0; js < 2; ++js) {
      // bytes 2 g, 2 g + 1 of dword js: the scales of groups 0, 1 of K-block 2 js + g, as fp32 (NaN for 0x7f / 0xff, +-0 for 0x00 / 0x80)
      const f32x2_t sc = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w.s[js] >> (16 * g), 1.0f, false);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const unsigned u8 = w.c[js][d];
        const f32x2_t s2 = {sc[d >> 1], sc[d >> 1]};
        // the two codes of byte b (byte_sel, an immediate) are elements 2 b, 2 b + 1
        const bf16x2_t w0 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 0) * s2, bf16x2_t);
        const bf16x2_t w1 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 1) * s2, bf16x2_t);
        const bf16x2_t w2 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 2) * s2, bf16x2_t);
        const bf16x2_t w3 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 3) * s2, bf16x2_t);
        const v4i wi = {__builtin_bit_cast(int, w0), __builtin_bit_cast(int, w1), __builtin_bit_cast(int, w2), __builtin_bit_cast(int, w3)};
        const v8bf B8 = __builtin_bit_cast(v8bf, wi);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8, __builtin_bit_cast(v8bf, fa[t][4 * js + d]), acc[t], 0, 0, 0);
      }
    }
    if constexpr (RING) {
      fence();
      issue_b(kt_next, wb[u]);   // behind the last convert: into the registers it freed
    }
    fence();
  };
  if constexpr (!RING) {
    static_for<0, SPW>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((SPW - 1 - j) * LPS) : "memory");   // this wave's stage j landed (its later stages may still be in flight)
      fence();
      consume(jc, 0);
    });
  } else {
    // the wave's stages kt = wave + 4 j, j = 0, 1, ...: slot j % SPW; behind the wait for stage j exactly the SPW - 1 stages after it are outstanding.  Every round
    // consumes all SPW slots (no branch inside a round: the compiler's own count for the register loads stays the one below); a slot whose stage lies past K holds zeros.
    for (int kt = wave; kt < KT; kt += 4 * SPW) {
      static_for<0, SPW>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((SPW - 1) * LPS) : "memory");
        fence();
        consume(uc, kt + 4 * u + 4 * SPW);
      });
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // every wave's reads of the stage areas are done: they become the sum's scratch
  fence();

  // ---- cross-wave sum: [wave][row][8 chunks of 4 fp32], chunk ^ (row & 7) ---------------------------------------------------------------------------
  // acc[4 q + e] = column 8 q + 4 g + e of token row i32: chunk 2 q + g
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *(v4f*)(smem + (wave * C::TM + 32 * t + i32) * 128 + (((2 * q + g) ^ (i32 & 7)) << 4)) = v4f{acc[t][4 * q + 0], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
  __syncthreads();
  const int er = tid >> 2, ec = tid & 3;   // the epilogue's row of the tile and chunk of 8 columns
  if (er >= C::TM) return;                 // (TM = 32: the first two waves)

  // ---- epilogue: ((w0 + w1) + w2) + w3, one multiply by alpha, one rounding to bf16, one 16-byte store -----------------------------------------------
  v4i y;
#pragma unroll
  for (int h = 0; h < 2; ++h) {   // chunks 2 ec + h
    v4f s[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w] = *(const v4f*)(smem + (w * C::TM + er) * 128 + (((2 * ec + h) ^ (er & 7)) << 4));
    v4f t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = ((s[0][e] + s[1][e]) + s[2][e]) + s[3][e];
    y[2 * h] = (int)pack_bf16x2(t[0] * alpha, t[1] * alpha);
    y[2 * h + 1] = (int)pack_bf16x2(t[2] * alpha, t[3] * alpha);
  }
  const int row = m0 + er, col = n0 + 8 * ec;
  if (row < gend && col < p.N) *(v4i*)(p.D + (size_t)row * p.ldd + col) = y;   // N % 8 == 0: a chunk lies inside N or past it
#endif
}

}  // namespace qamd
