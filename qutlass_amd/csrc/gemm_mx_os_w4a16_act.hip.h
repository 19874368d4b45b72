// Gate/up grouped W4A16 GEMM with the activation fused into its epilogue, for gfx950 (extensions: grouped_matmul_bf16_mxf4_silu_bf16_tn,
// grouped_matmul_bf16_mxf4_swiglu_oai_bf16_tn): bf16 tokens against the (E, 2 I, K/2) [gate | up] MXFP4 weights of an expert layer, and what leaves the kernel is the
// down GEMM's A operand -- (M, I) bf16 -- bit for bit what
//   silu_and_mul / swiglu_oai_and_mul (grouped_matmul_bf16_mxf4_bf16_tn(...))
// writes; the (M, 2 I) bf16 tensor between the two launches never exists.  The contract of gemm_mx_os_w4a16.hip.h carries over with N = 2 I (scale bytes, NaN and inf,
// malformed offs, the 2 GiB bounds, GATHER: src_row outside [0, T) reads a zero token, E <= 1024), plus I % 32 == 0.
//
// A kernel of its own (gemm_mx_os_w4a16.hip.h keeps its code and its names).  Four waves, wave w owns the 128-element K stages w, w + 4, ... and walks them without a
// barrier; a workgroup owns TM = 32 or 64 token rows x 32 ACTIVATION columns n0 .. n0 + 31: the 32 gate weight rows n0 .. AND the 32 up weight rows I + n0 .. .
//   tokens    as in the W4A16 kernel: a stage row is 256 B = one LDS bank row, LDS-DMA pieces of 4 rows, physical 16-byte chunk = logical chunk ^ (row & 15)
//             (conflict-free, derived there); GATHER puts src_row[r] * 2 K into the row part of the lane offset, bit 31 for a row past the group or an index outside [0, T).
//   weights   NOT in LDS.  In a wave-owned stage every 16-byte weight chunk is read by exactly one lane of one wave -- lane (i32, g) of the stage's wave converts K-blocks
//             g and 2 + g of weight rows n0 + i32 and I + n0 + i32 -- so LDS would share nothing.  Per stage and lane: four buffer_load_dwordx4 (gate / up x js = 0, 1:
//             K-block 2 js + g) and two buffer_load_dword (the row's four scale bytes of the stage; the lane uses bytes g and 2 + g) straight into VGPRs, 18 registers per
//             slot.  They are requested with the stage's A pieces and counted in the same vmcnt sequence: LPS = TM / 4 + 6 loads per stage, all landed behind ONE wait.
//             In a ring the A pieces of the slot's next stage go out as soon as the LDS reads have returned, its weight loads behind the stage's last convert (the
//             registers they land in are the ones that convert frees); the loads of a stage stay together, so the count per stage does not change.
//   MFMAs     dword d of a chunk through four v_cvt_scalef32_pk_bf16_fp4 with the block's scale as fp32 (byte << 23; byte 255: one NaN element poisons the row, as in
//             the W4A16 kernel) into the operand of v_mfma_f32_32x32x16_bf16.  Per stage and m-tile sixteen MFMAs, eight gate and eight up, on the same token fragment;
//             a weight fragment is converted once and used for both m-tiles of the 64-row form.  Per accumulator the sequence is the W4A16 kernel's: stages w, w + 4, ...
//             in order, js = 0, 1, d = 0 ... 3 inside a stage.
//   slots     SPW per wave.  A stage is TM x 256 B and nothing else, so LDS = 4 SPW TM 256 B, which is SPW times the sum's scratch (below); a CU has 160 KiB:
//               TM = 32 (form 618):  SPW 1  32 KiB (K <= 512; 4 / CU)   2  64 KiB (2 / CU): one shot up to K = 1024, rings of 2 beyond
//               TM = 64 (form 619):  SPW 1  64 KiB (K <= 512; 2 / CU)                                  2  128 KiB (1 / CU): one shot up to K = 1024, rings of 2 beyond
//             (the W4A8-act layout -- weights and scales in LDS, TM 256 + 64 64 + 256 B per stage -- gives 12.25 / 20.25 KiB: two slots of the 64-row form are 162 KiB,
//             over the CU.)  Three and four slots of the 32-row form fit (96 / 128 KiB) but leave one workgroup per CU, where the fused W4A8 op lost; not built.
//             Registers (profiles/kernel_resources_w4a16_act.diff): 78-92 VGPRs + 32 AGPRs one shot, 109 + 32 ring (618); 95-123 + 64, 145 + 64 (619); no scratch --
//             the workgroups per CU above are the LDS's, the registers allow them.
//             A ring consumes all its slots every round: the stages past K are zero-fill loads (offset bit 31), acc + 0 x 0, at most one per wave.
//   sum       [wave][TM][64] fp32 in the freed stage area -- a row is 16 chunks of 4 fp32, 0-7 gate, 8-15 up, chunk ^ (row & 15), as in the W4A8-act kernel --,
//             ((w0 + w1) + w2) + w3, one multiply by alpha[g], one rounding to bf16: the W4A16 op's output row, bit for bit.
//   epilogue  thread (row = tid >> 2, c = tid & 3) holds gate and up columns 8 c .. + 7 of its row as packed bf16; the activation is quantize.hip.h's silu_mul8 /
//             swiglu_oai_mul8<BIAS> (bias chunks of the TILE's expert, one 16-byte load each, requested behind the K loop's last wait); one 16-byte store, masked to the
//             group's rows.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"
#include "gemm_mx_os_w4a16.hip.h"   // W4A16Params
#include "quantize.hip.h"

namespace qamd {

struct W4A16ActParams : W4A16Params {   // N = 2 I (the weight's rows), tiles_n = I / 32; D (M, I) bf16, ldd = I
  const uint16_t* bias;  // (E, 2 I) bf16 [gate | up], ACT_OAI_BIAS only
  int inter;             // I
  SwigluOaiAct oai;      // ACT_OAI / ACT_OAI_BIAS
};

template <int SPW_, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 128 elements (RING: any K)
struct OsW4A16ActCfg {
  static constexpr int TM = TM_, TN = 32, ROWA = 256, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                           // m-tiles of 32 rows
  static constexpr int STAGE = TM * ROWA;                      // tokens only
  static constexpr int NPA = TM / 4, NLB = 6;                  // A pieces / weight and scale register loads per stage
  static constexpr int LPS = NPA + NLB;                        // vector memory instructions per stage
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 256;                     // cross-wave sum: [wave] TM x 64 fp32
  static constexpr int LDS_BYTES = KTMAX * STAGE;
  static_assert(LDS_BYTES >= RED, "the stage area holds the sum's scratch");
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
// slots per wave of both forms (the ladder of launch_grouped_w4a16_act_os): 2 x 4 x 8 KiB = 64 KiB, 2 x 4 x 16 KiB = 128 KiB
constexpr int os_w4a16_act_smax(int) { return 2; }

// the weight side of one stage in registers: 16 B of gate and of up codes per js, the two rows' scale dwords
struct W4A16ActB {
  v4u g[2], u[2];
  uint32_t sg, su;
};

// The epilogue's fp32 adds and multiplies are compiled as the W4A16 kernel's and the streaming activation kernels' are -- the unit's default, no function attribute: an
// IEEE add or multiply has the same bits in its single and its paired (v_pk_*) form except for the sign of a NaN it GENERATES (0 x inf), so "any operands" asks for the
// forms those kernels have.  RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at most 4 SPW stages, every stage has a slot of its own)
template <class C, int ACT, bool RING = false, bool GATHER = false>
__global__ __launch_bounds__(256) void gemm_mx_os_w4a16_act_kernel(const W4A16ActParams p) {
  constexpr int SPW = C::SPW, LPS = C::LPS, MT = C::MT;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the kernel's symbol -- as gemm_mx_os_w4a16_kernel)
  GroupTile gt;
  if (!grouped_tile(p.offs, p.E, p.M, C::TM, p.tiles_n, (int)blockIdx.x, gt)) return;   // an m-tile slot past the real tiles: no work
  asm volatile("" :: "s"(p.A), "s"(p.D), "s"(p.K), "s"(p.b_bytes), "s"(p.alpha));   // all scalar argument loads in one round
  const int grp = uniform(gt.g), gend = uniform(gt.row0 + gt.rows), m0 = uniform(gt.row0), n0 = uniform(gt.nt * 32), I = p.inter;
  const float alpha = p.alpha[p.n_alpha > 1 ? grp : 0];
  const uint8_t* Bg = p.B + (size_t)grp * p.b_bytes;        // 64-bit: the stacked weight may exceed 2 GiB
  const uint8_t* SFBg = p.SFB + (size_t)grp * p.sfb_bytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), i32 = lane & 31, g = lane >> 5;
  const int rowA = p.K << 1, rowB = p.K >> 1, KT = p.K >> 7, KB = p.K >> 5;   // bytes per A / B row, stages, scale bytes per row
  const int er = tid >> 2, ec = tid & 3;                                       // the epilogue's row of the tile and chunk of 8 activation columns

  // ---- sources -------------------------------------------------------------------------------------------------------------------------------
  const uint32_t a_off = GATHER ? 0u : (uint32_t)m0 * rowA, b_off = (uint32_t)n0 * rowB, sb_off = (uint32_t)n0 * KB;
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
  // weights: the lane's gate row i32 and up row I + i32 of the tile (both below N = 2 I: I % 32 == 0), K-block g of the stage; js adds 32 B, the stage 64 B
  const int vBG = i32 * rowB + 16 * g, vBU = vBG + I * rowB;   // (I rowB < one expert's bytes < 2^31)
  const int vSG = i32 * KB, vSU = vSG + I * KB;

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
  auto issue_b = [&](const int kt, W4A16ActB& w) __attribute__((always_inline)) {      // the weights of stage kt into registers (kt >= KT: zeros)
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
    const int hi = (int)0x80000000 & oob;
#pragma unroll
    for (int js = 0; js < 2; ++js) {
      w.g[js] = __builtin_amdgcn_raw_buffer_load_b128(rB, ((vBG + 32 * js) & ~oob) | hi, kt * 64, 0);
      w.u[js] = __builtin_amdgcn_raw_buffer_load_b128(rB, ((vBU + 32 * js) & ~oob) | hi, kt * 64, 0);
    }
    w.sg = __builtin_amdgcn_raw_buffer_load_b32(rSB, (vSG & ~oob) | hi, kt * 4, 0);
    w.su = __builtin_amdgcn_raw_buffer_load_b32(rSB, (vSU & ~oob) | hi, kt * 4, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
  W4A16ActB wb[SPW];
  static_for<0, SPW>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    issue_a(wave + 4 * j, j);
    issue_b(wave + 4 * j, wb[j]);
  });

  const int swA = i32 & 15;
  v16f accg[MT], accu[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accg[t][r] = 0.f; accu[t][r] = 0.f; }
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
    const W4A16ActB w = wb[u];
    const unsigned sgs = w.sg >> (8 * g), sus = w.su >> (8 * g);   // "my" scale byte of K-block 2 js + g at byte 2 js
#pragma unroll
    for (int js = 0; js < 2; ++js) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {   // 0: gate, 1: up
        const unsigned byte = ((half ? sus : sgs) >> (16 * js)) & 0xffu;
        const float scale = __builtin_bit_cast(float, byte << 23);   // 2^(byte - 127) for bytes 1 ... 254
        const int nan = byte == 0xffu ? 0x7fc0 : 0;                  // byte 255: one NaN element poisons the weight row's sums
        const v4u fb = half ? w.u[js] : w.g[js];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const unsigned u8 = fb[d];
          const bf16x2_t w0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 0), w1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 1);
          const bf16x2_t w2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 2), w3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 3);
          v4i wi = {__builtin_bit_cast(int, w0), __builtin_bit_cast(int, w1), __builtin_bit_cast(int, w2), __builtin_bit_cast(int, w3)};
          if (d == 0) wi[0] |= nan;
          const v8bf B8 = __builtin_bit_cast(v8bf, wi);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const v8bf A8 = __builtin_bit_cast(v8bf, fa[t][4 * js + d]);
            if (half) accu[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8, A8, accu[t], 0, 0, 0);
            else accg[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8, A8, accg[t], 0, 0, 0);
          }
        }
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
  // the bias chunks, behind the last counted wait and in flight across the sum
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
  if (er >= C::TM) return;   // (TM = 32: the first two waves)

  // ---- epilogue: ((w0 + w1) + w2) + w3, one multiply by alpha, one rounding to bf16 -- the W4A16 op's output -- then the activation on the packed bf16 ----
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
  const int row = m0 + er;
  if (row < gend) *(v4i*)(p.D + (size_t)row * I + n0 + 8 * ec) = act;
#endif
}

}  // namespace qamd
