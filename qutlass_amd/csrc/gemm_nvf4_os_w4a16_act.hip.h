// Gate/up grouped W4A16 GEMM on NVFP4 expert weights with the activation fused into its epilogue, for gfx950 (extensions: grouped_matmul_bf16_nvf4_silu_bf16_tn,
// grouped_matmul_bf16_nvf4_swiglu_oai_bf16_tn): bf16 tokens against the (E, 2 I, K/2) [gate | up] NVFP4 weights of an expert layer -- e2m1 codes, one e4m3 scale per 16
// elements, row-major (E, 2 I, K/16), the per-expert global scale in alpha --, and what leaves the kernel is the down GEMM's A operand -- (M, I) bf16 -- bit for bit what
//   silu_and_mul / swiglu_oai_and_mul (grouped_matmul_bf16_nvf4_bf16_tn(...))
// writes; the (M, 2 I) bf16 tensor between the two launches never exists.  The contract of gemm_nvf4_os_w4a16.hip.h carries over with N = 2 I (every finite scale byte
// exact, 0x7f / 0xff poison their weight row, NaN and inf in the tokens, malformed offs, the 2 GiB bounds, GATHER: src_row outside [0, T) reads a zero token, E <= 1024),
// plus I % 32 == 0.  A poisoned gate row or up row is a NaN activation column for that expert's rows.
//
// A kernel of its own (gemm_nvf4_os_w4a16.hip.h and gemm_mx_os_w4a16_act.hip.h keep their code and names).  Four waves, wave w owns the 128-element K stages w, w + 4, ...
// and walks them without a barrier; a workgroup owns TM = 32 (form 622) or 64 (form 623) token rows x 32 ACTIVATION columns n0 .. n0 + 31: the 32 gate weight rows n0 ..
// AND the 32 up weight rows I + n0 .. .
//   tokens    as in the two relatives: a stage row is 256 B = one LDS bank row, LDS-DMA pieces of 4 rows, physical 16-byte chunk = logical chunk ^ (row & 15)
//             (conflict-free, derived in gemm_mx_os_w4a16.hip.h); GATHER puts src_row[r] * 2 K into the row part of the lane offset, bit 31 for a row past the group or
//             an index outside [0, T).
//   weights   NOT in LDS: in a wave-owned stage every 16-byte code chunk is read by exactly one lane of one wave, so LDS would share nothing.  Lane (i32, g) holds
//             K-blocks (32 codes) 2 js + g, js = 0, 1, of gate row n0 + i32 and of up row I + n0 + i32: four buffer_load_dwordx4 (gate / up x js; js adds 32 B, the
//             stage 64 B) and two buffer_load_dwordx2, each row's 8 scale bytes of the stage (the lane uses bytes 2 g, 2 g + 1 of dword js), straight into VGPRs, 20
//             registers per slot.  They are requested with the stage's token pieces and counted in the same vmcnt sequence: LPS = TM / 4 + 6 loads per stage, all landed
//             behind ONE wait.  In a ring the token pieces of the slot's next stage go out as soon as the LDS reads have returned, its weight loads behind the stage's
//             last convert (the registers they land in are the ones that convert frees); the loads of a stage stay together, so the count per stage does not change.
//             Both rows lie below N = 2 I (I % 32 == 0), so no weight load relies on the descriptor's end except the zero-fill of a stage past K.
//   dequant   the NVFP4 kernel's triple per pair of codes -- v_cvt_scalef32_pk_f32_fp4 at scale 1.0, v_pk_mul_f32 by the group's scale, v_cvt_pk_bf16_f32 --, the
//             lane's two group scales per row and js from ONE v_lshrrev and ONE v_cvt_scalef32_pk_f32_fp8: exact for all 254 finite bytes by construction, a zero scale
//             gives +-0, a NaN scale makes all 16 elements of the group NaN -- IEEE arithmetic, no select (derived in gemm_nvf4_os_w4a16.hip.h).
//   MFMAs     per stage and m-tile sixteen v_mfma_f32_32x32x16_bf16, eight gate and eight up, on the same token fragment; a weight fragment is converted once and used
//             for both m-tiles of the 64-row form.  Per accumulator the sequence is the NVFP4 W4A16 kernel's: stages w, w + 4, ... in order, js = 0, 1, d = 0 ... 3
//             inside a stage.  Gate and up alternate per js (gate js, up js): the converts of one half's four fragments have the other half's MFMAs in flight before
//             them, and the two accumulator sets never wait on each other.  Converting all of gate before all of up was not built: it orders the same instructions and
//             holds the up codes four MFMA groups longer.
//   balance   (a DERIVATION from instruction counts, NOT measured: no counter run separates the two pipes; it assumes four cycles for every VALU instruction,
//             v_pk_mul_f32 included, and no overlap inside a wave)  per lane and stage: 2 halves x 2 js x 4 d x 4 pairs x 3 = 192 VALU for the fragments + 2 x 2 x 2 = 8
//             for the scales = 200, of four cycles each = 800 cycles on the wave's SIMD; the MFMAs of the stage are 16 x 32 = 512 cycles (TM = 32) / 32 x 32 = 1024
//             (TM = 64).  The ratios 800 : 512 and 800 : 1024 are the unfused NVFP4 kernel's 400 : 256 and 400 : 512: the 32-row form would be bounded by the
//             converts, the 64-row form by the MFMAs with the converts hidden behind them.
//   slots     SPW per wave.  A stage is TM x 256 B of LDS and nothing else, so LDS = 4 SPW TM 256 B; a CU has 160 KiB:
//               TM = 32 (622):  SPW 1  32 KiB (K <= 512)   2  64 KiB (2 / CU): one shot up to K = 1024, rings of 2 beyond
//               TM = 64 (623):  SPW 1  64 KiB (K <= 512)   2  128 KiB (1 / CU): one shot up to K = 1024, rings of 2 beyond
//             (the relatives' ladder; three or four slots were not built.)  A ring consumes all its slots every round: the stages past K are zero-fill loads (offset
//             bit 31: zero tokens, zero codes, zero scales), acc + 0 x 0, at most one per wave.  Registers: profiles/kernel_resources_bf16_nvf4_act.diff; no scratch.
//   sum       [wave][TM][64] fp32 in the freed stage area -- a row is 16 chunks of 4 fp32, 0-7 gate, 8-15 up, chunk ^ (row & 15), as in the MXFP4 fused kernel --,
//             ((w0 + w1) + w2) + w3, one multiply by alpha[g], one rounding to bf16: the NVFP4 W4A16 op's output row, bit for bit.
//   epilogue  thread (row = tid >> 2, c = tid & 3) holds gate and up columns 8 c .. + 7 of its row as packed bf16; the activation is quantize.hip.h's silu_mul8 /
//             swiglu_oai_mul8<BIAS> (bias chunks of the TILE's expert, one 16-byte load each, requested behind the K loop's last wait); one 16-byte store, masked to the
//             group's rows.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"
#include "gemm_mx_os_w4a16_act.hip.h"   // W4A16ActParams
#include "gemm_nvf4_os_w4a16.hip.h"     // v2u
#include "quantize.hip.h"

namespace qamd {

template <int SPW_, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 128 elements (RING: any K)
struct OsNvW4A16ActCfg {
  static constexpr int TM = TM_, TN = 32, ROWA = 256, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                           // m-tiles of 32 rows
  static constexpr int STAGE = TM * ROWA;                      // tokens only
  static constexpr int NPA = TM / 4, NLB = 6;                  // A pieces / code and scale register loads per stage
  static constexpr int LPS = NPA + NLB;                        // vector memory instructions per stage
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 256;                     // cross-wave sum: [wave] TM x 64 fp32
  static constexpr int LDS_BYTES = KTMAX * STAGE;
  static_assert(LDS_BYTES >= RED, "the stage area holds the sum's scratch");
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// the weight side of one stage in registers: 16 B of gate and of up codes per js, each row's 8 scale bytes of the stage
struct NvW4A16ActB {
  v4u g[2], u[2];
  v2u sg, su;
};

// The epilogue's fp32 adds and multiplies are compiled as the NVFP4 W4A16 kernel's and the streaming activation kernels' are -- the unit's default, no function
// attribute: an IEEE add or multiply has the same bits in its single and its paired (v_pk_*) form except for the sign of a NaN it GENERATES (0 x inf), so "any operands"
// asks for the forms those kernels have (the note above gemm_mx_os_w4a16_act_kernel).  RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at
// most 4 SPW stages, every stage has a slot of its own); GATHER: A rows through p.src_row
template <class C, int ACT, bool RING = false, bool GATHER = false>
__global__ __launch_bounds__(256) void gemm_nvf4_os_w4a16_act_kernel(const W4A16ActParams p) {
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
  const int rowA = p.K << 1, rowB = p.K >> 1, KT = p.K >> 7, KS = p.K >> 4;   // bytes per A / B row, stages, scale bytes per row
  const int er = tid >> 2, ec = tid & 3;                                       // the epilogue's row of the tile and chunk of 8 activation columns

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
  // weights: the lane's gate row i32 and up row I + i32 of the tile (both below N = 2 I: I % 32 == 0), K-block g of the stage; js adds 32 B, the stage 64 B (codes) /
  // 8 B (scales)
  const int vBG = i32 * rowB + 16 * g, vBU = vBG + I * rowB;   // (I rowB < one expert's bytes < 2^31)
  const int vSG = i32 * KS, vSU = vSG + I * KS;

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
  auto issue_b = [&](const int kt, NvW4A16ActB& w) __attribute__((always_inline)) {    // the weights of stage kt into registers (kt >= KT: zeros)
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
    const int hi = (int)0x80000000 & oob;
#pragma unroll
    for (int js = 0; js < 2; ++js) {
      w.g[js] = __builtin_amdgcn_raw_buffer_load_b128(rB, ((vBG + 32 * js) & ~oob) | hi, kt * 64, 0);
      w.u[js] = __builtin_amdgcn_raw_buffer_load_b128(rB, ((vBU + 32 * js) & ~oob) | hi, kt * 64, 0);
    }
    w.sg = __builtin_amdgcn_raw_buffer_load_b64(rSB, (vSG & ~oob) | hi, kt * 8, 0);
    w.su = __builtin_amdgcn_raw_buffer_load_b64(rSB, (vSU & ~oob) | hi, kt * 8, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
  NvW4A16ActB wb[SPW];
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
    const NvW4A16ActB w = wb[u];
#pragma unroll
    for (int js = 0; js < 2; ++js) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {   // 0: gate, 1: up
        // bytes 2 g, 2 g + 1 of the row's dword js: the scales of groups 0, 1 of K-block 2 js + g, as fp32 (NaN for 0x7f / 0xff, +-0 for 0x00 / 0x80)
        const f32x2_t sc = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((half ? w.su : w.sg)[js] >> (16 * g), 1.0f, false);
        const v4u fb = half ? w.u[js] : w.g[js];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const unsigned u8 = fb[d];
          const f32x2_t s2 = {sc[d >> 1], sc[d >> 1]};
          // the two codes of byte b (byte_sel, an immediate) are elements 2 b, 2 b + 1
          const bf16x2_t w0 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 0) * s2, bf16x2_t);
          const bf16x2_t w1 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 1) * s2, bf16x2_t);
          const bf16x2_t w2 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 2) * s2, bf16x2_t);
          const bf16x2_t w3 = __builtin_convertvector(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u8, 1.0f, 3) * s2, bf16x2_t);
          const v4i wi = {__builtin_bit_cast(int, w0), __builtin_bit_cast(int, w1), __builtin_bit_cast(int, w2), __builtin_bit_cast(int, w3)};
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

  // ---- epilogue: ((w0 + w1) + w2) + w3, one multiply by alpha, one rounding to bf16 -- the NVFP4 W4A16 op's output -- then the activation on the packed bf16 ----
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
