// Gate/up grouped MXFP4 GEMM (W4A4) with the activation, the 32 x 32 rotation and the MXFP4 quantizer fused into its epilogue, for gfx950 (extensions:
// grouped_matmul_mxf4_silu_mxf4_tn, grouped_matmul_mxf4_swiglu_oai_mxf4_tn): MXFP4 tokens against the (E, 2 I, K/2) [gate | up] MXFP4 weights of an expert layer, and
// what leaves the kernel is the down GEMM's A operand -- (M, I/2) e2m1 codes with one e8m0 scale per 32 -- byte for byte what
//   fusedSiluMulQuantizeMx / fusedSwigluOaiQuantizeMx (grouped_matmul_mxf4_bf16_tn(...), h of 32 x 32, quest or abs_max)
// writes wherever the GEMM's fp32 sums do not depend on their order (gemm_mx_os.hip.h's header: every split plan's regime); the (M, 2 I) bf16 tensor between the two
// launches never exists.
//
// A kernel of its own on gemm_mx_os.hip.h's wave-owned K stages (that header and gemm_mx_os_w4a8_act.hip.h keep their code and names): four waves, wave w owns stages
// w, w + 4, ... of 256 K elements, LDS-DMA pieces XOR-swizzled at the source, v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = blgp = 4 (both fragments e2m1).  The tile
// is the W4A8 fused kernel's: TM rows x 32 ACTIVATION columns n0 .. n0 + 31 -- the 32 gate rows n0 .. of the weight AND the 32 up rows I + n0 .. -- which is one MX
// scale group AND one rotation block of the output, so rotation, group statistic, scale and codes all stay inside the workgroup.
//   stage     TM x 128 B of A and 64 weight rows x 128 B (gate rows, then up rows) as pieces of 8 rows, 16-byte chunk ^ ((row >> 1) & 7) -- gemm_mx_os.hip.h's; one
//             dword piece of A scales per m-tile, one of the gate rows' and one of the up rows' B scales (lane (i32, g): bytes 8 kt + 4 g .. + 3 of row i32's K / 32).
//             (TM + 64) x 128 B + (MT + 2) x 256 B: 12.75 KiB for TM = 32, 17 KiB for TM = 64.  K % 256 == 128: the last stage's chunks 4 .. 7 and the scale dwords of
//             lane half 1 fall off the descriptors and read zeros, as there.
//   MFMAs     eight per m-tile and stage (four k-slices x gate / up) on one token fragment, each accumulator in gemm_mx_os_kernel's order (stage by stage, js = 0 .. 3).
//   slots     SPW per wave, 4 SPW stages per workgroup; LDS = 4 SPW STAGE, at least the sum's scratch plus the parked activation tile.  A CU has 160 KiB:
//               TM = 32:  SPW 1   51 KiB (3 / CU)   2  102 KiB (1 / CU)   3  153 KiB (1 / CU)      one shot up to K = 3072, rings of 3 beyond
//               TM = 64:  SPW 1   69 KiB (2 / CU; the scratch + the tile)   2  136 KiB (1 / CU)    one shot up to K = 2048, rings of 2 beyond
//             (vmcnt's 63 outstanding pieces allow SPW 4 / 3 at 15 / 20 pieces per stage; the LDS stops the ladder first.)  So K <= 1024 keeps three 32-row or two
//             64-row workgroups on a CU.
//             Stages of 128 elements (64-byte rows, the W4A8 kernels' B geometry) were worked out against this: 6.5 / 8.5 KiB per stage, 8 / 10 pieces, SPW up to 6 / 4 --
//             one shot up to the SAME K (3072 / 2048), two 64-row workgroups up to the same K = 1024; the one gain is two 32-row workgroups per CU for 1024 < K <= 1536
//             (SPW 3 = 78 KiB).  Against it: every request fetches half a 128-byte line per row, a K extent takes twice the waits and scale pieces (K = 1536: 96 pieces
//             per workgroup against 90), and a stage stops being the chain GEMM's stage.  256-element stages it is.
//   sum       [wave][TM][64] fp32 in the freed stage area (the W4A8 fused kernel's layout), ((w0 + w1) + w2) + w3, one multiply by alpha[g], one rounding to bf16: the
//             wave-owned GEMM forms' output value bit for bit, the ring form 593's wherever the sums are exact.
//   epilogue  (a) thread (row = tid >> 2, c = tid & 3) holds gate and up columns 8 c .. + 7 of its row as packed bf16; the activation is quantize.hip.h's silu_mul8 /
//                 swiglu_oai_mul8<BIAS> (bias chunks of the TILE's expert, requested behind the K loop's last wait); the 8 activations are parked in LDS behind the
//                 sum's scratch, a row 80 bytes apart.  TM = 64: all four waves; TM = 32: 128 rows x chunks, waves 0 and 1.
//             (b) wave t < MT rotates m-tile t: lane (row = l & 31, half = l >> 5) re-reads 16 contiguous bytes, k = 16 kc + 8 half, the X^T fragment of
//                 fused_quantize_body at R = 32, and multiplies by the H^T fragment hT[j = row][k = 16 kc + 8 half ..] = h[k][row] (sixteen 2-byte loads per lane,
//                 requested behind the K loop by the rotating waves only: 2 KiB per workgroup, once) in the same two v_mfma_f32_32x32x16_bf16 steps, kc = 0 then 1.
//                 A rotation is ONE accumulator chain of one wave, so it cannot be spread further: the waves past MT have nothing left to do.
//             (c) lane (row, half) now holds j = 8 q + 4 half + e of its row's one group: the quantizer's register layout.  From here the lines ARE
//                 fused_quantize_body's MX e2m1 arm (METHOD quest / abs-max, no clip mask, hardware convert), restated below with their origin -- quantize.hip.h's
//                 kernels are not touched -- down to the store: 8 bytes of codes per lane, one scale byte per row and tile, masked to the group's rows.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"
#include "gemm_mx_os_w4a8_act.hip.h"   // QAMD_NO_PACKED_F32
#include "quantize.hip.h"

namespace qamd {

struct Mxf4ActParams : GroupedParams {   // N = 2 I (the weight's rows), tiles_n = I / 32; D is not written
  uint8_t* codes;        // (M, I / 2) e2m1
  uint8_t* out_sf;       // flat (M, I / 32) e8m0
  const uint16_t* bias;  // (E, 2 I) bf16 [gate | up], ACT_OAI_BIAS only
  const uint16_t* h;     // (32, 32) bf16 row-major
  int inter;             // I
  SwigluOaiAct oai;      // ACT_OAI / ACT_OAI_BIAS
};

template <int SPW_, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 256 elements (RING: any K)
struct OsMxf4ActCfg {
  static constexpr int TM = TM_, TN = 32, ROWB = 128, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                                                        // m-tiles of 32 rows
  static constexpr int OFF_B = TM * ROWB, OFF_BU = OFF_B + 32 * ROWB, OFF_S = OFF_BU + 32 * ROWB, OFF_SB = OFF_S + MT * 256, STAGE = OFF_SB + 512;
  static constexpr int NPA = TM / 8, NPB = 8;                                               // A / B pieces per stage
  static constexpr int LPS = NPA + NPB + MT + 2;                                            // LDS-DMA instructions per stage
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 256;                                                  // cross-wave sum: [wave] TM x 64 fp32
  static constexpr int ACTROW = 80, OFF_ACT = RED;                                          // the parked activation tile: TM rows of 32 bf16, 16 bytes of padding each
  static constexpr int EPI = RED + TM * ACTROW;
  static constexpr int LDS_BYTES = KTMAX * STAGE > EPI ? KTMAX * STAGE : EPI;
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
// slots per wave that fit the LDS: 12 stages of 12.75 KiB = 153 KiB, 8 of 17 KiB = 136 KiB
constexpr int os_mxf4_act_smax(int TM) { return TM == 32 ? 3 : 2; }
// the largest K form `tall ? 64 : 32` rows runs in one shot (the ring starts at the next multiple of 128)
constexpr int os_mxf4_act_one_shot_k(int TM) { return 4 * os_mxf4_act_smax(TM) * 256; }

// QAMD_NO_PACKED_F32 (gemm_mx_os_w4a8_act.hip.h): this function's fp32 arithmetic is compiled to the single forms; scale_pk's v2f products become two v_mul_f32 with the
// same bits.  RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at most 4 SPW stages, every stage has a slot of its own)
template <class C, int ACT, int METHOD, bool RING = false>
__global__ __launch_bounds__(256) QAMD_NO_PACKED_F32 void gemm_mx_os_mxf4_act_kernel(const Mxf4ActParams p) {
  constexpr int SPW = C::SPW, LPS = C::LPS, MT = C::MT;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the kernel's symbol)
  GroupTile gt;
  if (!grouped_tile(p.offs, p.E, p.M, C::TM, p.tiles_n, (int)blockIdx.x, gt)) return;   // an m-tile slot past the real tiles: no work
  asm volatile("" :: "s"(p.A), "s"(p.codes), "s"(p.K), "s"(p.b_bytes), "s"(p.alpha));   // all scalar argument loads in one round
  const int grp = uniform(gt.g), gend = uniform(gt.row0 + gt.rows), m0 = uniform(gt.row0), n0 = uniform(gt.nt * 32), I = p.inter;
  const float alpha = p.alpha[p.n_alpha > 1 ? grp : 0];
  const uint8_t* Bg = p.B + (size_t)grp * p.b_bytes;        // 64-bit: the stacked weight may exceed 2 GiB
  const uint8_t* SFBg = p.SFB + (size_t)grp * p.sfb_bytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), i32 = lane & 31, g = lane >> 5;
  const int rowbytes = p.K >> 1, KT = (rowbytes + C::ROWB - 1) / C::ROWB, KB = p.K >> 5;   // bytes per row, stages, scale bytes per row
  const int tailbytes = rowbytes - (KT - 1) * C::ROWB;                                    // bytes per row of the last stage (128 or 64)
  const int er = tid >> 2, ec = tid & 3;                                                  // (a): row of the tile and chunk of 8 activation columns

  // ---- LDS-DMA sources: gemm_mx_os_kernel's (grouped, row-major scales), with the up rows I weight rows behind the gate rows ---------------------
  const uint32_t a_off = (uint32_t)m0 * rowbytes, b_off = (uint32_t)n0 * rowbytes;
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A + a_off, (uint32_t)gend * rowbytes - a_off), rB = make_rsrc(Bg + b_off, p.b_bytes - b_off);
  // piece qq = rows 8 qq .. + 7; lane -> row 8 qq + (l >> 3), physical chunk l & 7 = logical chunk ^ ((row >> 1) & 7): only the parity of qq matters
  int vP[2], chP[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    chP[par] = (lane & 7) ^ (((lane >> 4) + 4 * par) & 7);
    vP[par] = (lane >> 3) * rowbytes + (chP[par] << 4);
  }
  const int rstep = 8 * rowbytes, upB = I * rowbytes;   // (I rowbytes < one expert's bytes < 2^31)
  const uint32_t sa_off = (uint32_t)m0 * KB, sb_off = (uint32_t)n0 * KB;
  const __amdgpu_buffer_rsrc_t rSA = make_rsrc(p.SFA + sa_off, (uint32_t)gend * KB - sa_off), rSB = make_rsrc(SFBg + sb_off, p.sfb_bytes - sb_off);
  const int vSA = i32 * KB + 4 * g, vSBu = (I + i32) * KB + 4 * g;   // (+ 32 t KB for m-tile t; the gate rows' dword is vSA's)

  auto issue = [&](const int kt, const int slot) __attribute__((always_inline)) {   // stage kt into slot `slot` of this wave (kt >= KT: every piece out of range -> zeros)
    char* st = smem + (wave * SPW + slot) * C::STAGE;
    int tail = (kt == KT - 1) ? tailbytes : C::ROWB;
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(tail), "+v"(oob));
    const int soff = kt * C::ROWB;
#pragma unroll
    for (int t = 0; t < C::NPA + C::NPB; ++t) {   // B pieces 0 .. 3: gate rows 8 qq ..; 4 .. 7: up rows
      const bool isB = t >= C::NPA;
      const int qq = isB ? t - C::NPA : t, par = qq & 1;
      const int o = oob | ((chP[par] << 4) < tail ? 0 : -1);
      const int src = vP[par] + (isB ? (qq & 3) * rstep + (qq >> 2) * upB : qq * rstep);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(isB ? rB : rA, (lds_ptr_t)(st + (isB ? C::OFF_B : 0) + qq * 1024), 16, (src & ~o) | ((int)0x80000000 & o), soff, 0, 0);
    }
    const int os = (kt < KT && 8 * kt + 4 * g < KB) ? 0 : -1;   // K-blocks past K / 32 are the next row's
#pragma unroll
    for (int t = 0; t < MT; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rSA, (lds_ptr_t)(st + C::OFF_S + t * 256), 4, ((vSA + 32 * t * KB) & ~os) | ((int)0x80000000 & os), kt * 8, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSB, (lds_ptr_t)(st + C::OFF_SB), 4, (vSA & ~os) | ((int)0x80000000 & os), kt * 8, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSB, (lds_ptr_t)(st + C::OFF_SB + 256), 4, (vSBu & ~os) | ((int)0x80000000 & os), kt * 8, 0, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
#pragma unroll
  for (int j = 0; j < SPW; ++j) issue(wave + 4 * j, j);

  const int sw = (i32 >> 1) & 7;
  v16f accg[MT], accu[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { accg[t][r] = 0.f; accu[t][r] = 0.f; }
  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };

  // one stage out of slot u; RING: kt_next (>= KT: zeros) is requested into the slot as soon as the reads have returned
  auto consume = [&](const int u, const int kt_next) __attribute__((always_inline)) {
    const char* st = smem + (wave * SPW + u) * C::STAGE;
    v4i fa[MT][4], fbg[4], fbu[4];
#pragma unroll
    for (int js = 0; js < 4; ++js) {   // logical chunk 4 g + js: lane half g owns K-blocks 4 g .. 4 g + 3 of the stage
      const int off = i32 * C::ROWB + (((4 * g + js) ^ sw) << 4);
#pragma unroll
      for (int t = 0; t < MT; ++t) fa[t][js] = *(const v4i*)(st + t * 32 * C::ROWB + off);
      fbg[js] = *(const v4i*)(st + C::OFF_B + off);
      fbu[js] = *(const v4i*)(st + C::OFF_BU + off);
    }
    int sa[MT], sbg, sbu;
#pragma unroll
    for (int t = 0; t < MT; ++t) sa[t] = *(const int*)(st + C::OFF_S + t * 256 + lane * 4);
    sbg = *(const int*)(st + C::OFF_SB + lane * 4);
    sbu = *(const int*)(st + C::OFF_SB + 256 + lane * 4);
    fence();   // every read issued before the first MFMA
    if constexpr (RING) {
      if constexpr (MT == 1)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]), "+v"(fbg[0]), "+v"(fbg[1]), "+v"(fbg[2]), "+v"(fbg[3]), "+v"(fbu[0]),
                     "+v"(fbu[1]), "+v"(fbu[2]), "+v"(fbu[3]), "+v"(sa[0]), "+v"(sbg), "+v"(sbu) :: "memory");   // the slot is free
      else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]), "+v"(fa[MT - 1][0]), "+v"(fa[MT - 1][1]), "+v"(fa[MT - 1][2]),
                     "+v"(fa[MT - 1][3]), "+v"(fbg[0]), "+v"(fbg[1]), "+v"(fbg[2]), "+v"(fbg[3]), "+v"(fbu[0]), "+v"(fbu[1]), "+v"(fbu[2]), "+v"(fbu[3]), "+v"(sa[0]),
                     "+v"(sa[MT - 1]), "+v"(sbg), "+v"(sbu) :: "memory");
      issue(kt_next, u);
      fence();
    }
    // cbsz = format of srcA (the weight fragment), blgp = format of srcB (the token fragment): 4 = e2m1; op_sel js picks the scale byte of K-block 4 g + js
    static_for<0, 4>([&](auto jc) __attribute__((always_inline)) {
      constexpr int js = decltype(jc)::value;
      const v8i G8 = {fbg[js][0], fbg[js][1], fbg[js][2], fbg[js][3], 0, 0, 0, 0};
      const v8i U8 = {fbu[js][0], fbu[js][1], fbu[js][2], fbu[js][3], 0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const v8i A8 = {fa[t][js][0], fa[t][js][1], fa[t][js][2], fa[t][js][3], 0, 0, 0, 0};
        accg[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(G8, A8, accg[t], 4, 4, js, sbg, js, sa[t]);
        accu[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(U8, A8, accu[t], 4, 4, js, sbu, js, sa[t]);
      }
    });
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
  // behind the last counted wait (the K loop's vmcnt immediates count LDS-DMA pieces only) and in flight across the sum: the bias chunks of the tile's own expert (in
  // range whatever the row) and, in the waves that will rotate, the H^T fragments -- hT[j = i32][k = 16 kc + 8 g + i] = h[k][i32]
  v4i bgate = {0, 0, 0, 0}, bup = {0, 0, 0, 0};
  if constexpr (ACT == ACT_OAI_BIAS) {
    if (er < C::TM) {
      const uint16_t* b = p.bias + (size_t)grp * (2 * (size_t)I) + n0 + 8 * ec;
      bgate = *(const v4i*)b;
      bup = *(const v4i*)(b + I);
    }
  }
  v8u16 hv[2] = {};
  if (wave < MT) {
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int i = 0; i < 8; ++i) hv[kc][i] = p.h[(16 * kc + 8 * g + i) * 32 + i32];
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

  // ---- (a) ((w0 + w1) + w2) + w3, one multiply by alpha, one rounding to bf16 -- the GEMM op's output -- then the activation, parked for the rotation -------
  if (er < C::TM) {
    v4i yg, yu;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {   // chunks 2 ec + hh of the gate and of the up half
      v4f sg[4], su[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const char* rowp = smem + (w * C::TM + er) * 256;
        sg[w] = *(const v4f*)(rowp + (((2 * ec + hh) ^ (er & 15)) << 4));
        su[w] = *(const v4f*)(rowp + (((8 + 2 * ec + hh) ^ (er & 15)) << 4));
      }
      v4f tg, tu;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        tg[e] = ((sg[0][e] + sg[1][e]) + sg[2][e]) + sg[3][e];
        tu[e] = ((su[0][e] + su[1][e]) + su[2][e]) + su[3][e];
      }
      yg[2 * hh] = (int)pack_bf16x2(tg[0] * alpha, tg[1] * alpha);
      yg[2 * hh + 1] = (int)pack_bf16x2(tg[2] * alpha, tg[3] * alpha);
      yu[2 * hh] = (int)pack_bf16x2(tu[0] * alpha, tu[1] * alpha);
      yu[2 * hh + 1] = (int)pack_bf16x2(tu[2] * alpha, tu[3] * alpha);
    }
    v4i act;
    if constexpr (ACT == ACT_SILU) act = silu_mul8(yg, yu);
    else if constexpr (ACT == ACT_OAI_BIAS) act = swiglu_oai_mul8<true>(yg, yu, bgate, bup, p.oai);
    else act = swiglu_oai_mul8<false>(yg, yu, yg, yu, p.oai);   // (no bias: the last two are not read)
    *(v4i*)(smem + C::OFF_ACT + er * C::ACTROW + ec * 16) = act;   // (behind the scratch: other threads may still be reading it)
  }
  __syncthreads();
  if (wave >= MT) return;

  // ---- (b) the rotation of m-tile `wave`: fused_quantize_body at R = 32 -- X^T chunk kc of lane (row, half) = act[row][16 kc + 8 half .. + 7] ----------------
  const int row = i32, half = g;
  v16f acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    const v8bf xf = *(const v8bf*)(smem + C::OFF_ACT + (32 * wave + row) * C::ACTROW + (2 * kc + half) * 16);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, hv[kc]), xf, acc, 0, 0, 0);
  }
  // acc[4q+e] = y[row][8q + 4 half + e]

  // ---- (c) quantize.hip.h fused_quantize_body, "MX: e8m0 per 32" arm with MASK = false, HWCVT = true, BLK = false -- its lines, in its order -----------------
  float scale;
  bool nan_risk;   // the group may hold NaNs (see there); only such groups pay for the NaN -> 0x7 fix-up
  if (METHOD == METHOD_ABSMAX) {
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(acc[r]));
    m = xhalf_max(m);
    scale = m + 1e-8f;
    nan_risk = m == 0.f;
  } else {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s1 += acc[r];
      s2 = fmaf(acc[r], acc[r], s2);
    }
    s1 = xhalf_add(s1);
    s2 = xhalf_add(s2);
    float mean = s1 * 0.03125f;
    float var = fmaf(-mean, mean, s2 * 0.03125f);
    if (__builtin_expect(!(var > s2 * (0.03125f * 0.0009765625f)), 0)) {   // sign of the variance at stake: the reference's summation order
      quest_sums_in_reference_order<4>(acc, 0, s1, s2);
      mean = s1 * 0.03125f;
      var = fmaf(-mean, mean, s2 * 0.03125f);
    }
    scale = 1.0f;
    if (var >= 0.f) scale = (float)((double)sqrtf(var) * (2.92247856 / 6.) + 1e-8);
    nan_risk = !(var >= 0.f);
  }
  const uint32_t e8 = (__float_as_uint(scale) >> 23) & 0xffu;   // floor to 2^e, keep exponent
  int sh = 127 - (int)e8;                                       // y / 2^(e8-127) == ldexp(y, sh)
  const bool inf_scale = e8 == 255u;                            // finite / inf = 0, inf / inf = NaN -> 0x7: multiply by 0 first, convert with unit scale
  if (__builtin_expect(inf_scale, 0)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc[r] * 0.0f;
    sh = 0;
  }
  if (__builtin_expect(inf_scale || nan_risk, 0)) {   // NaN -> +inf -> code 0x7
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = nan_to_pinf(acc[r]);
  }
  float t[16];
  float cs = 1.0f;   // scale operand of the hardware convert
  if (METHOD == METHOD_ABSMAX) {
    scale_pk<16>(acc, 0, ldexpf(3.0f, sh), t);   // (y * 2^sh) * 3 == y * (3 * 2^sh)
  } else {
    cs = inf_scale ? 1.0f : __uint_as_float(e8 << 23);   // y / 2^(e8-127) happens inside the convert
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = acc[r];
  }
  // bytes: q-th group of 4 values -> group bytes 4q + 2 half, 4q + 2 half + 1
  const uint32_t P = e2m1_pack8<true>(t, cs);       // halfwords H[0+half], H[2+half]
  const uint32_t Q = e2m1_pack8<true>(t + 8, cs);   // halfwords H[4+half], H[6+half]
  auto swp = __builtin_amdgcn_permlane32_swap(P, Q, false, false);
  const uint32_t X = swp[0], Y = swp[1];
  // half 0: X = own P, Y = partner P ; half 1: X = partner Q, Y = own Q
  v2i o;
  o[0] = (int)((X & 0xffffu) | (Y << 16));
  o[1] = (int)((X >> 16) | (Y & 0xffff0000u));
  const int orow = m0 + 32 * wave + row;
  if (orow < gend) {   // (grp32 = orow * (I / 32) + the column tile: the quantizer's flat group index of an (M, I) operand)
    const size_t grp32 = (size_t)orow * (I >> 5) + gt.nt;
    *(v2i*)(p.codes + grp32 * 16 + half * 8) = o;
    if (half == 0) p.out_sf[grp32] = (uint8_t)e8;
  }
#endif
}

}  // namespace qamd
