// Gate/up grouped NVFP4 GEMM (W4A4) with the activation, the 32 x 32 rotation and the NVFP4 quantizer fused into its epilogue, for gfx950 (extensions:
// grouped_matmul_nvf4_silu_nvf4_tn, grouped_matmul_nvf4_swiglu_oai_nvf4_tn): NVFP4 tokens against the (E, 2 I, K/2) [gate | up] NVFP4 weights of an expert layer, and
// what leaves the kernel is the down GEMM's A operand -- (M, I/2) e2m1 codes with one e4m3 scale per 16 -- byte for byte what
//   fusedSiluMulQuantizeNvGrouped / swiglu_oai_and_mul + fusedGatherQuantizeNvGrouped (grouped_matmul_nvf4_bf16_tn(...), h of 32 x 32, quest or abs_max)
// writes, FOR ANY FINITE OPERANDS, whenever that GEMM runs the tile form this kernel mirrors; the (M, 2 I) bf16 tensor between the launches never exists.
//
// A kernel of its own on gemm_nvf4_kernel<C, false, false, GRP = true>'s tile bodies (gemm_nvf4.hip.h keeps its code and names), the forms the chain's GEMM runs nearly
// everywhere (capi.hip grouped_nv_plan):
//   form 624   64 token rows x 32 activation columns = NvCfg<64, 64, 2, 2>, form 600's body: B rows 0 .. 31 of the tile are gate rows n0 .., rows 32 .. 63 up rows I + n0 ..
//   form 625  128 token rows x 64 activation columns = NvCfg<128, 128, 2, 2>, form 601's body: 64 gate rows, 64 up rows
// Four waves, 2 x 2: wave (wave_m, wave_n = 0) accumulates the GATE columns of its rows, (wave_m, 1) the UP columns of the same rows.  The two-buffer ring, the LDS image
// of a stage (A, B, both scale images), the fragment reads, the on-the-fly dequantisation to f16 and the order of the v_mfma_f32_32x32x16_f16 of every accumulator
// (stage by stage, steps 0 .. 15) are that kernel's, so a gate/up value has the GEMM op's bits whatever the operands: the fp32 sums are the same sums in the same order.
//
// What changes in how operands reach LDS: the B fetch and the B-scale fetch address TWO row segments.
//   B          piece q of a stage = tile rows 8 q .. 8 q + 7 (lane -> row 8 q + (l >> 3), 16-byte chunk (l & 7) ^ ((row >> 1) & 7)): a piece lies wholly in the gate or in
//              the up half (the halves are 32 / 64 rows), so only its source row moves, row + (I - BN / 2) for the up half.  LDS side: the same 1-KiB piece at the same
//              place with the same swizzle -- the DMA writes 64 x 16 contiguous bytes, the fragment reads (ds_read_b128, chunk ^ ((row >> 1) & 7)) hit the banks they hit in
//              the GEMM: conflict-free as there.  Memory side: a piece is still 8 rows x 128 contiguous bytes; the rows of a stage come from two runs of BN / 2 rows
//              instead of one of BN.
//   B scales   dword piece (column tile c, half h): lane l -> tile row 32 (l & 3) + 16 h + (l >> 2); rows < BN / 2 read the gate segment, the rest row + (I - BN / 2).
//              Form 624: l & 3 = 0 is the gate segment, 1 the up segment, 2 and 3 fetch nothing (as in form 600); form 625: 0, 1 gate, 2, 3 up.  The image in LDS and
//              load_scale1's reads are unchanged.
//   vmcnt      the pieces per wave and stage are the GEMM's (NA + NB of operands, 4 of scales), every wait in the K loop is vmcnt(0) in front of the stage's barrier:
//              nothing to re-count there.  The epilogue's own requests (bias chunks, H^T, the global scale) are made BEHIND the K loop's last wait, so no counted wait
//              ever sees them; the compiler places their waits where the values are used.
//   ranges     rows past the weight's 2 I rows fall off the descriptor and read zeros.  I % 64 == 32 on form 625: the last column tile's gate rows 32 .. 63 are the up
//              rows 0 .. 31 (in range, finite or not -- their columns are not stored) and its up rows 32 .. 63 read zeros.
//
// Epilogue, all inside the workgroup (the ring's two stage buffers, 40 / 72 KiB, are free behind the K loop's last barrier):
//   (1) every accumulator times alpha[g], rounded to bf16 in pairs: pack_bf16x2(acc * alpha, ..) -- the GEMM's store value.
//   (2) the TM x 2 TN bf16 gate/up tile is staged in LDS exactly as the GEMM stages its output tile (8-byte granule ^ (row & 15): 8 / 32 KiB), so all FOUR waves share
//       the activation: thread (row, chunk) reads 16 bytes of gate and the 16 bytes of up TN columns further on, and applies quantize.hip.h's silu_mul8 /
//       swiglu_oai_mul8<BIAS>.  Bias: two 16-byte chunks of the TILE's expert.  (A first version handed the up waves' values to the gate waves and ran the
//       activation on those two waves only: the op lost 3 ... 7 % to the chain on the model cells, profiles/calib_grouped_nvf4_act.txt.)
//   (3) the bf16 activation tile is parked behind that, TM rows of TN bf16 + 16 bytes of padding (row pitch 80 / 144 bytes = 20 / 36 dwords: 16 consecutive rows start
//       in 16 different multiples of 4 banks, so the 16-byte reads below do not conflict): 4 KiB + pad = 5 KiB, 16 KiB + pad = 18 KiB.
//   (4) rotation tiles of 32 rows x 32 columns, 2 (form 624: waves 0, 1) or 8 (form 625: two per wave): lane (row = l & 31, half = l >> 5) re-reads 16 contiguous bytes,
//       k = 16 kc + 8 half, the X^T fragment of fused_quantize_body at R = 32, and multiplies by hT[j = row][k ..] = h[k][row] in the same two
//       v_mfma_f32_32x32x16_bf16 steps, kc = 0 then 1.
//   (5) lane (row, half) holds j = 8 q + 4 half + e of its row's block: the lines below ARE fused_quantize_body's "NV: e4m3 per 16" arm (MASK = false, HWCVT = true,
//       BLK = false), restated with their origin -- group statistic per 16, the tile's expert's global scale (abs-max; quest never reads one), the e4m3 scale, the codes.
//   (6) 4 bytes of codes per lane and group, one scale byte per row and group, masked to the group's rows and to columns below I.
#pragma once
#include "gemm_nvf4.hip.h"
#include "quantize.hip.h"

namespace qamd {

struct NvActParams : NvGroupedParams {   // N = 2 I (the weight's rows), tiles_n = cdiv(I, TN); D is not written
  uint8_t* codes;         // (M, I / 2) e2m1
  uint8_t* out_sf;        // flat (M, I / 16) e4m3
  const uint16_t* bias;   // (E, 2 I) bf16 [gate | up], ACT_OAI_BIAS only
  const uint16_t* h;      // (32, 32) bf16 row-major
  const float* gscale;    // (E,) the down projection's per-expert input scale (abs-max only)
  int inter;              // I
  SwigluOaiAct oai;       // ACT_OAI / ACT_OAI_BIAS
};

template <int BM_>
struct NvActCfg : NvCfg<BM_, BM_, 2, 2> {
  using G = NvCfg<BM_, BM_, 2, 2>;                                   // the GEMM body's configuration: form 600's / 601's
  static constexpr int TM = BM_, TN = BM_ / 2;                       // token rows, ACTIVATION columns
  static constexpr int NBLK = TN / 32, ROT = (TM / 32) * NBLK;       // rotation blocks per row, rotation tiles per workgroup
  static constexpr int RING = 2;                                     // stage buffers of the K loop
  static constexpr int ACTROW = TN * 2 + 16, OFF_ACT = TM * G::SROW;  // the parked activation tile, behind the staged gate/up tile (TM x 2 TN bf16)
  static_assert(BM_ == 64 || BM_ == 128, "forms 624 / 625");
  static_assert(OFF_ACT + TM * ACTROW <= RING * G::STAGE_BYTES && G::LDS_BYTES == RING * G::STAGE_BYTES, "the epilogue lives in the freed ring");
};
// the smallest K that fills the ring once (one stage = 256 elements)
constexpr int nvf4_act_ring_k() { return NvActCfg<64>::RING * 2 * NvActCfg<64>::ROWB; }

template <class C, int ACT, int METHOD>
__global__ __launch_bounds__(C::THREADS) void gemm_nvf4_act_kernel(const NvActParams p) {
  constexpr int BM = C::BM, BN = C::BN, MT = C::MT, NT = C::NT, HB = BN / 2;
  static_assert(C::WTN == HB && C::NWAVES == 4, "wave_n = 0: the gate half, 1: the up half");
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass only needs the kernel's symbol)
  GroupTile gt;
  if (!grouped_tile(p.offs, p.E, p.M, BM, p.tiles_n, (int)blockIdx.x, gt)) return;   // an m-tile slot past the real tiles: no work
  const int grp = uniform(gt.g), gend = uniform(gt.row0 + gt.rows), m0 = uniform(gt.row0), n0 = uniform(gt.nt * HB), I = p.inter;
  const float alpha_k = p.alpha[p.n_alpha > 1 ? grp : 0];
  const uint8_t* Bg = p.B + (size_t)grp * p.b_bytes;        // 64-bit: the stacked weight may exceed 2 GiB
  const uint8_t* SFBg = p.SFB + (size_t)grp * p.sfb_bytes;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = uniform(tid >> 6);
  const int wave_m = wave / C::WAVES_N, wave_n = wave % C::WAVES_N;
  const int i32 = lane & 31, g = lane >> 5;

  // ---- gemm_nvf4_kernel<C, false, false, true> from here to the end of the K loop; the two-segment B and B-scale sources are marked [2seg] ----------------------
  const int rowbytes = p.K >> 1, KS = p.K >> 4;
  const int KT = (rowbytes + C::ROWB - 1) / C::ROWB;
  const int CB = (p.K / 16 + 3) >> 2;
  const bool ktail = (rowbytes % C::ROWB) != 0;
  const int seg = I - HB;   // [2seg] tile row r >= HB is weight row n0 + r + seg

  const uint32_t a_off = (uint32_t)m0 * rowbytes, b_off = (uint32_t)n0 * rowbytes;
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A + a_off, (uint32_t)gend * rowbytes - a_off);
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(Bg + b_off, p.b_bytes - b_off);
  const uint32_t sa_off = (uint32_t)m0 * KS, sb_off = (uint32_t)n0 * KS;

  int voffA[C::NA], voffB[C::NB], chA[C::NA], chB[C::NB];
#pragma unroll
  for (int t = 0; t < C::NA; ++t) {
    const int q = wave * C::NA + t, row = 8 * q + (lane >> 3);
    chA[t] = (lane & 7) ^ ((row >> 1) & 7);
    voffA[t] = row * rowbytes + chA[t] * 16;
  }
#pragma unroll
  for (int t = 0; t < C::NB; ++t) {
    const int q = wave * C::NB + t, row = 8 * q + (lane >> 3);
    chB[t] = (lane & 7) ^ ((row >> 1) & 7);
    voffB[t] = (row + (row >= HB ? seg : 0)) * rowbytes + chB[t] * 16;   // [2seg] (< one expert's bytes < 2^31)
  }
  // wave w carries four of the sixteen dword pieces of a stage -- operand w >> 1, column tiles 2 (w & 1), + 1, both halves
  int voffG[4];
  const bool opB = wave >> 1;
  const __amdgpu_buffer_rsrc_t rSG = opB ? make_rsrc(SFBg + sb_off, p.sfb_bytes - sb_off) : make_rsrc(p.SFA + sa_off, (uint32_t)gend * KS - sa_off);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = (lane & 3) * 32 + 16 * (e & 1) + (lane >> 2);
    const int sr = r + ((opB && r >= HB) ? seg : 0);   // [2seg]
    voffG[e] = r < BM ? sr * KS + (2 * (wave & 1) + (e >> 1)) * 4 : 0x7fffffff;
  }

  auto issue_stage = [&](int kt, int buf) {
    char* st = smem + buf * C::STAGE_BYTES;
    const int soff = kt * C::ROWB;
    const bool tail = ktail && (kt == KT - 1);
#pragma unroll
    for (int t = 0; t < C::NA; ++t) {
      int v = voffA[t];
      if (tail && (soff + chA[t] * 16 >= rowbytes)) v = 0x7fffffff;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)(st + (wave * C::NA + t) * 1024), 16, v, soff, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < C::NB; ++t) {
      int v = voffB[t];
      if (tail && (soff + chB[t] * 16 >= rowbytes)) v = 0x7fffffff;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr_t)(st + C::OFF_B + (wave * C::NB + t) * 1024), 16, v, soff, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 2 * (wave & 1) + (e >> 1);
      // a scale column past K is the NEXT ROW's first scales in the row-major layout (K % 256 == 128: the last stage's upper two dwords): out of range -> 0
      const int v = (kt * C::SCT + c < CB) ? voffG[e] : 0x7fffffff;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rSG, (lds_ptr_t)(st + (wave >> 1 ? C::OFF_SB : C::OFF_SA) + c * 512 + (e & 1) * 256), 4, v, kt * 16, 0, 0);
    }
  };

  const int sw = (i32 >> 1) & 7;
  int rdA[4], rdB[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * g + j;
    rdA[j] = (wave_m * C::WTM + i32) * C::ROWB + ((c ^ sw) << 4);
    rdB[j] = C::OFF_B + (wave_n * C::WTN + i32) * C::ROWB + ((c ^ sw) << 4);
  }
  int rdSA[MT], rdSB[NT];   // address of column tile 2g; tile 2g+1 is +512
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int r = wave_m * C::WTM + 32 * t;
    rdSA[t] = C::OFF_SA + ((r >> 7) * C::SCT + 2 * g) * 512 + i32 * 16 + ((r & 127) >> 5) * 4;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int r = wave_n * C::WTN + 32 * t;
    rdSB[t] = C::OFF_SB + ((r >> 7) * C::SCT + 2 * g) * 512 + i32 * 16 + ((r & 127) >> 5) * 4;
  }

  v16f acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  h2_t sa[2][MT][2], sb[2][NT][2];     // [jj & 1][.][jl]
  v4i ca[2][MT], cb[2][NT];            // [j & 1]
  h8_t fa[2][MT], fb[2][NT];           // [s & 1]
  auto load_scales = [&](const char* st, const int jj) __attribute__((always_inline)) {
#pragma unroll
    for (int f = 0; f < MT; ++f) e4m3x4_to_f16(*(const uint32_t*)(st + rdSA[f] + jj * 512), sa[jj & 1][f][0], sa[jj & 1][f][1]);
#pragma unroll
    for (int f = 0; f < NT; ++f) e4m3x4_to_f16(*(const uint32_t*)(st + rdSB[f] + jj * 512), sb[jj & 1][f][0], sb[jj & 1][f][1]);
  };
  auto load_chunks = [&](const char* st, const int j) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < MT; ++t) ca[j & 1][t] = *(const v4i*)(st + rdA[j] + t * 32 * C::ROWB);
#pragma unroll
    for (int t = 0; t < NT; ++t) cb[j & 1][t] = *(const v4i*)(st + rdB[j] + t * 32 * C::ROWB);
  };
  // half of one fragment of step s: dword bytes 2 hh, 2 hh + 1 -> elements 4 hh .. 4 hh + 3 (2 converts + 2 packed multiplies, both exact)
  auto dq_half = [&](const int s, const int f, const int hh) __attribute__((always_inline)) {
    const int j = s >> 2, u = s & 3, jj = j >> 1, jl = j & 1;
    const bool isA = f < MT;
    const int t = isA ? f : f - MT;
    const _Float16 sc = isA ? sa[jj & 1][t][jl][u >> 1] : sb[jj & 1][t][jl][u >> 1];
    const uint32_t w = (uint32_t)(isA ? ca[j & 1][t][u] : cb[j & 1][t][u]);
    const h2_t s2 = {sc, sc};
    h2_t lo, hi;
    if (hh == 0) {
      lo = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0) * s2;
      hi = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1) * s2;
    } else {
      lo = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2) * s2;
      hi = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3) * s2;
    }
    h8_t& d = isA ? fa[s & 1][t] : fb[s & 1][t];
    d[4 * hh + 0] = lo[0]; d[4 * hh + 1] = lo[1]; d[4 * hh + 2] = hi[0]; d[4 * hh + 3] = hi[1];
  };
  auto dq_step = [&](const int s) __attribute__((always_inline)) {
#pragma unroll
    for (int f = 0; f < MT + NT; ++f) { dq_half(s, f, 0); dq_half(s, f, 1); }
  };

  // the epilogue's operands, requested behind the K loop's LAST wait and in flight across the last stage's MFMAs: thread (er = tid / CPR, ec = tid % CPR) applies the
  // activation to chunk ec (8 columns) of rows er, er + RPP, ...: the bias chunks of the tile's own expert; the rotating waves' H^T fragments; the expert's global scale
  constexpr int CPR = HB / 8, RPP = C::THREADS / CPR;
  const int ec = tid % CPR, er = tid / CPR;
  v4i bgate = {0, 0, 0, 0}, bup = {0, 0, 0, 0};
  v8u16 hv[2] = {};
  float gs = 1.0f;
  auto request_epilogue = [&]() __attribute__((always_inline)) {
    if constexpr (ACT == ACT_OAI_BIAS) {
      if (n0 + 8 * ec < I) {   // (a column block past I has no bias: its up chunk would lie past the expert's row)
        const uint16_t* b = p.bias + (size_t)grp * (2 * (size_t)I) + n0 + 8 * ec;
        bgate = *(const v4i*)b;
        bup = *(const v4i*)(b + I);
      }
    }
    if (wave < C::ROT) {   // hT[j = i32][k = 16 kc + 8 g + i] = h[k][i32]
#pragma unroll
      for (int kc = 0; kc < 2; ++kc)
#pragma unroll
        for (int i = 0; i < 8; ++i) hv[kc][i] = p.h[(16 * kc + 8 * g + i) * 32 + i32];
    }
    if constexpr (METHOD == METHOD_ABSMAX) gs = p.gscale[grp];
  };

  issue_stage(0, 0);
  asm volatile("" :: "s"(alpha_k));   // alpha is waited for HERE, behind the first stage's DMA
  for (int kt = 0; kt < KT; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const char* st = smem + (kt & 1) * C::STAGE_BYTES;
    if (kt + 1 < KT) issue_stage(kt + 1, (kt + 1) & 1);
    else request_epilogue();
    load_scales(st, 0);
    load_chunks(st, 0);
    dq_step(0);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + 1 < 16) {
        if (s == 1) load_scales(st, 1);                                        // second scale column tile: used from step 8
        if ((s & 3) == 0 && (s >> 2) + 1 < 4) load_chunks(st, (s >> 2) + 1);   // raw chunk of j + 1: one chunk (4 steps) ahead
        dq_step(s + 1);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[s & 1][n], fa[s & 1][m], acc[m][n], 0, 0, 0);
    }
  }

  const float alpha = alpha_k;
  __syncthreads();   // every wave's reads of the stage buffers are done: they become the epilogue's scratch

  // ---- (1), (2) the GEMM's bf16 store value of every accumulator, staged as the GEMM stages its output tile: row SROW + ((8-byte granule ^ (row & 15)) << 3) ----------
  // acc[m][n][4 q + e] = tile column wave_n WTN + 32 n + 8 q + 4 g + e (gate columns 0 .. HB - 1, then up) of token row wave_m WTM + 32 m + i32
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int trow = wave_m * C::WTM + 32 * m + i32;
        const int cg = (wave_n * C::WTN + 32 * n + 8 * q + 4 * g) >> 2;
        v2i w;
        w[0] = pack_bf16x2(acc[m][n][4 * q + 0] * alpha, acc[m][n][4 * q + 1] * alpha);
        w[1] = pack_bf16x2(acc[m][n][4 * q + 2] * alpha, acc[m][n][4 * q + 3] * alpha);
        *(v2i*)(smem + trow * C::SROW + ((cg ^ (trow & 15)) << 3)) = w;
      }
  __syncthreads();
  // ---- (3) all four waves: 8 gate + 8 up columns of a row -> 8 activations, parked behind the staged tile ------------------------------------------------------------
  auto chunk16 = [&](const int trow, const int chunk) __attribute__((always_inline)) {   // the GEMM's read of a 16-byte chunk of the staged tile
    v4i v = *(const v4i*)(smem + trow * C::SROW + ((((2 * chunk) ^ (trow & 15)) & ~1) << 3));
    if (trow & 1) v = v4i{v[2], v[3], v[0], v[1]};
    return v;
  };
#pragma unroll
  for (int pss = 0; pss < BM / RPP; ++pss) {
    const int trow = pss * RPP + er;
    const v4i yg = chunk16(trow, ec), yu = chunk16(trow, CPR + ec);
    v4i act;
    if constexpr (ACT == ACT_SILU) act = silu_mul8(yg, yu);
    else if constexpr (ACT == ACT_OAI_BIAS) act = swiglu_oai_mul8<true>(yg, yu, bgate, bup, p.oai);
    else act = swiglu_oai_mul8<false>(yg, yu, yg, yu, p.oai);   // (no bias: the last two are not read)
    *(v4i*)(smem + C::OFF_ACT + trow * C::ACTROW + ec * 16) = act;
  }
  __syncthreads();

  // ---- (4) rotation tile t = wave, wave + 4: rows 32 (t / NBLK) .., columns 32 (t % NBLK) .. -- fused_quantize_body at R = 32 -------------------------------------
  const int row = i32, half = g;
#pragma unroll
  for (int t0 = 0; t0 < C::ROT; t0 += 4) {
    const int t = t0 + wave;
    if (t >= C::ROT) break;
    const int mt = t / C::NBLK, blk = t % C::NBLK;
    v16f ra;
#pragma unroll
    for (int r = 0; r < 16; ++r) ra[r] = 0.f;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {   // X^T chunk kc of lane (row, half) = act[row][16 kc + 8 half .. + 7]
      const v8bf xf = *(const v8bf*)(smem + C::OFF_ACT + (32 * mt + row) * C::ACTROW + blk * 64 + (2 * kc + half) * 16);
      ra = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, hv[kc]), xf, ra, 0, 0, 0);
    }
    // ra[4q+e] = y[row][8q + 4 half + e]
    const int orow = m0 + 32 * mt + row;
    const bool ok = orow < gend && n0 + 32 * blk < I;
    const size_t grp32 = (size_t)orow * (I >> 5) + ((n0 >> 5) + blk);   // the quantizer's flat 32-group index of an (M, I) operand

    // ---- (5) quantize.hip.h fused_quantize_body, "NV: e4m3 per 16" arm with MASK = false, HWCVT = true, BLK = false -- its lines, in its order ----------------------
    // lane holds j = 8q + 4 half + e: q in {0,1} belong to 16-group 2*grp32, q in {2,3} to +1
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      float v8[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v8[r] = ra[sub * 8 + r];
      float out_scale;
      uint32_t sfb;
      bool nan_risk;   // the group may hold NaNs (see there)
      if (METHOD == METHOD_ABSMAX) {
        float m = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) m = fmaxf(m, fabsf(v8[r]));   // group statistic per 16: a lane's 8, then the partner half's
        m = xhalf_max(m);
        nan_risk = m == 0.f || !(m < __builtin_inff());
        float sf = gs * (m * (1.0f / 6.0f));                      // the tile's expert's global scale (GSCALE: the row's expert)
        sfb = e4m3_encode_pos(sf);                                // the e4m3 scale
        sf = e4m3_decode_pos(sfb);
        out_scale = (sf != 0.f) ? __frcp_rn(sf * __frcp_rn(gs)) : 0.0f;
      } else {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          s1 += v8[r];
          s2 = fmaf(v8[r], v8[r], s2);
        }
        s1 = xhalf_add(s1);
        s2 = xhalf_add(s2);
        float mean = s1 * 0.0625f;
        float var = fmaf(-mean, mean, s2 * 0.0625f);   // (no clamp at 0: a NaN scale byte as in the reference, see there)
        if (__builtin_expect(!(var > s2 * (0.0625f * 0.0009765625f)), 0)) {   // whether it is negative depends on the order of the additions: the reference's
          quest_sums_in_reference_order<2>(v8, 0, s1, s2);
          mean = s1 * 0.0625f;
          var = fmaf(-mean, mean, s2 * 0.0625f);
        }
        nan_risk = !(var >= 0.f);
        const float sc = (float)((double)sqrtf(var) * (2.92247856 / 6.) + 1e-8);   // quest: no global scale
        sfb = e4m3_encode_pos(sc);
        const float sq = e4m3_decode_pos(sfb);
        out_scale = (sq > 0.f) ? __frcp_rn(sq) : 0.0f;
      }
      float tq[8];
      scale_pk<8>(v8, 0, out_scale, tq);
      if (__builtin_expect(nan_risk, 0)) {
#pragma unroll
        for (int r = 0; r < 8; ++r) tq[r] = nan_to_pinf(tq[r]);
      }
      // the codes: 8 values = bytes {0,1,4,5} + 2*half of the 8-byte group: halfwords H[half], H[2+half]
      const uint32_t P = e2m1_pack8<true>(tq);
      auto swp = __builtin_amdgcn_permlane32_swap(P, P, false, false);
      // half 0: swp[0] = own P (H0,H2), swp[1] = partner P (H1,H3); half 1: swp[0] = partner P (H0,H2), swp[1] = own P (H1,H3)
      const uint32_t X = swp[0], Y = swp[1];
      const uint32_t d0 = (X & 0xffffu) | (Y << 16);          // bytes 0..3
      const uint32_t d1 = (X >> 16) | (Y & 0xffff0000u);      // bytes 4..7
      // ---- (6) masked to the group's rows and to the activation's columns
      if (ok) {
        const size_t grp16 = grp32 * 2 + sub;
        *(uint32_t*)(p.codes + grp16 * 8 + half * 4) = half ? d1 : d0;
        if (half == 0) p.out_sf[grp16] = (uint8_t)sfb;
      }
    }
  }
#endif
}

}  // namespace qamd
