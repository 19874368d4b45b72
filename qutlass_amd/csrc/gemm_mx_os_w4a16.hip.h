// Grouped W4A16 GEMM for gfx950 (extension: grouped_matmul_bf16_mxf4_bf16_tn): bf16 tokens, unquantised and without scales, against MXFP4 stacked expert weights
// (e2m1 codes, row-major e8m0 scales: what fusedQuantizeMx writes, what a gpt-oss checkpoint stores and what grouped_matmul_mxf4_bf16_tn / ..._mxf8_mxf4_... read).
//
// CONTRACT.  out[r, n] = bf16( alpha[g] * sum_k x[r, k] * w[g, n, k] ) for every row r of group g, w = e2m1(code) * 2^(sfb - 127) HELD AS bf16.  Every product of two
// bf16 is exact in fp32; the sums are fp32 (the MFMA's, then ((w0 + w1) + w2) + w3 across the waves); one fp32 multiply by alpha[g], one rounding to bf16.
//   * w is exact whenever it is 0 or 2^-126 <= |w| <= bf16's largest finite value: every code under the scale bytes 2 ... 252 is.
//   * scale byte 255 (the e8m0 NaN) makes EVERY output of that weight row n NaN for the rows of that expert: one element of the block's fragment is set to NaN, and
//     x * NaN is NaN for every x (0 and inf included).  (byte << 23 alone is +inf: 0 * inf, inf * code 0 ... would leave finite and inf outputs.)
//   * bytes 0, 1, 253, 254 are OUTSIDE the exact contract: byte 0 is taken as the fp32 bits 0 (w = 0 where the mathematics say code * 2^-127), byte 1 gives
//     bf16 subnormals (0.5 * 2^-126), 253 / 254 overflow bf16 for the larger codes (inf).
//   * NaN and inf in x propagate as in fp64 arithmetic on the same operands (inf * 0 = NaN, inf - inf = NaN).
//   * K % 128 == 0, N % 8 == 0, E <= 1024, the token matrix (M * 2K bytes) and one expert's weight (N * K/2) below 2 GiB; rows at or past offs[E - 1] are not written;
//     malformed offs as in the other grouped ops (gemm_mx_grouped.hip.h: clamped to [0, M], a decreasing offset is an empty group).
//   * GATHER (src_row (M,) int32): A is the UNSORTED (T, K) tokens and row r of the output reads x[src_row[r]]; T * K * 2 < 2 GiB.  An index outside [0, T) reads an
//     all-zero token and never addresses memory; src_row itself is read at rows below the group's end only.
//
// The mixed-width form of gemm_mx_os.hip.h's wave-owned tile body in its GRP + RM mode -- a kernel of its own, as gemm_mx_os_w4a8.hip.h is, so that every kernel of
// those headers keeps its code and its name.  A stage is 128 K elements:
//   A rows of a stage are 256 bytes = one whole LDS bank row.  One LDS-DMA piece covers 4 rows (lane l -> row 4 qq + (l >> 4), physical 16-byte chunk l & 15).  The 16
//     lanes of a ds_read_b128 group read the same logical chunk of rows {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}; at a 256-byte pitch every row starts at slot 0, so the
//     16 rows must XOR 16 distinct values into the chunk: row & 3 takes all four values within each run of four rows, and row >> 2 of the runs is {0, 3, 5, 6} or
//     {1, 2, 4, 7} -- distinct mod 4 -- so physical chunk = logical chunk ^ (row & 15) puts the 16 lanes on the 16 slots.  At the source only qq & 3 enters beside the lane:
//     (4 qq + (l >> 4)) & 15 = 4 (qq & 3) | (l >> 4).
//   B rows are 64 bytes and the scales one dword per row and stage, fetched and read exactly as gemm_mx_os_w4a8.hip.h does (16 rows per piece, chunk ^ ((row >> 2) & 3)).
//   Per stage EIGHT v_mfma_f32_32x32x16_bf16 per m-tile.  Lane (i32, g) holds B chunks 2 js + g (K-block 2 js + g of the stage, 32 codes), js = 0, 1; dword d of the
//     chunk -- 8 codes, k = 32 (2 js + g) + 8 d ... + 7 -- goes through four v_cvt_scalef32_pk_bf16_fp4 (byte_sel 0 ... 3: the two codes of byte b are elements 2 b, 2 b + 1)
//     with the block's scale as fp32 (byte << 23) and is the 8-element operand of MFMA (js, d).  The A operand of that MFMA is the lane's row's bf16 at the same k:
//     16-byte chunk 4 (2 js + g) + d of the row.  (The K order inside a stage is free as long as both fragments agree and every code meets its own block's scale.)
// One shot while 4 SPW stages hold the tile's K extent, wave-owned rings of SPW slots beyond: a 32-row tile's stage is 10.25 KiB (3 slots per wave = 123 KiB), a 64-row
// tile's 18.25 KiB (2 slots = 146 KiB).  Epilogue as in the W4A8 kernel.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"

namespace qamd {

struct W4A16Params : GroupedParams {   // SFA / sfa_bytes unused (bf16 tokens carry no scales); a_bytes = M x 2 K
  const int* src_row;   // GATHER kernels: (M,) token index of every sorted row; A is then the unsorted (T, K) tokens
  int T;                // GATHER kernels: rows of A
};

template <int SPW_, int TN_ = 32, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 128 elements (RING: any K)
struct OsW4A16Cfg {
  static constexpr int TM = TM_, TN = TN_, ROWA = 256, ROWB = 64, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                                                        // m-tiles of 32 rows
  static constexpr int OFF_B = TM * ROWA, OFF_SB = OFF_B + 32 * ROWB, STAGE = OFF_SB + 256;  // (the B area keeps 32 rows: the fragment reads span them)
  static constexpr int NPA = TM / 4, NPB = TN / 16;                                         // A / B pieces per stage
  static constexpr int LPS = NPA + NPB + 1;                                                 // LDS-DMA instructions per stage
  static_assert(TN == 32 || TN == 16, "tile width");
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 128;                                                  // cross-wave sum: [wave] TM x 32 fp32
  static constexpr int LDS_BYTES = KTMAX * STAGE > RED ? KTMAX * STAGE : RED;
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
// slots per wave that fit the LDS, from the stage bytes: the most SPW with 4 SPW stages within 160 KiB
constexpr int os_w4a16_smax(int TM) { return 160 * 1024 / (4 * (TM * 256 + 32 * 64 + 256)); }
static_assert(os_w4a16_smax(32) == 3 && os_w4a16_smax(64) == 2, "the one-shot ladders of launch_grouped_w4a16_os");

// RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at most 4 SPW stages, every stage has a slot of its own)
// GATHER: A rows through p.src_row
template <class C, bool RING = false, bool GATHER = false>
__global__ __launch_bounds__(256) void gemm_mx_os_w4a16_kernel(const W4A16Params p) {
  constexpr int SPW = C::SPW, LPS = C::LPS, MT = C::MT;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass does not resolve the unconditional device-side tile decode; it only needs the kernel's symbol -- as gemm_mx_grouped_ring_kernel)
  GroupedView gv{};
  if (!grouped_setup<C::TM, C::TN, 16>(p, gv)) return;   // an m-tile slot past the real tiles: no work (16: the A side's element width -- a_bytes = rows x 2 K)
  asm volatile("" :: "s"(p.A), "s"(p.D), "s"(p.K), "s"(p.b_bytes), "s"(p.alpha));   // all scalar argument loads in one round
  const float alpha = *gv.alpha;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), i32 = lane & 31, g = lane >> 5;
  const int m0 = gv.m0, n0 = gv.n0;
  const int rowA = p.K << 1, rowB = p.K >> 1, KT = p.K >> 7, KB = p.K >> 5;   // bytes per A / B row, stages, scale bytes per row

  // ---- LDS-DMA sources --------------------------------------------------------------------------------------------------------------
  const uint32_t a_off = GATHER ? 0u : (uint32_t)m0 * rowA, b_off = (uint32_t)n0 * rowB;
  const __amdgpu_buffer_rsrc_t rA = GATHER ? make_rsrc(p.A, (uint32_t)p.T * rowA) : make_rsrc(p.A + a_off, gv.a_bytes - a_off);
  const __amdgpu_buffer_rsrc_t rB = make_rsrc(gv.B + b_off, p.b_bytes - b_off);
  // A piece qq = rows 4 qq .. + 3; lane -> row 4 qq + (l >> 4), physical chunk l & 15 = logical chunk ^ (row & 15) = logical chunk ^ (4 (qq & 3) | (l >> 4))
  const int cA = ((lane & 15) ^ (lane >> 4)) << 4;
  int vRA[C::NPA];   // the row part of every piece's offset; GATHER: bit 31 (past every descriptor) for a row past the group's end or an index outside [0, T)
  if constexpr (GATHER) {
    int idx[C::NPA];
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {   // unconditional, in-bounds loads: one round trip, before the K walk
      const int r = m0 + 4 * qq + (lane >> 4);
      idx[qq] = p.src_row[r < gv.M ? r : m0];
    }
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {
      const int r = m0 + 4 * qq + (lane >> 4);
      const bool ok = r < gv.M && (unsigned)idx[qq] < (unsigned)p.T;
      vRA[qq] = ok ? idx[qq] * rowA : (int)0x80000000;
    }
  } else {
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) vRA[qq] = (4 * qq + (lane >> 4)) * rowA;
  }
  // B piece qq = rows 16 qq .. + 15; lane -> row 16 qq + (l >> 2), physical chunk l & 3 = logical chunk ^ ((row >> 2) & 3)
  const int vPB = (lane >> 2) * rowB + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
  const int stepB = 16 * rowB;
  // scale dwords: bytes 4 kt .. + 3 of the row's K / 32; both lane halves fetch the row's dword; rows past N lie past the descriptor
  const uint32_t sb_off = (uint32_t)n0 * KB;
  const __amdgpu_buffer_rsrc_t rSB = make_rsrc(gv.SFB + sb_off, p.sfb_bytes - sb_off);
  const int vSB = i32 * KB;

  auto issue = [&](const int kt, const int slot) __attribute__((always_inline)) {   // stage kt into slot `slot` of this wave (kt >= KT: every piece out of range -> zeros)
    char* st = smem + (wave * SPW + slot) * C::STAGE;
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {
      const int v = ((vRA[qq] + (cA ^ (64 * (qq & 3)))) & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)(st + qq * 1024), 16, v, kt * C::ROWA, 0, 0);
    }
#pragma unroll
    for (int qq = 0; qq < C::NPB; ++qq) {
      const int v = ((vPB + qq * stepB) & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr_t)(st + C::OFF_B + qq * 1024), 16, v, kt * C::ROWB, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSB, (lds_ptr_t)(st + C::OFF_SB), 4, (vSB & ~oob) | ((int)0x80000000 & oob), kt * 4, 0, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
#pragma unroll
  for (int j = 0; j < SPW; ++j) issue(wave + 4 * j, j);

  const int swA = i32 & 15, swB = (i32 >> 2) & 3;
  v16f acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };

  // one stage out of slot u; RING: kt_next (>= KT: zeros) is requested into the slot as soon as the reads have returned
  auto consume = [&](const int u, const int kt_next) __attribute__((always_inline)) {
    const char* st = smem + (wave * SPW + u) * C::STAGE;
    v4i fa[MT][8], fb[2];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {   // c8 = 4 js + d: A chunk 4 (2 js + g) + d (elements 8 d .. + 7 of K-block 2 js + g)
      const int chunk = 4 * (2 * (c8 >> 2) + g) + (c8 & 3);
      const int off = i32 * C::ROWA + ((chunk ^ swA) << 4);
#pragma unroll
      for (int t = 0; t < MT; ++t) fa[t][c8] = *(const v4i*)(st + t * 32 * C::ROWA + off);
    }
#pragma unroll
    for (int js = 0; js < 2; ++js) fb[js] = *(const v4i*)(st + C::OFF_B + i32 * C::ROWB + (((2 * js + g) ^ swB) << 4));   // B chunk = K-block 2 js + g
    int sb = *(const int*)(st + C::OFF_SB + lane * 4);
    fence();   // every read issued before the first convert
    if constexpr (RING) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0]), "+v"(fa[0][1]), "+v"(fa[0][2]), "+v"(fa[0][3]), "+v"(fa[0][4]), "+v"(fa[0][5]), "+v"(fa[0][6]), "+v"(fa[0][7]),
                   "+v"(fb[0]), "+v"(fb[1]), "+v"(sb) :: "memory");   // the slot is free
      if constexpr (MT == 2)
        asm volatile("" : "+v"(fa[1][0]), "+v"(fa[1][1]), "+v"(fa[1][2]), "+v"(fa[1][3]), "+v"(fa[1][4]), "+v"(fa[1][5]), "+v"(fa[1][6]), "+v"(fa[1][7]) :: "memory");
      issue(kt_next, u);
      fence();
    }
    const unsigned sbs = (unsigned)sb >> (8 * g);   // "my" scale byte of K-block 2 js + g at byte 2 js
#pragma unroll
    for (int js = 0; js < 2; ++js) {
      const unsigned byte = (sbs >> (16 * js)) & 0xffu;
      const float scale = __builtin_bit_cast(float, byte << 23);   // 2^(byte - 127) for bytes 1 ... 254
      const int nan = byte == 0xffu ? 0x7fc0 : 0;                  // byte 255: one NaN element poisons the weight row's sums
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const unsigned u8 = (unsigned)fb[js][d];
        const bf16x2_t w0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 0), w1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 1);
        const bf16x2_t w2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 2), w3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u8, scale, 3);
        v4i wi = {__builtin_bit_cast(int, w0), __builtin_bit_cast(int, w1), __builtin_bit_cast(int, w2), __builtin_bit_cast(int, w3)};
        if (d == 0) wi[0] |= nan;
        const v8bf B8 = __builtin_bit_cast(v8bf, wi);
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8, __builtin_bit_cast(v8bf, fa[t][4 * js + d]), acc[t], 0, 0, 0);
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
  __builtin_amdgcn_s_barrier();   // every wave's reads of the stage areas are done: they become the sum's scratch
  fence();

  // ---- cross-wave sum: [wave][row][8 chunks of 4 fp32], chunk ^ (row & 7); ((w0 + w1) + w2) + w3, one multiply by alpha, one rounding to bf16 ----------------
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *(v4f*)(smem + (wave * C::TM + 32 * t + i32) * 128 + (((2 * q + g) ^ (i32 & 7)) << 4)) = v4f{acc[t][4 * q + 0], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
  __syncthreads();
  const int cq = tid & 7;   // chunk of 4 columns
#pragma unroll
  for (int h = 0; h < MT; ++h) {
    const int rr = (tid >> 3) + 32 * h;   // row of the tile
    v4f s[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w] = *(const v4f*)(smem + (w * C::TM + rr) * 128 + ((cq ^ (rr & 7)) << 4));
    v4f t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = ((s[0][e] + s[1][e]) + s[2][e]) + s[3][e];
    const int row = m0 + rr, col = n0 + 4 * cq;
    if (row < gv.M && col < p.N && 4 * cq < C::TN) {
      v2i o;
      o[0] = (int)pack_bf16x2(t[0] * alpha, t[1] * alpha);
      o[1] = (int)pack_bf16x2(t[2] * alpha, t[3] * alpha);
      *(v2i*)(p.D + (size_t)row * p.ldd + col) = o;
    }
  }
#endif
}

}  // namespace qamd
