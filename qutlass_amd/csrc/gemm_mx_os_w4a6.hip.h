// Grouped W4A6 GEMM for gfx950 (extension: grouped_matmul_mxf6_mxf4_bf16_tn): MXFP6 tokens (e2m3, as fusedQuantizeMxf6 / fusedGatherQuantizeMxf6 write them: element k of
// a row in bits 6 k .. 6 k + 5 of the row read as one little-endian bit string, 3 K / 4 bytes per row) against MXFP4 stacked expert weights (e2m1, as fusedQuantizeMx
// writes them and grouped_matmul_mxf4_bf16_tn reads them), row-major e8m0 scales on both sides.
//
// gemm_mx_os_w4a8.hip.h with a 6-bit A side -- a kernel of its own, so that every kernel of that header keeps its code and its name.
// v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = 4 (srcA, the B fragment, is e2m1) and blgp = 2 (srcB, the A fragment, is e2m3): 8 passes, the FP4 rate, against 16 as soon
// as one operand is 8 bits wide.  A stage is 128 K elements:
//   A rows are 96 bytes per stage -- six 16-byte chunks -- at a row pitch of 3 K / 4 bytes in memory and 96 bytes in the LDS.  The LDS-DMA writes 64 lanes x 16 bytes to
//     a linear 1 KiB destination from per-lane sources: a 32-row A tile is THREE pieces, lane l of piece qq holds physical chunk P = 64 qq + l = 6 row + c'.
//     The A fragment of lane (i32, g) for the MFMA js is the 24 bytes of K-block b = 2 js + g: bytes 24 b .. + 23 of the row's 96, six dwords, registers 6 and 7 zero.
//     24-byte runs start at 8-byte, not 16-byte boundaries (blocks 1 and 3), so they are read as three ds_read_b64 -- 8-byte units u = 3 b .. 3 b + 2, unit u = half
//     u & 1 of chunk u >> 1 -- and an 8-byte unit never straddles a chunk, so the chunks of a row may be permuted.
//     Banks: ds_read_b64 is served per 32-lane half (all lanes of a half read the same unit u of rows 0 .. 31), the bank row is 256 B = 16 chunk slots.  Linear, row r's
//     chunk c sits in slot (6 r + c) mod 16, and 6 r mod 16 takes 8 values (the even ones), each for the four rows r, r + 8, r + 16, r + 24: a 4-way conflict.  With
//     16-byte DMA granules and one unit per instruction the 32 lanes can reach 16 of the bank row's 32 8-byte positions (those of half u & 1), so 2-way is the floor.
//     The swizzle c' = (c + ((r >> 3) & 1)) mod 6, a rotation of the row's chunks for rows 8-15 and 24-31, reaches it: rows r and r + 16 keep slot 6 r + c, rows r + 8
//     and r + 24 move to 6 r + (c + 1) mod 6, which has the other parity -- every slot is read by exactly two lanes.  A ds_read_b64 then takes 4 LDS cycles instead of 2;
//     the six of a stage and m-tile cost 24 cycles beside the 64 of its two MFMAs (the W4A8 kernel's four ds_read_b128: 16).
//   B rows, their pieces and swizzle, the scale dwords and the B fragment are exactly the W4A8 kernel's; both scale bytes are those of K-block 2 js + g.
// The stage is (TM x 96 + 32 x 64) B + 512 B of scale dwords: 5.5 KiB for a 32-row tile (W4A8: 6.5), 8.5 KiB for a 64-row tile (10.5).
// One shot while 4 SPW stages hold the tile's K extent, wave-owned rings of SPW slots beyond (gemm_mx_os.hip.h); K % 128 == 0, so no stage has a short tail.
#pragma once
#include "gemm_mx.hip.h"
#include "gemm_mx_grouped.hip.h"

namespace qamd {

template <int SPW_, int TN_ = 32, int TM_ = 32>   // SPW: K stages per wave -- the kernel covers 4 SPW stages of 128 elements (RING: any K)
struct OsW4A6Cfg {
  static constexpr int TM = TM_, TN = TN_, ROWA = 96, ROWB = 64, SPW = SPW_, KTMAX = 4 * SPW_;
  static constexpr int MT = TM / 32;                                                        // m-tiles of 32 rows
  static constexpr int OFF_B = TM * ROWA, OFF_S = OFF_B + 32 * ROWB, OFF_SB = OFF_S + 256, STAGE = OFF_SB + 256;   // (the B area keeps 32 rows: the fragment reads span them)
  static constexpr int NPA = TM * 6 / 64, NPB = TN / 16;                                    // A / B pieces per stage
  static constexpr int LPS = NPA + NPB + 2;                                                 // LDS-DMA instructions per stage
  static_assert(TN == 32 || TN == 16, "tile width");
  static_assert(TM == 32 || TM == 64, "tile height");
  static constexpr int RED = 4 * TM * 128;                                                  // cross-wave sum: [wave] TM x 32 fp32
  static constexpr int LDS_BYTES = KTMAX * STAGE > RED ? KTMAX * STAGE : RED;
  static_assert(SPW >= 1 && SPW * LPS <= 63, "vmcnt immediate");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
// slots per wave that fit the LDS: a 32-row tile's stage is 5.5 KiB (28 of them = 154 KiB), a 64-row tile's 8.5 KiB (16 = 136 KiB)
constexpr int os_w4a6_smax(int TM) { return TM == 32 ? 7 : 4; }

// RING: any K -- the wave's SPW slots are refilled as they are consumed (false: at most 4 SPW stages, every stage has a slot of its own)
template <class C, bool RING = false>
__global__ __launch_bounds__(256) void gemm_mx_os_w4a6_kernel(const GroupedParams p) {
  constexpr int SPW = C::SPW, LPS = C::LPS, MT = C::MT;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass does not resolve the unconditional device-side tile decode; it only needs the kernel's symbol -- as gemm_mx_grouped_ring_kernel)
  GroupedView gv{};
  if (!grouped_setup<C::TM, C::TN, 6>(p, gv)) return;   // an m-tile slot past the real tiles: no work (6: the A side's element width -- a_bytes = rows x 3 K / 4)
  asm volatile("" :: "s"(p.A), "s"(p.D), "s"(p.K), "s"(p.b_bytes), "s"(p.alpha));   // all scalar argument loads in one round
  const float alpha = *gv.alpha;
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), i32 = lane & 31, g = lane >> 5;
  const int m0 = gv.m0, n0 = gv.n0;
  const int rowA = (p.K >> 2) * 3, rowB = p.K >> 1, KT = p.K >> 7, KB = p.K >> 5;   // bytes per A / B row, stages, scale bytes per row

  // ---- LDS-DMA sources --------------------------------------------------------------------------------------------------------------
  const uint32_t a_off = (uint32_t)m0 * rowA, b_off = (uint32_t)n0 * rowB;
  const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A + a_off, gv.a_bytes - a_off), rB = make_rsrc(gv.B + b_off, p.b_bytes - b_off);
  // A piece qq: lane -> physical chunk P = 64 qq + l of the tile = row P / 6, physical chunk c' = P % 6 = (logical chunk + ((row >> 3) & 1)) mod 6
  int vPA[C::NPA];
#pragma unroll
  for (int qq = 0; qq < C::NPA; ++qq) {
    const int P = 64 * qq + lane, r = P / 6, cp = P - 6 * r;
    int c = cp - ((r >> 3) & 1);
    c += c < 0 ? 6 : 0;
    vPA[qq] = r * rowA + (c << 4);
  }
  // B piece qq = rows 16 qq .. + 15; lane -> row 16 qq + (l >> 2), physical chunk l & 3 = logical chunk ^ ((row >> 2) & 3)
  const int vPB = (lane >> 2) * rowB + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
  const int stepB = 16 * rowB;
  // scale dwords: bytes 4 kt .. + 3 of the row's K / 32; both lane halves fetch the row's dword (TM = 64: lane half g fetches m-tile g's); rows past the group's end / past N
  // lie past the descriptor
  const uint32_t sa_off = (uint32_t)m0 * KB, sb_off = (uint32_t)n0 * KB;
  const __amdgpu_buffer_rsrc_t rSA = make_rsrc(p.SFA + sa_off, gv.sfa_bytes - sa_off), rSB = make_rsrc(gv.SFB + sb_off, p.sfb_bytes - sb_off);
  const int vSA = (32 * (MT == 2 ? g : 0) + i32) * KB, vSB = i32 * KB;

  auto issue = [&](const int kt, const int slot) __attribute__((always_inline)) {   // stage kt into slot `slot` of this wave (kt >= KT: every piece out of range -> zeros)
    char* st = smem + (wave * SPW + slot) * C::STAGE;
    int oob = (kt < KT) ? 0 : -1;
    asm volatile("" : "+v"(oob));
#pragma unroll
    for (int qq = 0; qq < C::NPA; ++qq) {
      const int v = (vPA[qq] & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)(st + qq * 1024), 16, v, kt * C::ROWA, 0, 0);
    }
#pragma unroll
    for (int qq = 0; qq < C::NPB; ++qq) {
      const int v = ((vPB + qq * stepB) & ~oob) | ((int)0x80000000 & oob);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_ptr_t)(st + C::OFF_B + qq * 1024), 16, v, kt * C::ROWB, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSA, (lds_ptr_t)(st + C::OFF_S), 4, (vSA & ~oob) | ((int)0x80000000 & oob), kt * 4, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rSB, (lds_ptr_t)(st + C::OFF_SB), 4, (vSB & ~oob) | ((int)0x80000000 & oob), kt * 4, 0, 0);
  };

  // ---- everything this wave will ever read (RING: its first SPW stages), requested now ---------------------------------------------------------
#pragma unroll
  for (int j = 0; j < SPW; ++j) issue(wave + 4 * j, j);

  // A fragment reads: unit u = 3 (2 js + g) + j of the row -> byte ((u >> 1) + swA) mod 6 * 16 + (u & 1) * 8 of its 96
  const int swA = (i32 >> 3) & 1, swB = (i32 >> 2) & 3;
  int offA[2][3];
#pragma unroll
  for (int js = 0; js < 2; ++js)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int u = 3 * (2 * js + g) + j;
      int c = (u >> 1) + swA;
      c -= c >= 6 ? 6 : 0;
      offA[js][j] = i32 * C::ROWA + (c << 4) + ((u & 1) << 3);
    }
  v16f acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };

  // one stage out of slot u; RING: kt_next (>= KT: zeros) is requested into the slot as soon as the reads have returned
  auto consume = [&](const int u, const int kt_next) __attribute__((always_inline)) {
    const char* st = smem + (wave * SPW + u) * C::STAGE;
    v2i fa[MT][2][3];
    v4i fb[2];
#pragma unroll
    for (int js = 0; js < 2; ++js)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t) fa[t][js][j] = *(const v2i*)(st + t * 32 * C::ROWA + offA[js][j]);
#pragma unroll
    for (int js = 0; js < 2; ++js) fb[js] = *(const v4i*)(st + C::OFF_B + i32 * C::ROWB + (((2 * js + g) ^ swB) << 4));   // B chunk = K-block 2 js + g
    int sa[MT], sb;
#pragma unroll
    for (int t = 0; t < MT; ++t) sa[t] = *(const int*)(st + C::OFF_S + (MT == 2 ? (32 * t + i32) * 4 : lane * 4));
    sb = *(const int*)(st + C::OFF_SB + lane * 4);
    fence();   // every read issued before the first MFMA
    if constexpr (RING) {
      if constexpr (MT == 1)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0][0]), "+v"(fa[0][0][1]), "+v"(fa[0][0][2]), "+v"(fa[0][1][0]), "+v"(fa[0][1][1]), "+v"(fa[0][1][2]),
                     "+v"(fb[0]), "+v"(fb[1]), "+v"(sa[0]), "+v"(sb) :: "memory");   // the slot is free
      else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[0][0][0]), "+v"(fa[0][0][1]), "+v"(fa[0][0][2]), "+v"(fa[0][1][0]), "+v"(fa[0][1][1]), "+v"(fa[0][1][2]),
                     "+v"(fa[MT - 1][0][0]), "+v"(fa[MT - 1][0][1]), "+v"(fa[MT - 1][0][2]), "+v"(fa[MT - 1][1][0]), "+v"(fa[MT - 1][1][1]), "+v"(fa[MT - 1][1][2]),
                     "+v"(fb[0]), "+v"(fb[1]), "+v"(sa[0]), "+v"(sa[MT - 1]), "+v"(sb) :: "memory");
      issue(kt_next, u);
      fence();
    }
    // "my" scale byte of K-block 2 js + g down to byte 2 js: op_sel 2 js picks it
#pragma unroll
    for (int t = 0; t < MT; ++t) sa[t] = (int)((unsigned)sa[t] >> (8 * g));
    sb = (int)((unsigned)sb >> (8 * g));
    // cbsz = format of srcA (the B fragment): 4 = e2m1; blgp = format of srcB (the A fragment): 2 = e2m3, six dwords
#pragma unroll
    for (int js = 0; js < 2; ++js) {
      const v8i B8 = {fb[js][0], fb[js][1], fb[js][2], fb[js][3], 0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const v8i A8 = {fa[t][js][0][0], fa[t][js][0][1], fa[t][js][1][0], fa[t][js][1][1], fa[t][js][2][0], fa[t][js][2][1], 0, 0};
        if (js == 0) acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B8, A8, acc[t], 4, 2, 0, sb, 0, sa[t]);
        if (js == 1) acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B8, A8, acc[t], 4, 2, 2, sb, 2, sa[t]);
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
