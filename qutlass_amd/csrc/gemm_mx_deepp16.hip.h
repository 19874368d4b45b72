// The one-tile form of the persistent MXFP4 256x256 kernel (gemm_mx_deepp.hip.h, ONETILE, even stage count) on v_mfma_scale_f32_16x16x128_f8f6f4.
//
// Why: the launch sits at the socket power cap, two thirds of its joules are MFMAs, and on quantised-Gaussian codes the 16x16x128 shape delivers 10 - 12 % more
// FLOP/s than the 32x32x64 shape at equal cycles per flop -- 5 - 7 % with a K stage's fragment reads, LDS-DMA, scale reads and shifts in the loop
// (tests/native/energy_ubench16.hip, profiles/energy_ubench16_r8a.txt).
//
// Unchanged against gemm_mx_deepp<..., ONETILE>: the tile walk and XCD remap, the LDS-DMA pieces / descriptors / zero fill (GemmCtx), the LDS image (two stages of
// 72 KiB, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7) -- conflict-free for the 16-row access too: the 16 lanes of a ds_read_b128 group still meet 16
// different 16-byte slots), one hand-off per stage, write-through whole-line stores with rows >= M and columns >= N falling off the descriptor, 256 accumulator
// registers.
// What differs:
//   * a wave's 128x128 tile is 8 x 8 tiles of 16x16 (v4f each).  A stage (K = 256) is two halves of K = 128; in half h lane (r = l & 15, kq = l >> 4) takes the
//     16-byte chunk 4 h + kq of row 16 t + r: K-blocks 4 h .. 4 h + 3 = column tile h of the to_blocked scale image, whose dword for the row is exactly the MFMA's
//     four K-blocks.  The lane's scale byte is byte kq: the dword shifted right by 8 kq, op_sel 0 (as the decode kernels, gemm_mx_os.hip.h).
//   * scale dwords: rows 16 t + r = 32 (t >> 1) + 16 (t & 1) + r, so the 16-byte line of row 16 p + r holds the dwords of t = p, p + 2, p + 4, p + 6:
//     two ds_read_b128 per operand and half, then 16 shifts.
//   * per stage: half 0 runs on register set 0 while set 1 (half 1 of the same buffer) is read; hand-off; half 1 runs while the stage's 17 DMA items are issued
//     and set 0 is read from the other buffer.  One fragment read behind every second MFMA, never more than two single-issue instructions behind one MFMA
//     (an MFMA of 16 cycles holds the vector issue for 8 of them).  What exactly rides between the MFMAs is the K loop's form KL, below: the product issues the
//     pieces of every stage that fetches neither the K tail nor past the end as one statement each (M0 write, MFMA, load), spread over the whole of half 1.
//   * last stage: half 0 as ever, then half 1 in (m, n) order: the 8 tiles of tile row m (16 rows x 128 columns of fp32 = the wave's 8-KiB scratch slice of
//     buffer 1) are final after MFMA 8 m + 7 and retire in the shadows of the next rows' MFMAs: 8 ds_write_b128 (chunk 4 n + kq of row r at
//     (c & ~7) | ((c & 7) ^ (r & 7)): the 8 lanes of a write group meet 8 different slots), read back row-major (lane -> row l / 8, columns 8 (l % 8) .. + 7 of a
//     64-column half: the 16 lanes of a read group meet 16 different slots), alpha, bf16, one 16-byte store: 8 rows x 128 B per store instruction.
// The products and their partial sums are exact in fp32 on quantised data under the spread condition of docs/history.md section 3.1, so grouping K by 128 instead
// of 64 changes no bit there; with adversarial exponent spreads the usual tolerance applies.
#pragma once
#include "gemm_mx_deepp.hip.h"

namespace qamd {

// Which one-tile form the product launches (capi.hip launch_gemm_deepp); the lab library reaches both ("gemm_variant" 190 / 191, and 192 ... 197: 191 with the K loop's form forced).
constexpr bool kDeeppOneTile16 = true;

// post-hand-off MFMA index of the last stage at which tile ROW m (8 tiles) is final: e(m) = 8 m + 7; inverse (-1: none)
constexpr int deepp16_row_done_at(int s) { return (s >= 7 && s <= 63 && (s - 7) % 8 == 0) ? (s - 7) / 8 : -1; }

// ---- the K loop's form (template parameter KL of the kernel): what rides between the MFMAs of a stage ---------------------------------------------------------
//   KL_SCALES  K-blocks interleaved across the stage's two MFMAs per accumulator instead of split into halves: MFMA s gives lane group kq the block
//              4 (kq >> 1) + 2 (kq & 1) + s, so the lane's two scale bytes of a stage are the 16 bits at byte 2 (kq & 1) of its row's dword in column tile kq >> 1:
//              one ds_read_u16 per row tile, operand and STAGE, the register serves MFMA 0 with byte select 0 and MFMA 1 with byte select 1 -- no shift, no wait in
//              front of one.  The registers are kept per LDS buffer (the next stage's are read behind half 1 while half 1 still multiplies by this stage's).
//   KL_DMA     the stages that fetch neither the K tail nor past the end (kt < KT - 1) issue their 17 pieces from loop-invariant lane offsets (q * rstep folded in
//              once) and descriptor words, each piece in ONE statement with its MFMA -- s_mov m0 / MFMA / buffer_load ... lds: the MFMA is the wait state between
//              the M0 write and the load, so no s_nop, no v_add, no mask arithmetic.  The stages that fetch the tail keep the masked path.
//   KL_SPREAD  (with KL_DMA) the 17 pieces behind MFMAs 0, 2, 6, 10 ... 62 of half 1 instead of 0, 2, 4 ... 32
// 0 is the loop as it was before these existed (lab "gemm_variant" 192; 193 ... 197 force the other combinations); the product's is kDeepp16KLoop.
// Measured at 4096^3 (docs/history.md section 13, profiles/ab_deepp16_kloop.txt): what gains is WHERE the pieces are issued -- KL_DMA | KL_SPREAD -4 ... -6 % against the
// loop of 0 on three boxes, KL_DMA alone and KL_SCALES alone nothing outside the run-to-run spread, KL_SCALES on top of the other two -0.1 ... -0.3 us, inside the spread.
// So the product spreads the lean pieces and keeps the scale handling (and with it every output bit outside the exact regime too) as it was.
enum { KL_SCALES = 1, KL_DMA = 2, KL_SPREAD = 4 };
constexpr int kDeepp16KLoop = KL_DMA | KL_SPREAD;

// K-block (= 16-byte chunk of the row's 128 stage bytes = byte of the stage's two scale dwords) that lane group kq feeds to MFMA s of a stage
constexpr int deepp16_kblock(bool interleaved, int s, int kq) { return interleaved ? 4 * (kq >> 1) + 2 * (kq & 1) + s : 4 * s + kq; }
constexpr bool deepp16_kblocks_once(bool interleaved) {
  unsigned seen = 0;
  for (int s = 0; s < 2; ++s)
    for (int kq = 0; kq < 4; ++kq) {
      const unsigned bit = 1u << deepp16_kblock(interleaved, s, kq);
      if (seen & bit) return false;
      seen |= bit;
    }
  return seen == 0xffu;
}
static_assert(deepp16_kblocks_once(false) && deepp16_kblocks_once(true), "every one of a stage's 8 K-blocks goes to exactly one (MFMA, lane group)");
// half-1 MFMA slot -> DMA item riding with it (-1: none)
constexpr int deepp16_item_at(bool spread, int i) {
  return spread ? (i == 0 ? 0 : (i % 4 == 2 ? (i + 2) / 4 : -1)) : ((i % 2 == 0 && i < 34) ? i / 2 : -1);
}

#if QAMD_DMA_AUX == 0
#define QAMD_DMA_AUX_ASM ""
#elif QAMD_DMA_AUX == 1
#define QAMD_DMA_AUX_ASM " sc0"
#elif QAMD_DMA_AUX == 2
#define QAMD_DMA_AUX_ASM " nt"
#elif QAMD_DMA_AUX == 16
#define QAMD_DMA_AUX_ASM " sc1"
#elif QAMD_DMA_AUX == 17
#define QAMD_DMA_AUX_ASM " sc0 sc1"
#else
#error "QAMD_DMA_AUX: spell the cache-policy bits for the LDS-DMA statement of gemm_mx_deepp16"
#endif
#define QAMD_MFMA16(SRC_C, OP_SEL) "v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, " SRC_C ", %3, %4 " OP_SEL "op_sel_hi:[0,0,0] cbsz:4 blgp:4"

template <class C, int ST_AUX = 0, int KL = kDeepp16KLoop>
__device__ __forceinline__ void gemm_mx_deepp16(char* smem, const GemmParams& p, const int bid, const int G, const int ntiles) {
  static_assert(C::EBITS == 4 && C::BM == 256 && C::BN == 256 && C::WAVES_M == 2 && C::WAVES_N == 2 && C::NSTAGE == 2 && C::PPW == 2,
                "persistent deep schedule: fp4, 256x256 tiles, 4 waves of 128x128");
  static_assert((KL & ~7) == 0 && (!(KL & KL_SPREAD) || (KL & KL_DMA)), "K-loop form");
  constexpr bool IL = (KL & KL_SCALES) != 0, LEAN = (KL & KL_DMA) != 0, SPREAD = (KL & KL_SPREAD) != 0;
  constexpr int MT = 8, NT = 8;
  constexpr int STAGE = C::STAGE_BYTES, OFF_SCR = DeepPCfg<C>::OFF_SCR;
  GemmCtx<C> cx(smem, p);   // per-lane DMA offsets; its tile coordinates, descriptors and read addresses are NOT used here
  const int lane = cx.lane, wave = cx.wave, r16 = lane & 15, kq = lane >> 4;
  const int KT = cx.KT, KTe = (KT + 1) & ~1, CB = cx.CB, rowbytes = cx.rowbytes;
  const int tile = xcd_remap(bid, G);   // one tile per workgroup: G == ntiles

  auto fence = [&]() __attribute__((always_inline)) { __builtin_amdgcn_sched_barrier(0); };
  struct Desc { __amdgpu_buffer_rsrc_t a, b, s; };
  int m0, n0;
  {
    int tm, tn;
    raster_decode(tile < ntiles ? tile : ntiles - 1, p.tiles_m, p.tiles_n, p.raster_magic, tm, tn);
    m0 = uniform(tm * C::BM);
    n0 = uniform(tn * C::BN);
  }
  Desc cur;
  {
    const bool valid = tile < ntiles;
    const uint32_t a_off = (uint32_t)m0 * rowbytes, b_off = (uint32_t)n0 * rowbytes;
    const uint32_t sa_off = (uint32_t)(m0 >> 7) * CB * 512, sb_off = (uint32_t)(n0 >> 7) * CB * 512;
    cur.a = make_rsrc(p.A + a_off, valid ? p.a_bytes - a_off : 0u);
    cur.b = make_rsrc(p.B + b_off, valid ? p.b_bytes - b_off : 0u);
    cur.s = cx.sIsB ? make_rsrc(p.SFB + sb_off, valid ? p.sfb_bytes - sb_off : 0u) : make_rsrc(p.SFA + sa_off, valid ? p.sfa_bytes - sa_off : 0u);
  }
  // KL_DMA: the same three descriptors as the words an asm statement takes in SGPRs (base, stride 0, bytes, raw-buffer flags as make_rsrc)
  v4u dwA, dwB, dwS;
  if constexpr (LEAN) {
    auto words = [&](const uint8_t* base, const uint32_t bytes) __attribute__((always_inline)) {
      const uint64_t u = (uint64_t)(uintptr_t)base;
      v4u d = {(uint32_t)u, (uint32_t)(u >> 32) & 0xffffu, bytes, 0x00020000u};
      return d;
    };
    const uint32_t a_off = (uint32_t)m0 * rowbytes, b_off = (uint32_t)n0 * rowbytes;
    const uint32_t sa_off = (uint32_t)(m0 >> 7) * CB * 512, sb_off = (uint32_t)(n0 >> 7) * CB * 512;
    dwA = words(p.A + a_off, p.a_bytes - a_off);
    dwB = words(p.B + b_off, p.b_bytes - b_off);
    dwS = cx.sIsB ? words(p.SFB + sb_off, p.sfb_bytes - sb_off) : words(p.SFA + sa_off, p.sfa_bytes - sa_off);
  }

  // ---- registers -------------------------------------------------------------------------------------------------------
  v4f acc[MT][NT];
  v4i fa[2][MT], fb[2][NT];   // set = half of the stage
  // scale operands of a half, in the registers their dwords were read into: xq[h][0 / 1] = A rows 16 p + r16 (p = 0, 1) -> row tiles t = p, p + 2, p + 4, p + 6,
  // xq[h][2 / 3] = the same of B; each dword is shifted right by 8 kq in place
  v4i xq[2][4];
  const int sh = 8 * kq;
  // KL_SCALES: xs[buf][t] / xs[buf][8 + t] = the two scale bytes (zero-extended 16 bits) of A / B row tile t for the stage in LDS buffer buf
  int xs[2][MT + NT];

  // LDS read addresses.  Fragments: row wave_row0 + 16 t + r16, chunk (4 h + kq) ^ ((r16 >> 1) & 7); B = the same + rdBd.
  const int sw = (r16 >> 1) & 7;
  int rdF[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) rdF[h] = (cx.wave_m * C::WTM + r16) * C::ROWB + ((deepp16_kblock(IL, h, kq) ^ sw) << 4);
  const int rdBd = cx.rdBd;
  // scale image of a stage: 512-byte pieces, A's (row tile wave_m, column tile h) at piece 2 wave_m + h, B's behind the PA pieces of A; row r of a piece at (r & 31) * 16 + (r >> 5) * 4
  const int rdSA = C::OFF_S + (cx.wave_m * C::SCT) * 512 + r16 * 16, rdSB = C::OFF_S + (C::PA + cx.wave_n * C::SCT) * 512 + r16 * 16;
  static_assert(C::SCT == 2 && C::WTM == 128 && C::WTN == 128, "a wave's rows are one 128-row scale tile; a stage is two column tiles");
  // KL_SCALES: the lane's 16 bits of row 16 t + r16 = 32 (t >> 1) + 16 (t & 1) + r16 lie at rdS2x + (t & 1) * 256 + (t >> 1) * 4
  const int rdS2A = rdSA + (kq >> 1) * 512 + 2 * (kq & 1), rdS2B = rdSB + (kq >> 1) * 512 + 2 * (kq & 1);

  typedef __attribute__((address_space(3))) const v4i* lds_v4i_t;
  uint32_t rbA = 0, rbB = 0;   // 32-bit LDS addresses of the half being read (made opaque once per half: folded into every read they exceed the 16-bit DS offset field)
  auto read_base = [&](const int buf, const int h) __attribute__((always_inline)) {
    rbA = (uint32_t)(uintptr_t)(lds_ptr_t)(smem + buf * STAGE + rdF[h]);
    rbB = rbA + (uint32_t)rdBd;
    asm volatile("" : "+v"(rbA), "+v"(rbB));
  };
  auto read_frag = [&](const int h, const int i) __attribute__((always_inline)) {   // i = 0..7: A row tiles, 8..15: B row tiles
    if (i < MT) fa[h][i] = *(lds_v4i_t)(uintptr_t)(rbA + (uint32_t)(i * 16 * C::ROWB));
    else fb[h][i - MT] = *(lds_v4i_t)(uintptr_t)(rbB + (uint32_t)((i - MT) * 16 * C::ROWB));
  };
  auto read_raw = [&](const int buf, const int h, const int k) __attribute__((always_inline)) {   // k = 0, 1: A p = 0, 1; 2, 3: B
    xq[h][k] = *(const v4i*)(smem + buf * STAGE + (k < 2 ? rdSA : rdSB) + h * 512 + (k & 1) * 256);
  };
  auto shift1 = [&](const int h, const int k) __attribute__((always_inline)) {   // k = 0..15: dword k % 4 of quad k / 4
    xq[h][k >> 2][k & 3] = (int)((unsigned)xq[h][k >> 2][k & 3] >> sh);
  };
  auto read_scale = [&](const int buf, const int k) __attribute__((always_inline)) {   // KL_SCALES; k = 0..7: A row tiles, 8..15: B row tiles
    const int t = k & 7;
    xs[buf][k] = *(const uint16_t*)(smem + buf * STAGE + (k < MT ? rdS2A : rdS2B) + (t & 1) * 256 + (t >> 1) * 4);
  };
  // one scaled FP4 MFMA: acc[m][n] (+)= B-fragment n x A-fragment m of half h.
  // Written as the instruction itself, accumulator TIED (vdst == srcC): through the builtin the register allocator gave most of the 64 four-register accumulators a
  // destination other than their source -- with all 256 accumulator registers taken that means copies through VGPRs and scratch around every MFMA (216
  // v_accvgpr_read + 212 v_accvgpr_write per two stages, 94 spilled registers; the fault of tests/native/ubench.hip mode 26).  An fp4 operand is four registers
  // (cbsz / blgp = 4), the scale operands are the lanes' byte 0 (op_sel 0).  What the compiler no longer sees: the matrix pipe's write of these registers --
  // the one reader other than an MFMA is the retirement's ds_write_b128, which waits for it explicitly (retire_write).
  // KL_SCALES: sbuf = the LDS buffer of the stage (whose xs registers apply); the second MFMA of the stage (h == 1) takes byte 1 of both scale registers.
  auto mfma1 = [&](const int h, const int m, const int n, const bool zero_c, const int sbuf) __attribute__((always_inline)) {
    const v4i a = fa[h][m], b = fb[h][n];
    const int sb1 = IL ? xs[sbuf][MT + n] : xq[h][2 + (n & 1)][n >> 1], sa1 = IL ? xs[sbuf][m] : xq[h][m & 1][m >> 1];
    if (zero_c)
      asm volatile(QAMD_MFMA16("0", "") : "=a"(acc[m][n]) : "v"(b), "v"(a), "v"(sb1), "v"(sa1));
    else if (IL && h == 1)
      asm volatile(QAMD_MFMA16("%0", "op_sel:[1,1,0] ") : "+a"(acc[m][n]) : "v"(b), "v"(a), "v"(sb1), "v"(sa1));
    else
      asm volatile(QAMD_MFMA16("%0", "") : "+a"(acc[m][n]) : "v"(b), "v"(a), "v"(sb1), "v"(sa1));
  };
  // KL_DMA: the same MFMA (never the first of an accumulator) with one LDS-DMA piece in its statement: M0 = the piece's LDS address before the MFMA, the load
  // behind it.  The compiler keeps M0 for itself and sets it in front of every use of its own, so nothing of it lives across the statement.
  auto mfma1_dma = [&](const int h, const int m, const int n, const int sbuf, const v4u d, const uint32_t lds, const int voff, const int soff)
                       __attribute__((always_inline)) {
    const v4i a = fa[h][m], b = fb[h][n];
    const int sb1 = IL ? xs[sbuf][MT + n] : xq[h][2 + (n & 1)][n >> 1], sa1 = IL ? xs[sbuf][m] : xq[h][m & 1][m >> 1];
    if (IL && h == 1)
      asm volatile("s_mov_b32 m0, %5\n\t" QAMD_MFMA16("%0", "op_sel:[1,1,0] ") "\n\tbuffer_load_dwordx4 %6, %7, %8 offen lds" QAMD_DMA_AUX_ASM
                   : "+a"(acc[m][n]) : "v"(b), "v"(a), "v"(sb1), "v"(sa1), "s"(lds), "v"(voff), "s"(d), "s"(soff) : "memory");
    else
      asm volatile("s_mov_b32 m0, %5\n\t" QAMD_MFMA16("%0", "") "\n\tbuffer_load_dwordx4 %6, %7, %8 offen lds" QAMD_DMA_AUX_ASM
                   : "+a"(acc[m][n]) : "v"(b), "v"(a), "v"(sb1), "v"(sa1), "s"(lds), "v"(voff), "s"(d), "s"(soff) : "memory");
  };

  // ---- LDS-DMA of one stage, one instruction at a time (item 0..7: A pieces, 8..15: B pieces, 16: the scale piece): as gemm_mx_deepp ------------------------
  int vb0 = 0, vb1 = 0, vbS = 0;
  auto dma_prep = [&](int kt, bool valid) __attribute__((always_inline)) {
    int lastmask = (kt == KT - 1) ? -1 : 0;
    int oobm = (valid && kt < KT) ? 0 : -1;
    int oobs = (valid && kt * C::SCT + cx.colS < CB) ? 0 : -1;
    asm volatile("" : "+v"(lastmask), "+v"(oobm), "+v"(oobs));
    vb0 = (((cx.voffT[0] & lastmask) | (cx.voffAB[0] & ~lastmask)) & ~oobm) | ((int)0x80000000 & oobm);
    vb1 = (((cx.voffT[1] & lastmask) | (cx.voffAB[1] & ~lastmask)) & ~oobm) | ((int)0x80000000 & oobm);
    vbS = (cx.voffS & ~oobs) | ((int)0x80000000 & oobs);
  };
  auto dma_item = [&](const Desc& d, int kt, const int buf, const int item) __attribute__((always_inline)) {
    char* st = smem + buf * STAGE;
    if (item < 16) {
      const int t = item & 7, q = wave * 8 + t;
      const int v = ((t & 1) ? vb1 : vb0) + q * cx.rstep;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(item < 8 ? d.a : d.b, (lds_ptr_t)(st + (item < 8 ? 0 : C::OFF_B) + q * 1024), 16, v, kt * C::ROWB, 0, QAMD_DMA_AUX);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(d.s, (lds_ptr_t)(st + C::OFF_S + wave * 1024), 16, vbS, kt * C::SCT * 512, 0, 0);
    }
  };
  // KL_DMA: lane offsets of the wave's 8 pieces per operand with the piece's row offset folded in (rows past M / N stay out of the descriptor's range through
  // them, as in dma_item), for stages kt < KT - 1 only: no K tail, both scale column tiles exist.  Opaque, so that they stay registers and are not recomputed.
  int vq[8], vqS = cx.voffS;
  if constexpr (LEAN) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      vq[t] = cx.voffAB[t & 1] + (wave * 8 + t) * cx.rstep;
      asm volatile("" : "+v"(vq[t]));
    }
    asm volatile("" : "+v"(vqS));
  }
  // the MFMA of half-1 slot i with the slot's piece, if it has one (then true)
  auto lean_slot = [&](const int i, const int m, const int n, int kt, const int buf) __attribute__((always_inline)) {
    const int item = deepp16_item_at(SPREAD, i);
    if (item < 0) return false;
    char* st = smem + buf * STAGE;
    if (item < 16) {
      const int t = item & 7, q = wave * 8 + t;
      mfma1_dma(1, m, n, buf, item < 8 ? dwA : dwB, (uint32_t)(uintptr_t)(lds_ptr_t)(st + (item < 8 ? 0 : C::OFF_B) + q * 1024), vq[t], kt * C::ROWB);
    } else {
      mfma1_dma(1, m, n, buf, dwS, (uint32_t)(uintptr_t)(lds_ptr_t)(st + C::OFF_S + wave * 1024), vqS, kt * C::SCT * 512);
    }
    return true;
  };
  auto dma_stage = [&](const Desc& d, int kt, bool valid, const int buf) __attribute__((always_inline)) {
    dma_prep(kt, valid);
#pragma unroll
    for (int i = 0; i < 17; ++i) dma_item(d, kt, buf, i);
  };

  // s_waitcnt vmcnt(0) lgkmcnt(0) in front of a hand-off.  KL != 0: as the instruction the compiler's own wait counting reads (simm16 0x0070: vmcnt 0, expcnt 7 = no
  // wait, lgkmcnt 0).  Inside an asm statement it is invisible to that counting, and with no shift left to consume a scale read behind the half's fragment reads the
  // compiler put eight waits of its own (lgkmcnt(7) .. (3), all satisfied already) in front of the first MFMAs of half 1.
  auto handoff_wait = [&]() __attribute__((always_inline)) {
    if constexpr (KL != 0) {
      fence();
      __builtin_amdgcn_s_waitcnt(0x0070);
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
  };
  // the 64 MFMAs of half h in (m, n) order, each followed by extra(i)
  // (sbuf: the stage's LDS buffer, mfma1; with: a slot's MFMA issued together with something else -- true if it did)
  auto half = [&](const int h, const bool zero_c, const int sbuf, auto extra, auto with) __attribute__((always_inline)) {
    int i = 0;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        if (!with(i, m, n)) mfma1(h, m, n, zero_c, sbuf);
        extra(i);
        fence();
        ++i;
      }
  };
  // what rides behind the MFMAs of a half while register set hs is filled from (buf, half hs): 16 fragment reads behind the odd MFMAs 1 .. 31, the 4 scale reads
  // behind 33 .. 39, the 16 shifts behind 46 .. 61.  KL_SCALES: no scale work for set 1; with set 0 (the next stage) its 16 scale reads behind the odd MFMAs
  // 33 .. 63, B's first (the next half 0 needs all of B's within its first 8 MFMAs, A's one per 8)
  auto fill = [&](const int buf, const int hs, const int i) __attribute__((always_inline)) {
    if (i < 32 && (i & 1)) read_frag(hs, i >> 1);
    if constexpr (IL) {
      if (hs == 0 && i >= 33 && (i & 1)) read_scale(buf, (((i - 33) >> 1) + NT) & 15);
    } else {
      if (i >= 33 && i < 40 && (i & 1)) read_raw(buf, hs, (i - 33) >> 1);
      if (i >= 46 && i < 62) shift1(hs, i - 46);
    }
  };
  auto alone = [&](const int, const int, const int) __attribute__((always_inline)) { return false; };

  // ---- one K stage (not the last).  Entry: register set 0 holds half 0 of this stage; exit: the same for the next stage (other buffer).
  //      The DMA threaded through half 1 is stage ktl (into this stage's buffer, free after the hand-off).
  auto stage = [&](auto bufc, auto firstc, int ktl, bool dvalid, auto dmac) __attribute__((always_inline)) {
    constexpr int BUF = decltype(bufc)::value;
    constexpr bool FIRST = decltype(firstc)::value;
    constexpr int DMA = decltype(dmac)::value;   // 0: none, 1: the masked path (any stage), 2: KL_DMA (ktl < KT - 1)
    read_base(BUF, 1);
    half(0, FIRST, BUF, [&](const int i) __attribute__((always_inline)) {
      fill(BUF, 1, i);
      if (DMA == 1 && i == 42) dma_prep(ktl, dvalid);
      if (i == 63) read_base(BUF ^ 1, 0);
    }, alone);
    handoff_wait();   // own DMA of the next stage landed; own reads of this buffer done
    __builtin_amdgcn_s_barrier();
    fence();
    half(1, false, BUF, [&](const int i) __attribute__((always_inline)) {
      fill(BUF ^ 1, 0, i);
      if (DMA == 1 && !(i & 1) && i < 34) dma_item(cur, ktl, BUF, i >> 1);   // 17 items behind the even MFMAs 0 .. 32
    }, [&](const int i, const int m, const int n) __attribute__((always_inline)) {
      if constexpr (DMA == 2) return lean_slot(i, m, n, ktl, BUF);
      else return false;
    });
  };

  // ---- epilogue pieces: tile row m (16 rows x 128 columns) through the wave's scratch (fp32, 16 rows x 512 B), read back row-major -------------------------
  char* scr = smem + OFF_SCR + wave * DeepPCfg<C>::SCR_PER_WAVE;
  const int scrW = r16 * 512 + ((kq ^ (r16 & 7)) << 4);                            // chunk 4 n + kq: + 128 (n >> 1), ^ 64 for odd n
  const int rrl = lane >> 3, ccl = lane & 7;                                       // read-back: row rrl (+ 8), columns 8 ccl .. + 7 (+ 64)
  const int scrR = rrl * 512 + (ccl >> 2) * 128 + ((((2 * ccl) & 7) ^ rrl) << 4);   // chunk 2 ccl of that row; chunk 2 ccl + 1 = this ^ 16
  const float alpha = *p.alpha;
  __amdgpu_buffer_rsrc_t rD;
  int stLane, colLim;
  {
    const int64_t left = ((int64_t)(p.M - m0) * p.ldd - n0) * 2;
    rD = make_rsrc(p.D + ((int64_t)m0 * p.ldd + n0), (uint32_t)(left > 0x7fffffffll ? 0x7fffffffll : left));
    stLane = ((cx.wave_m * C::WTM + rrl) * p.ldd + cx.wave_n * C::WTN + 8 * ccl) * 2;
    colLim = p.N - n0 - cx.wave_n * C::WTN - 8 * ccl;   // column 64 ch + 8 ccl of the wave tile exists iff 64 ch < colLim
  }
  auto retire_write = [&](const int m) __attribute__((always_inline)) {
    // the row's last MFMA (16 cycles, issued one MFMA ago) has written its accumulator before the LDS store reads it: 16 wait states on top of the MFMA in between
    asm volatile("s_nop 15" ::: "memory");
#pragma unroll
    for (int n = 0; n < NT; ++n) *(v4f*)(scr + (scrW ^ ((n & 1) << 6)) + (n >> 1) * 128) = acc[m][n];
  };
  v4f rb[2][2];
  auto retire_read = [&](const int rh) __attribute__((always_inline)) {   // rows 8 rh .. + 7: passes 2 rh (columns 0 - 63), 2 rh + 1 (columns 64 - 127)
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      rb[ch][0] = *(const v4f*)(scr + scrR + rh * 4096 + ch * 256);
      rb[ch][1] = *(const v4f*)(scr + (scrR ^ 16) + rh * 4096 + ch * 256);
    }
  };
  // (a VALU write of a store's data registers must not sit DIRECTLY behind the store: tools/store_data_hazard.py scans the ISA for it)
  auto retire_store = [&](const int m, const int pass) __attribute__((always_inline)) {
    const int rh = pass >> 1, ch = pass & 1;
    const v4f lo = rb[ch][0], hi = rb[ch][1];
    v4i o;
    o[0] = (int)pack_bf16x2(lo[0] * alpha, lo[1] * alpha);
    o[1] = (int)pack_bf16x2(lo[2] * alpha, lo[3] * alpha);
    o[2] = (int)pack_bf16x2(hi[0] * alpha, hi[1] * alpha);
    o[3] = (int)pack_bf16x2(hi[2] * alpha, hi[3] * alpha);
    int ldd2 = p.ldd * 2;
    asm volatile("" : "+s"(ldd2));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, o), rD, (64 * ch < colLim) ? stLane : (int)0x80000000, (16 * m + 8 * rh) * ldd2 + 128 * ch, ST_AUX);
  };

  // ---- the LAST stage (buffer 1): half 0 as in every stage; hand-off (every wave has read what it needs of buffer 1: the A area becomes scratch); half 1 in
  //      (m, n) order with tile row m retiring behind the MFMAs that follow MFMA e = 8 m + 7:
  //        write e+1 | read rows 0-7 e+3 | stores e+5, e+6 | read rows 8-15 e+7 | stores e+9, e+10
  //      One scratch and one read-back register set per wave: write(m + 1) at e + 9 follows read(m) at e + 7, read(m + 1) at e + 11 follows the last store of m
  //      at e + 10 (within a slot: stores, then write, then read).
  auto final_stage = [&]() __attribute__((always_inline)) {
    read_base(1, 1);
    half(0, false, 1, [&](const int i) __attribute__((always_inline)) { fill(1, 1, i); }, alone);
    handoff_wait();
    __builtin_amdgcn_s_barrier();
    fence();
    static_for<0, 75>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value;
      if constexpr (s < 64) mfma1(1, s / 8, s % 8, false, 1);
      constexpr int d1 = s - 1, d3 = s - 3, d5 = s - 5, d6 = s - 6, d7 = s - 7, d9 = s - 9, d10 = s - 10;
      if constexpr (deepp16_row_done_at(d5) >= 0) retire_store(deepp16_row_done_at(d5), 0);
      if constexpr (deepp16_row_done_at(d6) >= 0) retire_store(deepp16_row_done_at(d6), 1);
      if constexpr (deepp16_row_done_at(d9) >= 0) retire_store(deepp16_row_done_at(d9), 2);
      if constexpr (deepp16_row_done_at(d10) >= 0) retire_store(deepp16_row_done_at(d10), 3);
      if constexpr (deepp16_row_done_at(d1) >= 0) retire_write(deepp16_row_done_at(d1));
      if constexpr (deepp16_row_done_at(d3) >= 0) retire_read(0);
      if constexpr (deepp16_row_done_at(d7) >= 0) retire_read(1);
      fence();
    });
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using BT = std::integral_constant<bool, true>;
  using BF = std::integral_constant<bool, false>;

  // ---- prologue: stages 0 and 1 in flight; stage 0 landed -> its half 0 into register set 0 --------------------------------------------------------------------
  dma_stage(cur, 0, true, 0);
  dma_stage(cur, 1, true, 1);
  asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  fence();
  if constexpr (IL) {
#pragma unroll
    for (int k = 0; k < MT + NT; ++k) read_scale(0, k);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) read_raw(0, 0, k);
  }
  read_base(0, 0);
#pragma unroll
  for (int i = 0; i < MT + NT; ++i) read_frag(0, i);
  if constexpr (!IL) {
#pragma unroll
    for (int k = 0; k < 16; ++k) shift1(0, k);
  }
  fence();

  // stage 0 (accumulators start from 0); its DMA is stage 2 (K <= 512: out of range, a zero fill of the buffer nobody reads again)
  stage(I0{}, BT{}, 2, true, I1{});
  int kt = 1;
  if constexpr (LEAN) {   // the pairs that fetch stages kt + 2, kt + 3 < KT - 1
    for (; kt + 4 < KT; kt += 2) {
      stage(I1{}, BF{}, kt + 2, true, I2{});
      stage(I0{}, BF{}, kt + 3, true, I2{});
    }
  }
  for (; kt + 4 < KTe; kt += 2) {   // (KL_DMA: at most once, and only for an odd KT >= 5 -- the pair that fetches its last stage; the launcher sends even stage counts here)
    stage(I1{}, BF{}, kt + 2, true, I1{});
    stage(I0{}, BF{}, kt + 3, true, I1{});
  }
  if (kt + 2 < KTe) {
    stage(I1{}, BF{}, kt + 2, true, I1{});
    stage(I0{}, BF{}, 0, false, I0{});   // stage KTe - 2: nothing is left to fetch
  }
  final_stage();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <class C, int ST_AUX = 0, int KL = kDeepp16KLoop>
__global__ __launch_bounds__(C::THREADS) void gemm_mx_deepp16_kernel(const GemmParams p) {
  __shared__ __attribute__((aligned(16))) char smem[DeepPCfg<C>::LDS_BYTES];
  asm volatile("" :: "s"(p.A), "s"(p.D), "s"(p.K), "s"(p.b_bytes), "s"((int)gridDim.x));   // (all scalar argument loads in one round, as in gemm_mx_deepp_kernel)
  gemm_mx_deepp16<C, ST_AUX, KL>(smem, p, (int)blockIdx.x, (int)gridDim.x, p.tiles_m * p.tiles_n);
}

}  // namespace qamd
