// Grouped MXFP4 / MXFP8 GEMM for mixture-of-experts layers (extensions: grouped_matmul_mxf4_bf16_tn, grouped_matmul_mxf8_bf16_tn -- the same with (M, K) /
// (E, N, K) fp8 operands, A e4m3 or e5m2, B e4m3).  Tokens sorted by expert, A (M, K/2) with row-major scales (M, K/32)
// as fusedQuantizeMx writes them; the stacked expert weights B (E, N, K/2) with row-major scales (E, N, K/32); offs (E,) int32 = the cumulative END rows of the groups
// (torch._grouped_mm's convention).  out[r] = alpha[g] (A_r . SFA) (B_g . SFB_g)^T for every row r of group g; rows at or past offs[E - 1] are not written.
//
// One launch over all experts, the group sizes read on the device (graph capture, torch.compile): every workgroup decodes its own (expert, first row, rows, column tile)
// from offs (grouped_tile below) and runs an EXISTING tile body on it -- no new main loop:
//   form (i)  gemm_mx_os_kernel<..., GRP = true> (gemm_mx_os.hip.h): 32x32, 32x16 and 64x32 tiles on wave-owned K stages, one shot while the tile's K extent fits the LDS,
//             wave-owned rings beyond;
//   form (ii) gemm_mx_grouped_ring_kernel (below): the 64x64 pipelined ring body with row-major scale fetch (gemm_mx.hip.h gemm_mx_ringp<C, true>) at the decoded origin.
// The tile's A rows start at the group's first row (any row: row-major scales need no 128-row alignment); the A / A-scale descriptors END at the group's last row, so the
// rows of a tile past its group read zeros exactly as rows past M do in the plain kernels, and the stores are masked to the group's rows.  B and its scales are rebased to
// expert g in 64-bit arithmetic (a stacked weight may exceed 2 GiB; one expert's stays below), alpha to alpha[g] when the caller passes one per expert.
#pragma once
#include <type_traits>

#include "gemm_mx.hip.h"

namespace qamd {

constexpr int GRP_MAX_E = 1024;   // experts per launch
constexpr int GRP_CPL = 16;       // groups per lane of the decode wave (64 lanes x 16 = GRP_MAX_E)

struct GroupedParams : GemmParams {   // A, SFA, alpha, D, M, N, K, ldd, a_bytes, sfa_bytes as for one GEMM over all M rows; B / SFB: expert 0, b_bytes / sfb_bytes:
                                      // ONE expert's weight / scales; tiles_n = column tiles of the form; ws / ctr unused (no split)
  const int* offs;  // (E,) cumulative end rows
  int E;
  int n_alpha;      // 1: alpha[0] for every group, E: alpha[g]
};

struct GroupTile {
  int g, row0, rows, nt;   // expert, first row, rows (1 ... TM), column tile
};

// ---- the grouped ops' formats (host): the ONE place where a form's tile is written -------------------------------------------------------------------------
// An op has up to four forms (nforms), numbered form0 ... form0 + nforms - 1 (the lab's gemm_variant option forces one); form i runs TM x TN = tile[i] tiles.  The argument checks, the
// debug plan entries and the launchers of both units (capi.hip, gemm_nvf4_os.hip.h) read a tile from here; a launcher whose kernel carries its tile as template
// arguments takes them from the table or static_asserts against it.
struct GroupedTileDim { int tm, tn; };
struct GroupedFormat {
  const char* name;   // the C entry without its prefix
  int form0;          // first form number
  int ebits;          // bits per element
  int sgroup;         // elements per scale
  GroupedTileDim tile[4];
  int nforms = 4;     // forms the op has (tile[0 .. nforms))
  int ebits_b = 0;    // bits per element of B where they differ from A's (0: ebits)
  constexpr bool has(int form) const { return form >= form0 && form < form0 + nforms; }
  constexpr int64_t row_bytes(int64_t K) const { return K / 8 * ebits; }                              // of an A row (K % 8 == 0; ebits may exceed 8, and K * ebits may not overflow)
  constexpr int64_t row_bytes_b(int64_t K) const { return K / 8 * (ebits_b ? ebits_b : ebits); }      // of a B row
};
constexpr GroupedFormat GRP_MXF4{"grouped_matmul_mxf4_bf16_tn", 590, 4, 32, {{32, 32}, {32, 16}, {64, 32}, {64, 64}}};
constexpr GroupedFormat GRP_MXF8{"grouped_matmul_mxf8_bf16_tn", 594, 8, 32, {{32, 32}, {32, 16}, {64, 32}, {64, 64}}};
constexpr GroupedFormat GRP_NVF4{"grouped_matmul_nvf4_bf16_tn", 598, 4, 16, {{32, 32}, {64, 32}, {64, 64}, {128, 128}}};
// W4A8: e4m3 tokens against e2m1 weights (gemm_mx_os_w4a8.hip.h) -- the three wave-owned forms, no ring form
constexpr GroupedFormat GRP_MXF8_MXF4{"grouped_matmul_mxf8_mxf4_bf16_tn", 602, 8, 32, {{32, 32}, {32, 16}, {64, 32}, {0, 0}}, 3, 4};
// W4A16: bf16 tokens WITHOUT scales against e2m1 weights (gemm_mx_os_w4a16.hip.h) -- the three wave-owned forms, no ring form; sgroup is the weights'
constexpr GroupedFormat GRP_BF16_MXF4{"grouped_matmul_bf16_mxf4_bf16_tn", 606, 16, 32, {{32, 32}, {32, 16}, {64, 32}, {0, 0}}, 3, 4};
// W4A6: e2m3 tokens, four codes in three bytes (an A row is 3 K / 4 bytes), against e2m1 weights (gemm_mx_os_w4a6.hip.h) -- the three wave-owned forms, no ring form
constexpr GroupedFormat GRP_MXF6_MXF4{"grouped_matmul_mxf6_mxf4_bf16_tn", 610, 6, 32, {{32, 32}, {32, 16}, {64, 32}, {0, 0}}, 3, 4};
// workgroups of a grouped launch: (m-tile slots cdiv(M, TM) + E) x column tiles -- the host's upper bound of the real tiles (grouped_tile: the rest return at once)
constexpr int64_t grouped_workgroups(int64_t M, int64_t N, int64_t E, int TM, int TN) { return ((M + TM - 1) / TM + E) * ((N + TN - 1) / TN); }

// ---- the tile decode: ONE function for the device and the host (qutlass_amd_debug_grouped_decode runs it on the CPU) ---------------------------------------
// Each group's end row is clamped to [0, M] and raised to the largest end before it, so a decreasing (malformed) offset is an empty group and every row range stays
// inside [0, M) -- for well-formed offs this is exactly rows [offs[g - 1], offs[g]).  Lane l of a wave holds groups l c ... l c + c - 1, c = ceil(E / 64) <= 16, read in
// one load round trip; a max scan gives each lane the end row before its first group, a sum scan the m-tile count before it (ceil(rows_g / TM) per group) and the total
// T.  Workgroup b < T tiles_n takes tile grp_raster(b) and a ballot finds the lane that holds its m-tile; the host sizes the grid by the bound (cdiv(M, TM) + E) tiles_n,
// and the workgroups past T tiles_n -- the last ones dispatched -- have no work.

__host__ __device__ __forceinline__ int grp_clamp(int v, int M) { return v < 0 ? 0 : v > M ? M : v; }

// one lane's groups: e[0 .. cl) their clamped end rows, `start` the end row before them.  Returns the lane's m-tile count; when 0 <= r < that count, (gi, row0, rows)
// = tile r of the lane (group index within the lane, first row, rows).
__host__ __device__ __forceinline__ int grp_lane_walk(const int* e, int cl, int start, int TM, int r, int& gi, int& row0, int& rows) {
  int s = start, t = 0;
  gi = 0; row0 = 0; rows = 0;
#pragma unroll
  for (int i = 0; i < GRP_CPL; ++i) {
    if (i < cl) {
      const int en = e[i] > s ? e[i] : s;
      const int n = (en - s + TM - 1) / TM;
      if (r >= t && r < t + n) {
        gi = i;
        row0 = s + (r - t) * TM;
        rows = en - row0 < TM ? en - row0 : TM;
      }
      t += n;
      s = en;
    }
  }
  return t;
}

// lane l's share of offs: cl groups (0 for lanes past E), their clamped ends, and the largest of them (0 if none)
__host__ __device__ __forceinline__ int grp_lane_load(const int* offs, int E, int M, int lane, int* e, int& cmax) {
  const int c = (E + 63) >> 6, first = lane * c;
  const int cl = E - first < 0 ? 0 : E - first > c ? c : E - first;
#pragma unroll
  for (int i = 0; i < GRP_CPL; ++i) {   // unconditional, in-bounds loads: one round trip
    const int idx = first + i < E ? first + i : E - 1;
    e[i] = grp_clamp(offs[idx], M);
  }
  cmax = 0;
#pragma unroll
  for (int i = 0; i < GRP_CPL; ++i)
    if (i < cl && e[i] > cmax) cmax = e[i];
  return cl;
}

// the real tiles, T m-tiles x tiles_n column tiles, in the grouped raster of the plain kernels (4 m-tiles walked column by column) but WITHOUT their XCD remap: the
// dispatcher deals consecutive workgroups to the 8 XCDs round-robin, so all XCDs stream the same expert's weight columns at the same time (shared in the memory-side
// cache) as they do in a per-expert launch -- an XCD-contiguous order had each XCD on a different expert at once (Mixtral-8x7B gate/up prefill: 1.20 x the per-expert
// loop's time against 1.0 x).  b < T tiles_n.
__host__ __device__ __forceinline__ void grp_raster(int b, int T, int tiles_n, int& mt, int& nt) {
  const int group = 4 * tiles_n, gid = b / group, first = gid * 4;
  const int gsz = T - first < 4 ? T - first : 4, rem = b - gid * group;
  mt = first + rem % gsz;
  nt = rem / gsz;
}

// workgroup b of a grouped launch with tiles_n column tiles -> its tile, or false: no work.  Device: every wave of the workgroup decodes on its own (same loads, same
// result; no barrier).
__host__ __device__ inline bool grouped_tile(const int* offs, int E, int M, int TM, int tiles_n, int b, GroupTile& out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lane = (int)(threadIdx.x & 63);
  int e[GRP_CPL], cmax;
  const int cl = grp_lane_load(offs, E, M, lane, e, cmax);
  int incl = cmax;   // inclusive max scan
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d && t > incl) incl = t;
  }
  int start = __shfl_up(incl, 1, 64);
  if (lane == 0) start = 0;
  int gi, row0, rows;
  const int tiles = grp_lane_walk(e, cl, start, TM, -1, gi, row0, rows);
  int sum = tiles;   // inclusive sum scan
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(sum, d, 64);
    if (lane >= d) sum += t;
  }
  const int total = uniform(__builtin_amdgcn_readlane(sum, 63));
  if (b >= total * tiles_n) return false;
  int mt, nt;
  grp_raster(b, total, tiles_n, mt, nt);
  mt = uniform(mt);
  const unsigned long long hit = __builtin_amdgcn_ballot_w64(sum > mt);   // lowest lane whose inclusive count passes mt
  const int L = uniform(__builtin_ffsll((long long)hit) - 1);
  grp_lane_walk(e, cl, start, TM, mt - (sum - tiles), gi, row0, rows);
  const int c = (E + 63) >> 6;
  out.g = uniform(__builtin_amdgcn_readlane(lane * c + gi, L));
  out.row0 = uniform(__builtin_amdgcn_readlane(row0, L));
  out.rows = uniform(__builtin_amdgcn_readlane(rows, L));
  out.nt = uniform(nt);
  return true;
#else   // the same lane functions, the 64 lanes one after the other
  int e[64][GRP_CPL], cl[64], cmax[64], start[64], tiles[64];
  for (int l = 0; l < 64; ++l) cl[l] = grp_lane_load(offs, E, M, l, e[l], cmax[l]);
  int run = 0, sum = 0, gi, row0, rows;
  for (int l = 0; l < 64; ++l) {
    start[l] = run;
    run = cmax[l] > run ? cmax[l] : run;
    tiles[l] = grp_lane_walk(e[l], cl[l], start[l], TM, -1, gi, row0, rows);
  }
  int total = 0, mt, nt;
  for (int l = 0; l < 64; ++l) total += tiles[l];
  if (b >= total * tiles_n) return false;
  grp_raster(b, total, tiles_n, mt, nt);
  for (int l = 0; l < 64; ++l) {
    if (mt < sum + tiles[l]) {
      grp_lane_walk(e[l], cl[l], start[l], TM, mt - sum, gi, row0, rows);
      out.g = l * ((E + 63) >> 6) + gi;
      out.row0 = row0;
      out.rows = rows;
      out.nt = nt;
      return true;
    }
    sum += tiles[l];
  }
  return false;
#endif
}

#if defined(__HIPCC__)
// the grouped parts of a tile's single-GEMM view: its origin, the group's end row (A / A-scale ranges and stores end there), expert g's B / B-scales / alpha
struct GroupedView {
  int m0, n0, M;
  uint32_t a_bytes, sfa_bytes;
  const uint8_t* B;
  const uint8_t* SFB;
  const float* alpha;
};
// workgroup -> the grouped parts of its tile's view, false: no work (EBITS: element width of A, 4 = MXFP4, 6 = MXFP6 -- K % 4 == 0 --, 8 = MXFP8, 16 = bf16)
template <int TM, int TN, int EBITS = 4>
__device__ __forceinline__ bool grouped_setup(const GroupedParams& pk, GroupedView& v) {
  GroupTile t;
  if (!grouped_tile(pk.offs, pk.E, pk.M, TM, pk.tiles_n, (int)blockIdx.x, t)) return false;
  const int g = uniform(t.g), gend = uniform(t.row0 + t.rows);
  const uint32_t rowbytes = EBITS == 16 ? (uint32_t)pk.K << 1 : EBITS == 8 ? (uint32_t)pk.K : EBITS == 6 ? ((uint32_t)pk.K >> 2) * 3u : (uint32_t)pk.K >> 1, KB = (uint32_t)pk.K >> 5;
  v.M = gend;                                      // stores masked to the group's rows ...
  v.a_bytes = (uint32_t)gend * rowbytes;           // ... and reads past them return zeros
  v.sfa_bytes = (uint32_t)gend * KB;
  v.B = pk.B + (size_t)g * pk.b_bytes;             // 64-bit: the stacked weight may exceed 2 GiB
  v.SFB = pk.SFB + (size_t)g * pk.sfb_bytes;
  v.alpha = pk.alpha + (pk.n_alpha > 1 ? g : 0);
  v.m0 = uniform(t.row0);
  v.n0 = uniform(t.nt * TN);
  return true;
}

// form (ii): the 64x64 pipelined ring body with row-major scale fetch (matmul_ada_mxf4_bf16_tn's kernel for M > 32) at the decoded tile origin.  Its configuration is a
// type of its own (same constants): the body's templates are instantiated for this kernel alone, so the compiler's view of the plain kernel's instantiation -- called
// from that kernel only -- and with it that kernel's code stay exactly as they were.
struct GroupedRingCfg : GemmCfg<64, 64, 2, 2, 4, false, 0, 3> {};
// grouped_matmul_mxf8_bf16_tn's: the tiles of matmul_mxf8_bf16_tn's product ring (split 8-bit fragments, MX_FORMS MXV_RING64 for MXFP8), A e4m3 (AFMT 0) or e5m2 (1)
template <int AFMT>
struct GroupedRing8Cfg : GemmCfg<64, 64, 2, 2, 8, true, 0, 3, AFMT> {};
template <class C>
__global__ __launch_bounds__(C::THREADS, (gemm_min_waves_per_eu<C, SCHED_RINGP_RM>())) void gemm_mx_grouped_ring_kernel(const GroupedParams pk) {
  static_assert(C::BM == 64 && C::BN == 64, "64x64 tiles");
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass of this unit does not resolve the body's device templates; it only needs the kernel's symbol)
  GroupedView v;
  if (!grouped_setup<C::BM, C::BN, C::EBITS>(pk, v)) return;
  GemmParams p = pk;
  p.M = v.M; p.a_bytes = v.a_bytes; p.sfa_bytes = v.sfa_bytes; p.B = v.B; p.SFB = v.SFB; p.alpha = v.alpha;
  p.tiles_m = 1; p.tiles_n = 1;
  gemm_mx_ringp<C, true>(smem, p, 0, v.m0, v.n0);
#endif
}
#endif

}  // namespace qamd
