// MoE routing: the step in front of the dispatch -> grouped GEMM -> combine chain.
//   moe_topk_softmax_kernel   router logits (T, E) -> the top-k expert ids (exact, ties to the lower index) and their softmax weights, one wave per token
//   moe_topk_grouped_kernel   the same skeleton for grouped routers (DeepSeek-V2 / V3, Kimi-K2): sigmoid or softmax scores, a selection bias, a top-k over the
//                             experts of the best topk_group of n_group groups; selection runs on the biased score c, the weights are the unbiased scores
//   moe_sort_kernel           (T, topk) expert ids -> src_row / offs / pos of a STABLE sort by expert: a counting sort without atomics and without any
//                             workgroup waiting on another (one workgroup in one launch, or count / scan / scatter in three launches ordered by the stream)
//   moe_route_fused_kernel, moe_route_grouped_fused_kernel   decode (T <= 64): either router and the one-workgroup sort in ONE launch of one workgroup -- the routers'
//                             own code (moe_topk_*_rows.inc) and the sort's (moe_sort_workgroup) with one barrier between them, the sort keys handed over in LDS
// All are plain wave64 code: no LDS in the first, 16 KiB of wave-private rows in the second (touched only when n_group > 1), 33 KiB of LDS counters in the third.
#pragma once
#include "common.hip.h"

namespace qamd {

// ---- top-k softmax ----------------------------------------------------------------------------------------------------------------------------------------
// Selection runs on an order-preserving integer image of the logit, never on a probability: key(x) is monotone in x as a floating-point number, -0 and +0 share
// one key (so they tie and the lower index wins), -inf has the lowest key of all numbers, and a NaN gets SOME key (its row's weights are unspecified, its ids
// are still distinct and in range).  Real elements have key >= 1; 0 marks "not a candidate": a column past E, or an expert already taken.
__device__ __forceinline__ uint32_t route_key(uint32_t bits) {
  const uint32_t u = bits == 0x80000000u ? 0u : bits;
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return k ? k : 1u;
}
__device__ __forceinline__ float route_key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ float wave_sum(float v) {   // every lane ends with the same bits: a + b and b + a round alike
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

struct MoeTopkParams {
  const void* logits;   // (T, E) bf16 or float32
  float* weights;       // (T, topk)
  int32_t* ids;         // (T, topk)
  int64_t t;
  int e, topk, renorm;
};

// One wave per token, four tokens per workgroup, the whole row in registers: lane l holds R candidates, column ((r / VEC) * 64 + l) * VEC + r % VEC for r < R --
// VEC = 8 bf16 / 4 float consecutive columns, one 16-byte load when LOADV (every row starts on a 16-byte boundary), VEC loads of one column otherwise.  The
// columns a lane holds do not depend on LOADV or on R, so neither do the sums: a row gives the same bits wherever it lies in memory.
// R * 64 >= E.  Then topk rounds of an arg-max over (key descending, column ascending): R compares in the lane, six butterfly steps across the wave on the
// 64-bit pair (key, ~column), and the owner strikes the winner out.  Round 0's winner is the row maximum m; the denominator sum_j exp(x_j - m) is taken right
// there, before anything is struck out.  Lane k keeps round k's pick and writes slot k.  No LDS, no barrier, no workspace.
template <typename T, int R, bool LOADV>
__global__ __launch_bounds__(256) void moe_topk_softmax_kernel(const MoeTopkParams p) {
#define MOE_ROWS_WAVES 4
#define MOE_ROWS_EMIT(slot, id)
#include "moe_topk_softmax_rows.inc"
#undef MOE_ROWS_WAVES
#undef MOE_ROWS_EMIT
}

// ---- grouped top-k ----------------------------------------------------------------------------------------------------------------------------------------
struct MoeGroupedParams {
  const void* logits;   // (T, E) bf16 or float32
  const float* bias;    // (E) or null: added to the score for the CHOICE only
  float* weights;       // (T, topk)
  int32_t* ids;         // (T, topk)
  float* scores;        // (T, E) or null
  int64_t t;
  int e, topk, renorm, sigmoid;
  int n_group, topk_group, s;   // s = e / n_group experts per group
  int lg_l;                     // log2 of the lanes that share one group in the group stage: the largest power of two L with n_group * L <= 64
  uint32_t magic;               // ceil(2^22 / s): (j * magic) >> 22 == j / s for every j < 1024 (j * (magic * s - 2^22) < 2^20 * 1 < 2^22; j * magic < 2^32)
  float scale;                  // routed_scaling_factor
};

// moe_topk_softmax_kernel's skeleton -- one wave per token, four tokens per workgroup, lane l holding the same R columns, the same two load paths, the same topk
// rounds of the (key, ~column) butterfly arg-max, key 0 = "not a candidate" -- with three differences:
//   scores   s_j = 1 / (1 + exp(-x_j)), or the softmax p_j (m by a wave max, the sum in moe_topk_softmax's order), kept in registers beside the keys: they are the
//            weights, and the optional (T, E) output
//   choice   the keys are those of c_j = s_j + bias_j (one fp32 add; the bias is read once per wave, before the token loop), not of the logits
//   groups   n_group > 1: the wave parks its c row in ITS OWN 4 KiB of LDS (16-byte writes, the lane's columns are consecutive in fours), L = 2^lg_l lanes per
//            group walk the group's s values with stride L for the two largest keys (one without a bias), log2 L butterfly steps merge them, one fp32 add makes the
//            group's score and route_key its key; n_group readlanes rank the groups by (key descending, index ascending), a ballot turns "rank < topk_group" into
//            a 64-bit mask, and every lane zeroes the keys of its columns whose group (j / s by the multiply-shift above) is not in it.
//            The stride-L walk puts the lanes of one group on consecutive banks; groups whose starts are a multiple of 32 words apart would share them (s = 32,
//            L = 8: four groups per 32-lane half on eight banks), so for s % 32 == 0 group g starts its walk g steps in (the order within a lane is free for a
//            top-2): the 32 / L groups of a half then sit on different banks.
// Nothing is fused: the bias add, the top-2 add and the final multiply are single roundings (fp contract off), so numpy repeats them from the returned scores.
// No workspace, no atomics, no barrier: the LDS row is wave-private, ordered by wavefront fences.
template <typename T, int R, bool LOADV>
__global__ __launch_bounds__(256) void moe_topk_grouped_kernel(const MoeGroupedParams p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float crow[4][1024];
#define MOE_ROWS_WAVES 4
#define MOE_ROWS_EMIT(slot, id)
#include "moe_topk_grouped_rows.inc"
#undef MOE_ROWS_WAVES
#undef MOE_ROWS_EMIT
}

// The launch of either router: a pure function of the shape, the CU count and whether the entry found its pointers 16-byte aligned (with a row length of whole vectors: 16-byte loads
// and stores; same layout, same bits, either way).  R = the smallest instantiated size with R * 64 >= E: 8 or 16, and 4 for float32 logits alone (four floats fill a vector, four bf16 do not).
struct MoeTopkLaunch { int R; bool loadv; int grid, threads; };
inline MoeTopkLaunch moe_topk_plan(int elem_bytes, int64_t e, int64_t t, bool rows_16B_aligned, int64_t cus) {
  const int64_t per_lane = (e + 63) / 64;   // columns a lane has to hold: 1 .. 16, in whole vectors of 16 bytes
  return {elem_bytes == 4 && per_lane <= 4 ? 4 : per_lane <= 8 ? 8 : 16, rows_16B_aligned && (e * elem_bytes) % 16 == 0, (int)std::min<int64_t>((t + 3) / 4, cus * 16), 256};
}

// ---- expert sort ------------------------------------------------------------------------------------------------------------------------------------------
// A counting sort on key = expert id, or E for a dropped slot (an id outside [0, E), before or after expert_map).  Stability comes from the order of the counts,
// not from any order of execution: a workgroup takes `spb` consecutive slots, each of its 8 waves a consecutive run of 64-slot chunks, and
//   pass 1   every wave counts its own slots into its OWN row of LDS counters: the lanes of a chunk that hold one key are found with nbits = bits(E) ballots,
//            the lowest such lane adds their number -- one writer per counter, no atomic;
//   scan     the counters are replaced by their exclusive prefix in (key, workgroup, wave) order;
//   pass 2   every wave walks its chunks again: row = counter[wave][key] + (lanes below me with my key); the lowest lane moves the counter on.
// MODE 0 is all of it in one workgroup (offs too).  MODE 1 is pass 1 of every workgroup, summed over its waves into row `blockIdx.x` of the workspace;
// moe_sort_scan_kernel turns the workspace into prefixes and writes offs; MODE 3 repeats pass 1, starts its scan from the workspace and runs pass 2.  The three
// are ordered by the stream; no workgroup ever waits on another.
constexpr int MOE_SORT_NT = 512, MOE_SORT_W = 8, MOE_SORT_MAXK = 1025;

struct MoeSortParams {
  const void* ids;        // (n) int32 or int64
  const int32_t* map;     // (g) or null
  int32_t* src_row;       // (n)
  int32_t* offs;          // (e)
  int32_t* pos;           // (n)
  uint32_t* ws;           // (rows + 1, e + 1): per-workgroup counts, then prefixes; row `rows` holds every key's first row
  int64_t n, spb;         // slots; slots per workgroup (a multiple of 512)
  int g, e, topk, nbits, rows;
};

__device__ __forceinline__ int moe_sort_key_of(const MoeSortParams& p, long long id) {
  if (p.map) id = (id >= 0 && id < p.g) ? (long long)p.map[id] : -1ll;   // an id outside [0, g) is dropped without reading the map
  return (id >= 0 && id < p.e) ? (int)id : p.e;
}
template <typename IdT>
__device__ __forceinline__ int moe_sort_key(const MoeSortParams& p, int64_t slot) {
  return moe_sort_key_of(p, (long long)((const IdT*)p.ids)[slot]);
}

// the lanes of the wave that are active and hold this lane's key
__device__ __forceinline__ unsigned long long moe_sort_peers(int key, bool active, int nbits) {
  unsigned long long m = __ballot(active);
  for (int b = 0; b < nbits; ++b) {
    const bool bit = (key >> b) & 1;
    const unsigned long long bal = __ballot(active && bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// exclusive prefix of v over the 512 threads of the workgroup, in thread order (every thread calls it, once per kernel)
__device__ __forceinline__ uint32_t moe_sort_block_scan(uint32_t v, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
    inc += lane >= off ? o : 0u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  return base + inc - v;
}

// One workgroup's part of the sort in the given MODE over the counters cnt (MOE_SORT_W * MOE_SORT_MAXK words of LDS) and wsum (MOE_SORT_W words): the code both
// moe_sort_kernel and the one-launch routing kernels run.  key_of(slot) is the slot's key in [0, E]: read from the ids (moe_sort_key), or from the LDS array the
// router of the same workgroup has just filled.
template <int MODE, typename KeyOf>
__device__ __forceinline__ void moe_sort_workgroup(const MoeSortParams& p, uint32_t* cnt, uint32_t* wsum, KeyOf key_of) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nk = p.e + 1;
  const int64_t b0 = (int64_t)blockIdx.x * p.spb, b1 = b0 + p.spb < p.n ? b0 + p.spb : p.n;
  const int chunks = b1 > b0 ? (int)((b1 - b0 + 63) >> 6) : 0;
  const int wact = chunks < MOE_SORT_W ? (chunks > 0 ? chunks : 1) : MOE_SORT_W;   // waves with work: the others' counter rows are not even cleared
  const int cpw = (chunks + wact - 1) / wact;
  const int c_begin = wave * cpw, c_end = c_begin + cpw < chunks ? c_begin + cpw : chunks;
  uint32_t* mine = cnt + (wave < wact ? wave : 0) * nk;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int i = tid; i < wact * nk; i += MOE_SORT_NT) cnt[i] = 0;
  __syncthreads();
  for (int c = c_begin; c < c_end; ++c) {
    const int64_t slot = b0 + (int64_t)c * 64 + lane;
    const bool active = slot < b1;
    const int key = active ? key_of(slot) : 0;
    const unsigned long long peers = moe_sort_peers(key, active, p.nbits);
    if (active && (peers & below) == 0) mine[key] += (uint32_t)__popcll(peers);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  __syncthreads();

  const int kpt = (nk + MOE_SORT_NT - 1) / MOE_SORT_NT;   // 1 .. 3 consecutive keys per thread
  const int k0 = tid * kpt;
  if constexpr (MODE == 1) {
    for (int i = 0; i < kpt; ++i) {
      const int k = k0 + i;
      if (k < nk) {
        uint32_t s = 0;
        for (int w = 0; w < wact; ++w) s += cnt[w * nk + k];
        p.ws[(int64_t)blockIdx.x * nk + k] = s;
      }
    }
    return;
  } else {
    uint32_t run = 0;
    if constexpr (MODE == 0) {
      uint32_t s = 0;
      for (int i = 0; i < kpt; ++i)
        if (k0 + i < nk)
          for (int w = 0; w < wact; ++w) s += cnt[w * nk + k0 + i];
      run = moe_sort_block_scan(s, wsum);
    }
    for (int i = 0; i < kpt; ++i) {
      const int k = k0 + i;
      if (k < nk) {
        if constexpr (MODE == 3) run = p.ws[(int64_t)p.rows * nk + k] + p.ws[(int64_t)blockIdx.x * nk + k];
        for (int w = 0; w < wact; ++w) {
          const uint32_t c = cnt[w * nk + k];
          cnt[w * nk + k] = run;
          run += c;
        }
        if (MODE == 0 && k < p.e) p.offs[k] = (int32_t)run;
      }
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
      const int64_t slot = b0 + (int64_t)c * 64 + lane;
      const bool active = slot < b1;
      const int key = active ? key_of(slot) : 0;
      const unsigned long long peers = moe_sort_peers(key, active, p.nbits);
      const uint32_t first = mine[key];
      if (active) {
        const uint32_t r = first + (uint32_t)__popcll(peers & below);
        if ((int64_t)r < p.n) p.src_row[r] = (int32_t)((uint32_t)slot / (uint32_t)p.topk);   // (r < n unless the ids changed between the launches)
        p.pos[slot] = key < p.e ? (int32_t)r : -1;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      if (active && (peers & below) == 0) mine[key] = first + (uint32_t)__popcll(peers);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
  }
}

template <typename IdT, int MODE>
__global__ __launch_bounds__(MOE_SORT_NT) void moe_sort_kernel(const MoeSortParams p) {
  __shared__ uint32_t cnt[MOE_SORT_W * MOE_SORT_MAXK];
  __shared__ uint32_t wsum[MOE_SORT_W];
  moe_sort_workgroup<MODE>(p, cnt, wsum, [&p](int64_t slot) { return moe_sort_key<IdT>(p, slot); });
}

// ---- one-launch routing for decode: router and sort in one workgroup --------------------------------------------------------------------------------------
// T <= MOE_ROUTE_FUSED_MAX_T tokens, so at most 64 * 32 = 2048 slots: ONE workgroup of MOE_SORT_NT threads.
//   phase 1  wave w routes tokens w, w + 8, ... with the router's own code (moe_topk_softmax_rows.inc / moe_topk_grouped_rows.inc, the text of the routers' kernels:
//            same lane-to-column map, same R / LOADV, same order of every sum -- the weights and ids are the two-launch ops' bit for bit) and writes weights and ids
//            to global memory as they do; the lane that writes a slot also leaves its sort key -- moe_sort_key's rule on the id it holds in a register -- in a
//            16-bit LDS array
//   barrier  one __syncthreads(); no global fence: phase 2 reads only LDS
//   phase 2  moe_sort_workgroup<0> (count, scan, scatter, offs) with the key of a slot taken from that array
// LDS: the sort's 32.8 KiB of counters, 4 KiB of keys, 32 bytes of wave sums.  The grouped router's eight 4 KiB rows are dead after the barrier, and the counters
// are cleared behind it: they share the counters' memory (32 KiB of its 32.8).  sp.ids is not read; sp.spb >= sp.n, sp.rows = 1.
constexpr int MOE_ROUTE_FUSED_MAX_T = 64, MOE_ROUTE_FUSED_MAX_SLOTS = MOE_ROUTE_FUSED_MAX_T * 32;
static_assert(MOE_SORT_W * MOE_SORT_MAXK >= MOE_SORT_W * 1024, "the counters hold a router row per wave");

template <typename T, int R, bool LOADV>
__global__ __launch_bounds__(MOE_SORT_NT) void moe_route_fused_kernel(const MoeTopkParams p, const MoeSortParams sp) {
  __shared__ uint32_t cnt[MOE_SORT_W * MOE_SORT_MAXK];
  __shared__ uint32_t wsum[MOE_SORT_W];
  __shared__ uint16_t keys[MOE_ROUTE_FUSED_MAX_SLOTS];
  {
#define MOE_ROWS_WAVES MOE_SORT_W
#define MOE_ROWS_EMIT(slot, id) keys[slot] = (uint16_t)moe_sort_key_of(sp, (long long)(id))
#include "moe_topk_softmax_rows.inc"
#undef MOE_ROWS_WAVES
#undef MOE_ROWS_EMIT
  }
  __syncthreads();
  moe_sort_workgroup<0>(sp, cnt, wsum, [&](int64_t slot) { return (int)keys[slot]; });
}

template <typename T, int R, bool LOADV>
__global__ __launch_bounds__(MOE_SORT_NT) void moe_route_grouped_fused_kernel(const MoeGroupedParams p, const MoeSortParams sp) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint32_t cnt[MOE_SORT_W * MOE_SORT_MAXK];
  __shared__ uint32_t wsum[MOE_SORT_W];
  __shared__ uint16_t keys[MOE_ROUTE_FUSED_MAX_SLOTS];
  {
    float (*crow)[1024] = (float (*)[1024])cnt;   // phase 1: the counters' memory holds a 4 KiB row of choice values per wave
#define MOE_ROWS_WAVES MOE_SORT_W
#define MOE_ROWS_EMIT(slot, id) keys[slot] = (uint16_t)moe_sort_key_of(sp, (long long)(id))
#include "moe_topk_grouped_rows.inc"
#undef MOE_ROWS_WAVES
#undef MOE_ROWS_EMIT
  }
  __syncthreads();
  moe_sort_workgroup<0>(sp, cnt, wsum, [&](int64_t slot) { return (int)keys[slot]; });
}

// One workgroup: ws[r][k] (the count of key k in workgroup r's slots) -> the number of slots with key k in the workgroups before r; row `rows` gets every key's
// first sorted row and offs its end.  A thread owns 1 .. 3 consecutive keys and walks the rows eight loads at a time.  (A template only so that this header can be
// included from several translation units: the parameter is not used.)
template <int UNUSED = 0>
__global__ __launch_bounds__(MOE_SORT_NT) void moe_sort_scan_kernel(const MoeSortParams p) {
  __shared__ uint32_t wsum[MOE_SORT_W];
  const int nk = p.e + 1, kpt = (nk + MOE_SORT_NT - 1) / MOE_SORT_NT, k0 = threadIdx.x * kpt;
  uint32_t tot[3] = {0, 0, 0}, s = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int k = k0 + i;
    if (i < kpt && k < nk) {
      uint32_t run = 0;
      for (int r = 0; r < p.rows; r += 8) {
        uint32_t c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = r + j < p.rows ? p.ws[(int64_t)(r + j) * nk + k] : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (r + j < p.rows) {
            p.ws[(int64_t)(r + j) * nk + k] = run;
            run += c[j];
          }
      }
      tot[i] = run;
      s += run;
    }
  }
  uint32_t run = moe_sort_block_scan(s, wsum);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int k = k0 + i;
    if (i < kpt && k < nk) {
      p.ws[(int64_t)p.rows * nk + k] = run;
      run += tot[i];
      if (k < p.e) p.offs[k] = (int32_t)run;
    }
  }
}

// The launch of the sort: a pure function of the slots n = T * topk in [0, 2^31), E and the one-launch bound (0 = the product's; the lab option "moe_sort_one_launch_max").  The scratch
// is sized by min(256, ceil(n / 4096)) rows, which the row count never exceeds (spb >= 4096 and spb >= n / 256) and which, unlike it, never shrinks as n grows.
// Up to MOE_SORT_ONE_LAUNCH_MAX slots: one workgroup, one launch.  Beyond: count, scan, scatter -- three launches over caller scratch, workgroups of
// `spb` consecutive slots (at least 4096 = 8 chunks of 64 per wave, and never more than 256 workgroups: the scratch stays below 1.01 MiB however large n is).
// The bound is measured (profiles/bench_moe_route_mi355x.txt): one workgroup costs 2.6 + 2.2 us per 1024 slots (E = 8; 2.7 + 3.2 at E = 128),
// three launches 18-19 us (24-25) from 4096 to 16384 slots; at 6144 slots one workgroup still wins (15.9 vs 18.5, 22.2 vs 23.9 us), at 8192 it has lost
// (20.4 vs 19.0, 28.6 vs 24.7).  6144 is the largest measured size at which one launch is faster for both expert counts.
constexpr int64_t MOE_SORT_ONE_LAUNCH_MAX = 6144;
struct MoeSortLaunch { int launches; int64_t spb; int rows; int64_t ws_bytes; };   // 1 or 3; MoeSortParams::spb, ::rows; the caller's scratch (0 for one launch)
inline MoeSortLaunch moe_sort_plan(int64_t n, int64_t num_experts, int64_t one_launch_max) {
  auto cdiv = [](int64_t x, int64_t y) { return (x + y - 1) / y; };
  if (n <= (one_launch_max > 0 ? one_launch_max : MOE_SORT_ONE_LAUNCH_MAX)) return {1, cdiv(n, 512) * 512, 1, 0};
  const int64_t spb = cdiv(std::max<int64_t>(4096, cdiv(n, 256)), 512) * 512;
  return {3, spb, (int)cdiv(n, spb), (std::min<int64_t>(256, cdiv(n, 4096)) + 1) * (num_experts + 1) * 4};
}

// The launch of either one-launch routing kernel: the router's own R and load path (moe_topk_plan -- neither depends on the grid), one workgroup of the sort's size.
inline MoeTopkLaunch moe_route_fused_plan(int elem_bytes, int64_t e, int64_t t, bool rows_16B_aligned) {
  const MoeTopkLaunch l = moe_topk_plan(elem_bytes, e, t, rows_16B_aligned, 1);
  return {l.R, l.loadv, 1, MOE_SORT_NT};
}
// Up to this many tokens the torch ops moe_route_fused / moe_route_grouped_fused take the one-launch kernels; beyond they run the router and the sort as two launches
// (the C entries always run the one launch, up to MOE_ROUTE_FUSED_MAX_T).  The bound is measured (profiles/bench_moe_route_fused_mi355x.txt):
// replayed graphs, one launch against moe_route / moe_route_grouped, T = 1 .. 8 (one token per wave): Mixtral-8x7B 5.3-5.8 against 8.3-8.6 us, gpt-oss-120b 6.7-7.3
// against 9.5-9.9, Qwen3-30B-A3B 8.6-9.6 against 11.4-12.0, DeepSeek-V3 10.6-12.2 against 13.4-13.8, Kimi-K2 9.9-11.4 against 12.4-13.2 -- 1.6 to 3.3 us less, many
// times either side's spread.  At T = 16 a wave routes two tokens in a row and the one launch has lost for four of the five (10.8 against 10.1 us .. 19.8 against
// 14.1; Mixtral still 8.0 against 8.7), at 64 it takes 23-64 us against 9-15.  8 is the largest T of the sweep at which one launch is faster for every router.
// The ops allocate their results without a fill, so up to the bound the op IS the one launch (op_us = fused_us in the file) and beyond it the two bare entries.
constexpr int64_t MOE_ROUTE_FUSED_TOKENS = 8;

}  // namespace qamd
