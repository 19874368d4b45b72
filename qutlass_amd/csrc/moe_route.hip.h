// MoE routing: the step in front of the dispatch -> grouped GEMM -> combine chain.
//   moe_topk_softmax_kernel   router logits (T, E) -> the top-k expert ids (exact, ties to the lower index) and their softmax weights, one wave per token
//   moe_topk_grouped_kernel   the same skeleton for grouped routers (DeepSeek-V2 / V3, Kimi-K2): sigmoid or softmax scores, a selection bias, a top-k over the
//                             experts of the best topk_group of n_group groups; selection runs on the biased score c, the weights are the unbiased scores
//   moe_sort_kernel           (T, topk) expert ids -> src_row / offs / pos of a STABLE sort by expert: a counting sort without atomics and without any
//                             workgroup waiting on another (one workgroup in one launch, or count / scan / scatter in three launches ordered by the stream)
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
  constexpr int VEC = 16 / (int)sizeof(T);
  static_assert(R % VEC == 0, "whole vectors per lane");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t e = (uint32_t)p.e;
  auto column = [lane](int r) { return (uint32_t)(((r / VEC) * 64 + lane) * VEC + r % VEC); };
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < p.t; t += (int64_t)gridDim.x * 4) {
    const T* row = (const T*)p.logits + t * p.e;
    uint32_t key[R];
    if constexpr (!LOADV) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t j = column(r);
        uint32_t bits = 0;
        if (j < e) {
          if constexpr (sizeof(T) == 2) bits = (uint32_t)((const uint16_t*)row)[j] << 16;
          else bits = ((const uint32_t*)row)[j];
        }
        key[r] = j < e ? route_key(bits) : 0u;
      }
    } else {
#pragma unroll
      for (int c = 0; c < R / VEC; ++c) {
        const uint32_t j0 = column(c * VEC);
        v4i raw = {0, 0, 0, 0};
        if (j0 < e) raw = *(const v4i*)(row + j0);   // E % VEC == 0: a vector is all inside the row or all outside
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          uint32_t bits;
          if constexpr (sizeof(T) == 2) bits = (i & 1) ? ((uint32_t)raw[i / 2] & 0xffff0000u) : ((uint32_t)raw[i / 2] << 16);
          else bits = (uint32_t)raw[i];
          key[c * VEC + i] = j0 < e ? route_key(bits) : 0u;
        }
      }
    }
    float m = 0.f, denom = 1.f, my_x = 0.f;
    uint32_t my_id = 0;
    for (int k = 0; k < p.topk; ++k) {
      uint32_t hi = key[0];
      int br = 0;
#pragma unroll
      for (int r = 1; r < R; ++r) {   // strictly greater: the lane's lowest column wins a tie
        const bool g = key[r] > hi;
        hi = g ? key[r] : hi;
        br = g ? r : br;
      }
      uint32_t lo = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) lo = br == r ? ~column(r) : lo;
      lo = hi ? lo : 0u;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {   // max of (hi, lo): the largest key, then the smallest column
        const uint32_t oh = (uint32_t)__shfl_xor((int)hi, off), ol = (uint32_t)__shfl_xor((int)lo, off);
        const bool g = oh > hi || (oh == hi && ol > lo);
        hi = g ? oh : hi;
        lo = g ? ol : lo;
      }
      const uint32_t win = ~lo;   // (topk <= E: a candidate is always left, so win < E)
      const float x = route_key_value(hi);
      if (k == 0) {
        m = x;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) s += key[r] ? expf(route_key_value(key[r]) - m) : 0.f;
        denom = wave_sum(s);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = column(r) == win ? 0u : key[r];
      if (lane == k) {
        my_id = win;
        my_x = x;
      }
    }
    float w = lane < p.topk ? expf(my_x - m) / denom : 0.f;
    if (p.renorm) w = w / wave_sum(w);
    if (lane < p.topk) {
      p.weights[t * p.topk + lane] = w;
      p.ids[t * p.topk + lane] = (int32_t)my_id;
    }
  }
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
  constexpr int VEC = 16 / (int)sizeof(T);
  static_assert(R % VEC == 0 && R % 4 == 0, "whole vectors per lane");
  __shared__ __attribute__((aligned(16))) float crow[4][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t e = (uint32_t)p.e;
  auto column = [lane](int r) { return (uint32_t)(((r / VEC) * 64 + lane) * VEC + r % VEC); };
  const bool has_bias = p.bias != nullptr, grouped = p.n_group > 1;
  float bias[R];
#pragma unroll
  for (int r = 0; r < R; ++r) bias[r] = has_bias && column(r) < e ? p.bias[column(r)] : 0.f;
  // the group stage's lane roles: L lanes per group
  const int L = 1 << p.lg_l, my_g = lane >> p.lg_l, sub = lane & (L - 1);
  const bool g_active = my_g < p.n_group;
  const int steps = (p.s + L - 1) >> p.lg_l;                     // walk steps (the last one may be past the group's end for some lanes)
  const int rot = (p.s & 31) == 0 ? my_g % steps : 0;            // s % 32 == 0: s % L == 0 too, every lane has exactly `steps` elements

  for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < p.t; t += (int64_t)gridDim.x * 4) {
    const T* row = (const T*)p.logits + t * p.e;
    float s[R];   // the logit, then the score
    if constexpr (!LOADV) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t j = column(r);
        uint32_t bits = 0;
        if (j < e) {
          if constexpr (sizeof(T) == 2) bits = (uint32_t)((const uint16_t*)row)[j] << 16;
          else bits = ((const uint32_t*)row)[j];
        }
        s[r] = __uint_as_float(bits);
      }
    } else {
#pragma unroll
      for (int c = 0; c < R / VEC; ++c) {
        const uint32_t j0 = column(c * VEC);
        v4i raw = {0, 0, 0, 0};
        if (j0 < e) raw = *(const v4i*)(row + j0);   // E % VEC == 0: a vector is all inside the row or all outside
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          uint32_t bits;
          if constexpr (sizeof(T) == 2) bits = (i & 1) ? ((uint32_t)raw[i / 2] & 0xffff0000u) : ((uint32_t)raw[i / 2] << 16);
          else bits = (uint32_t)raw[i];
          s[c * VEC + i] = __uint_as_float(bits);
        }
      }
    }
    // scores
    if (p.sigmoid) {
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] = 1.f / (1.f + expf(-s[r]));
    } else {
      float m = -INFINITY;
#pragma unroll
      for (int r = 0; r < R; ++r) m = column(r) < e ? fmaxf(m, s[r]) : m;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        s[r] = column(r) < e ? expf(s[r] - m) : 0.f;
        sum += s[r];
      }
      const float denom = wave_sum(sum);
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] = s[r] / denom;
    }
    if (p.scores) {
      float* out = p.scores + t * p.e;
      if constexpr (LOADV) {   // the host takes this path only when the scores' rows start on 16-byte boundaries too
#pragma unroll
        for (int q4 = 0; q4 < R / 4; ++q4) {
          const uint32_t j0 = column(q4 * 4);
          if (j0 < e) *(v4f*)(out + j0) = v4f{s[q4 * 4], s[q4 * 4 + 1], s[q4 * 4 + 2], s[q4 * 4 + 3]};
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (column(r) < e) out[column(r)] = s[r];
      }
    }
    // choice values and their keys
    uint32_t key[R];
    if (!grouped) {
#pragma unroll
      for (int r = 0; r < R; ++r) key[r] = column(r) < e ? route_key(__float_as_uint(has_bias ? s[r] + bias[r] : s[r])) : 0u;
    } else {
      float* mine = crow[wave];
#pragma unroll
      for (int q4 = 0; q4 < R / 4; ++q4) {
        float c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = q4 * 4 + i;
          c[i] = has_bias ? s[r] + bias[r] : s[r];
          key[r] = column(r) < e ? route_key(__float_as_uint(c[i])) : 0u;
        }
        *(v4f*)(mine + column(q4 * 4)) = v4f{c[0], c[1], c[2], c[3]};   // column(R - 1) < R * 64 <= 1024: columns past E land in the row's unused tail
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      uint32_t k1 = 0, k2 = 0;   // the group's two largest keys so far (0 = none)
      if (g_active) {
        const float* grp = mine + my_g * p.s;
        int i = rot;
        for (int n = 0; n < steps; ++n) {
          const int idx = sub + (i << p.lg_l);
          if (idx < p.s) {
            const uint32_t k = route_key(__float_as_uint(grp[idx]));
            k2 = k > k1 ? k1 : (k > k2 ? k : k2);
            k1 = k > k1 ? k : k1;
          }
          i = i + 1 == steps ? 0 : i + 1;
        }
      }
      for (int off = 1; off < L; off <<= 1) {   // merge the top two of the L lanes of a group (lanes of one group differ in their low lg_l bits only)
        const uint32_t o1 = (uint32_t)__shfl_xor((int)k1, off), o2 = (uint32_t)__shfl_xor((int)k2, off);
        const uint32_t lo1 = k1 < o1 ? k1 : o1, hi2 = k2 > o2 ? k2 : o2;
        k1 = k1 > o1 ? k1 : o1;
        k2 = lo1 > hi2 ? lo1 : hi2;
      }
      uint32_t gk = k1;   // without a bias: the group's largest c
      if (has_bias && k2 != 0u) gk = route_key(__float_as_uint(route_key_value(k1) + route_key_value(k2)));   // (a group of one expert scores that one value)
      int rank = 0;
      for (int g = 0; g < p.n_group; ++g) {
        const uint32_t og = (uint32_t)__builtin_amdgcn_readlane((int)gk, g << p.lg_l);
        rank += (og > gk || (og == gk && g < my_g)) ? 1 : 0;
      }
      const unsigned long long alive = __ballot(g_active && sub == 0 && rank < p.topk_group);   // bit (g << lg_l): group g survives
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t g = (column(r) * p.magic) >> 22;   // column(r) < 1024; a column past E has key 0 already, whatever g says
        key[r] = ((alive >> ((g << p.lg_l) & 63u)) & 1ull) ? key[r] : 0u;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the walk's reads are done before the next token's row is written
      __builtin_amdgcn_wave_barrier();
    }
    // selection: topk rounds of (key descending, column ascending); lane k keeps round k's pick and its UNBIASED score
    float my_s = 0.f;
    uint32_t my_id = 0;
    for (int k = 0; k < p.topk; ++k) {
      uint32_t hi = key[0];
      int br = 0;
#pragma unroll
      for (int r = 1; r < R; ++r) {   // strictly greater: the lane's lowest column wins a tie
        const bool g = key[r] > hi;
        hi = g ? key[r] : hi;
        br = g ? r : br;
      }
      uint32_t lo = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) lo = br == r ? ~column(r) : lo;
      lo = hi ? lo : 0u;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t oh = (uint32_t)__shfl_xor((int)hi, off), ol = (uint32_t)__shfl_xor((int)lo, off);
        const bool g = oh > hi || (oh == hi && ol > lo);
        hi = g ? oh : hi;
        lo = g ? ol : lo;
      }
      const uint32_t win = ~lo;   // (topk <= topk_group * s: a candidate is always left, so win < E)
      float ws = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool hit = column(r) == win;
        ws = hit ? s[r] : ws;
        key[r] = hit ? 0u : key[r];
      }
      const int owner = __builtin_amdgcn_readfirstlane((int)((win / VEC) & 63u));   // the lane that holds column `win` (every lane has the same win)
      ws = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ws), owner));
      if (lane == k) {
        my_id = win;
        my_s = ws;
      }
    }
    float w = lane < p.topk ? my_s : 0.f;
    if (p.renorm) w = w / wave_sum(w);
    w = w * p.scale;
    if (lane < p.topk) {
      p.weights[t * p.topk + lane] = w;
      p.ids[t * p.topk + lane] = (int32_t)my_id;
    }
  }
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

template <typename IdT>
__device__ __forceinline__ int moe_sort_key(const MoeSortParams& p, int64_t slot) {
  long long id = (long long)((const IdT*)p.ids)[slot];
  if (p.map) id = (id >= 0 && id < p.g) ? (long long)p.map[id] : -1ll;   // an id outside [0, g) is dropped without reading the map
  return (id >= 0 && id < p.e) ? (int)id : p.e;
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

template <typename IdT, int MODE>
__global__ __launch_bounds__(MOE_SORT_NT) void moe_sort_kernel(const MoeSortParams p) {
  __shared__ uint32_t cnt[MOE_SORT_W * MOE_SORT_MAXK];
  __shared__ uint32_t wsum[MOE_SORT_W];
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
    const int key = active ? moe_sort_key<IdT>(p, slot) : 0;
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
      const int key = active ? moe_sort_key<IdT>(p, slot) : 0;
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

}  // namespace qamd
