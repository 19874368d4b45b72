// The body of moe_topk_grouped_kernel and phase 1 of moe_route_grouped_fused_kernel (moe_route.hip.h): a FRAGMENT included inside both kernels, not a header.
// In scope where it is included:
//   p, T, R, LOADV  the kernel's MoeGroupedParams and template arguments
//   crow            float (*)[1024] or an array of such rows in LDS, 16-byte aligned: crow[wave] is the wave's own 4 KiB row; fp contraction is off
//   MOE_ROWS_WAVES  the waves of a workgroup: wave w of workgroup b takes tokens b * MOE_ROWS_WAVES + w, then steps by the whole grid
//   MOE_ROWS_EMIT(slot, id)  run by the lane that has just written slot = t * topk + lane (the router's own kernel: nothing)
// Text and not a __device__ function: the function form moved the register lines of the existing router kernels (55 -> 56 / 57 VGPRs, 141 -> 140 / 143, other SGPR
// counts, by value / by reference), and they are to stay as they were (profiles/kernel_resources_moe_route_fused.diff).
  constexpr int VEC = 16 / (int)sizeof(T);
  static_assert(R % VEC == 0 && R % 4 == 0, "whole vectors per lane");
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

  for (int64_t t = (int64_t)blockIdx.x * MOE_ROWS_WAVES + wave; t < p.t; t += (int64_t)gridDim.x * MOE_ROWS_WAVES) {
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
      MOE_ROWS_EMIT(t * p.topk + lane, my_id);
    }
  }
