// The body of moe_topk_softmax_kernel and phase 1 of moe_route_fused_kernel (moe_route.hip.h): a FRAGMENT included inside both kernels, not a header.
// In scope where it is included:
//   p, T, R, LOADV  the kernel's MoeTopkParams and template arguments
//   MOE_ROWS_WAVES  the waves of a workgroup: wave w of workgroup b takes tokens b * MOE_ROWS_WAVES + w, then steps by the whole grid
//   MOE_ROWS_EMIT(slot, id)  run by the lane that has just written slot = t * topk + lane (the router's own kernel: nothing)
// Text and not a __device__ function: the function form moved the register lines of the existing router kernels (55 -> 56 / 57 VGPRs, 141 -> 140 / 143, other SGPR
// counts, by value / by reference), and they are to stay as they were (profiles/kernel_resources_moe_route_fused.diff).
  constexpr int VEC = 16 / (int)sizeof(T);
  static_assert(R % VEC == 0, "whole vectors per lane");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t e = (uint32_t)p.e;
  auto column = [lane](int r) { return (uint32_t)(((r / VEC) * 64 + lane) * VEC + r % VEC); };
  for (int64_t t = (int64_t)blockIdx.x * MOE_ROWS_WAVES + wave; t < p.t; t += (int64_t)gridDim.x * MOE_ROWS_WAVES) {
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
      MOE_ROWS_EMIT(t * p.topk + lane, my_id);
    }
  }
