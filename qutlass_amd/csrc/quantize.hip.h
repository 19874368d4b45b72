// Fused rotate + quantize kernels for gfx950 (HBM-bound; 2 B/elem in, ~0.53-0.66 B/elem out; 1.03 B/elem out for the MXFP8 arm).
//
//   fusedQuantizeMx : y = x_g . h (bf16 x bf16 -> fp32, x viewed as (numel/R, R), h a RUNTIME RxR
//                     matrix), then per 32 values an e8m0 scale (abs-max or Quest) + 32 e2m1 codes
//                     [+ 32 clip-mask bits].  Replaces qutlass/csrc/fused_quantize_mx.cu:64-207,
//                     fused_quantize_mx_mask.cu:62-123 and the arithmetic of
//                     cutlass_extensions/epilogue/threadblock/epilogue_quant.h:460-812, :1087-1230.
//   fusedQuantizeNv : same rotation, per 16 values an e4m3 scale relative to a global scale.
//                     Replaces fused_quantize_nv.cu:109-252 / epilogue_quant.h:1560-2128.
//   fusedQuantizeMxf8: same rotation, per 32 values an e8m0 scale (abs-max) + 32 e4m3 or e5m2 codes: the A operand of the MXFP8 GEMMs.  No reference counterpart
//                     as a kernel; the scale rule is e8m0_shift7's (the FP8 arm of the epilogue below).
//
// CDNA4 mapping.  The rotation is computed TRANSPOSED on the bf16 MFMA:
//   D^T (32 j x 32 rows) = H^T (32 j x 16 k) . X^T (16 k x 32 rows)   [v_mfma_f32_32x32x16_bf16]
// so that after the MFMA lane (row = l&31, half = l>>5) holds 16 of the 32 values of ONE scale
// group of ONE row (j = 8q + 4*half + e) in registers: the group reduction is 15 in-register ops
// plus ONE wavefront exchange with lane l^32 (v_permlane32_swap), every lane of the wave is busy
// (the reference leaves 3 of 4 threads idle and round-trips accumulators through shared memory),
// and the X^T operand is exactly 16 contiguous bytes of the row per lane, loaded straight from
// global memory (buffer_load_dwordx4, out-of-range rows read as zero).
#pragma once
#include "common.hip.h"

namespace qamd {

enum { METHOD_QUEST = 0, METHOD_ABSMAX = 1 };
enum { QF_E2M1 = 0, QF_E4M3 = 1, QF_E5M2 = 2, QF_E2M3 = 3 };   // output code format of the kernels (FMT): 4-bit (MX / NV), one of the two 8-bit MX formats or the 6-bit one

// The constants of the clamped SwiGLU (swiglu_oai_mul8 below), made by the host from the caller's alpha and limit (swiglu_oai_act in capi.hip):
//   alpha * log2 e = c_hi + c_lo in fp64, c_hi of 16 significant bits;  nch = -c_hi,  klo = -ln 2 * c_lo,  tmax = 16 (or -1: every element through fp64)
struct SwigluOaiAct {
  float nch, klo, alpha, tmax, limit;
};
enum { ACT_SILU = 0, ACT_OAI = 1, ACT_OAI_BIAS = 2 };   // activation of the GATED kernels (ACT)

struct QuantParams {
  const uint16_t* x;   // bf16, numel
  const uint16_t* h;   // bf16, R x R row-major
  uint8_t* out;        // packed e2m1, numel/2 (FMT e4m3 / e5m2: one byte per element, numel; FMT e2m3: four codes in three bytes, numel * 3 / 4)
  uint8_t* out_sf;     // e8m0 (MX, numel/32) or e4m3 (NV, numel/16), flat group order
  uint32_t* out_mask;  // MX quest-with-mask: one u32 per 32-group (may be null)
  const float* global_scale;  // NV only
  int64_t numel;
  int ntiles;          // ceil(numel / (max(R,32) * 32)): tiles of 32 rows x max(R,32) elements
  // BLK kernels only (fusedQuantize{Mx,Nv}Blocked): the scales go straight into the to_blocked() layout of the logical
  // (sf_rows, sf_cols) scale matrix -- sf_rows = numel / K, sf_cols = K / 32 (MX) or K / 16 (NV) -- padding zero-filled
  int sf_rows, sf_cols;
  // GATED kernels only (fusedSiluMulQuantize*): x is (rows, 2 * inter) -- gate | up halves of every row -- and the operand that is rotated and quantized is
  // act = silu(gate) * up, (rows, inter); numel counts act.  The plain kernels never read it.  (Sits in the struct's tail padding: no other field moves.)
  int inter = 0;
  // GATHER kernels only (fusedGatherQuantize*): the operand is xg = x[src_row] -- row m of the (numel / inter, inter) operand is row src_row[m] of x = (src_n, inter);
  // inter is the row length K here.  An index outside [0, src_n) stands for an all-zero row.  The plain and the gated kernels never read these.
  const int32_t* src_row = nullptr;
  int src_n = 0;
  // GSCALE kernels only (fused{Gather,SiluMul}QuantizeNvGrouped): global_scale points at E floats, one per expert, and offs (E) holds the grouped GEMMs' cumulative END
  // rows -- row m of the operand takes global_scale[quant_group_of_row(offs, E, m)].  No other kernel reads them.  (E sits in the tail padding; offs grows the struct.)
  int E = 0;
  const int32_t* offs = nullptr;
  // OAI kernels only (fusedSwigluOaiQuantizeMx, fusedSwigluOaiQuantizeMxf8): the gated layout, with act = swiglu_oai(gate, up) (swiglu_oai_mul8 below) in place of
  // silu(gate) * up.  With a bias (ACT == ACT_OAI_BIAS): bias (E, 2 * inter) bf16 in the same [gate | up] halves, row m of x takes bias[quant_group_of_row(offs, E, m)]; E == 1 never reads offs.
  const uint16_t* bias = nullptr;
  SwigluOaiAct oai = {};
};

// The expert that owns operand row m: g(m) = min(E - 1, #{ g : offs[g] <= m }) for non-decreasing offs -- the group the grouped GEMMs put the row in; rows at or past
// offs[E - 1] (the dropped slots) belong to expert E - 1.  An upper-bound search over offs[0, E - 1) with a trip count that depends on E alone (uniform over a wave):
// base + n <= E - 1 holds throughout, so every index read lies in [0, E - 2] and the result in [0, E - 1] WHATEVER offs holds (negative, huge, decreasing: some
// expert, no fault).  At most 11 reads for E = 1024.  ONE function for the two GSCALE kernels and the host (qutlass_amd_debug_group_of_row runs it on the CPU).
__host__ __device__ __forceinline__ int quant_group_of_row(const int32_t* offs, int E, int m) {
  int base = 0, n = E - 1;
  while (n > 1) {
    const int half = n >> 1;
    base = offs[base + half - 1] <= m ? base + half : base;
    n -= half;
  }
  return (n == 1 && offs[base] <= m) ? base + 1 : base;
}
constexpr int QUANT_MAX_E = 1024;   // experts per launch of the GSCALE kernels (the grouped GEMMs' GRP_MAX_E): the workgroup's copy of offs is 4 KiB of LDS
// (a function, so that only the kernels that call it -- the GSCALE ones -- get the allocation)
__device__ __forceinline__ int32_t* quant_offs_lds() {
  __shared__ int32_t offs_s[QUANT_MAX_E];
  return offs_s;
}

// Host side: what the two formats of the family differ in (capi.hip builds every check and the QuantParams fill from it)
struct QuantFormat {
  bool nv;               // the kernels' NV template argument; a global scale is required
  int group;             // elements per scale: e8m0 per 32 (MX), e4m3 per 16 (NV)
  int min_rot;           // rotation sizes: min_rot, ..., 64, 128 (powers of two)
  bool mask;             // a clip mask may be asked for (method quest, R = 32)
  const char* rots;      // that set as the messages spell it
  const char* row_unit;  // the blocked row-length message names its unit "the rotation size" for MX (the unit is R) and gives the bare number for NV (max(R, 32))
  bool fp8 = false;      // MXFP8: one code byte per element (e4m3 or e5m2, the entry's fmt), abs-max only, no clip mask; scales as MX
  bool fp6 = false;      // MXFP6 (with fp8: the same chains): e2m3 codes, four in three bytes; no fmt argument, flat scales only
  constexpr bool has_rot(int rot) const { return rot >= min_rot && rot <= 128 && (rot & (rot - 1)) == 0; }
};
constexpr QuantFormat kQuantMx{false, 32, 32, true, "32, 64, or 128", "the rotation size "};
constexpr QuantFormat kQuantNv{true, 16, 16, false, "16, 32, 64, or 128", ""};
constexpr QuantFormat kQuantMxf8{false, 32, 32, false, "32, 64, or 128", "the rotation size ", true};
constexpr QuantFormat kQuantMxf6{false, 32, 32, false, "32, 64, or 128", "the rotation size ", true, true};

// byte offset of scale (row, col) in the 128x4-tiled block-scale layout (qutlass/utils.py:60-64, :190-193); CB = ceil(cols / 4)
__device__ __forceinline__ uint32_t blocked_sf_offset(uint32_t row, uint32_t col, uint32_t CB) {
  return ((row >> 7) * CB + (col >> 2)) * 512u + (row & 31u) * 16u + ((row & 127u) >> 5) * 4u + (col & 3u);
}

// --- e2m1 encoders -------------------------------------------------------------------------------
// Software RTNE-satfinite encoder (semantics of PTX cvt.rn.satfinite.e2m1x2.f32; oracle:
// orc_e2m1_encode).  Uses the fp32 adder as the rounder: adding 2^22 / 2^23 / 2^24 rounds |t| to a
// multiple of 0.5 / 1 / 2 with ties-to-even, which is exactly the e2m1 grid in [0,2) / [2,4) / [4,6].
__device__ __forceinline__ uint32_t e2m1_encode_sw(float t) {
  const uint32_t sign = (__float_as_uint(t) >> 28) & 8u;
  float a = fminf(fabsf(t), 6.0f);          // NaN -> 6 (fminf returns the non-NaN operand)
  const bool ge2 = a >= 2.0f, ge4 = a >= 4.0f;
  const float magic = ge4 ? 16777216.0f : (ge2 ? 8388608.0f : 4194304.0f);
  const uint32_t k = __float_as_uint(a + magic) - __float_as_uint(magic);
  return sign | (k + (ge4 ? 4u : (ge2 ? 2u : 0u)));
}

// Hardware converter v_cvt_scalef32_pk_fp4_f32: two fp32 -> one byte, lo -> low nibble.  Enabled only after tools/probe verified
// it against the oracle on device (scale operand 1.0).  [r3] The scale operand DIVIDES by a power of two exactly, before the
// rounding: cvt(y, 2^-sh) == cvt(ldexp(y, sh), 1.0) on 220 000 pairs incl. every rounding tie of the e2m1 grid, saturating values
// and products in the fp32 denormal range (tests/native/cvt_scale_probe.hip, profiles/cvt_scale_probe_r3.txt) -- so a
// power-of-two block scale costs no instruction of its own.
template <int BYTE>
__device__ __forceinline__ uint32_t e2m1_pack2_hw(uint32_t old, float lo, float hi, float scale = 1.0f) {
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, lo, hi, scale, BYTE);
}

// [r5] NaN -> +inf in one instruction (v_min_f32 returns its non-NaN operand; every other value, +-inf included, passes unchanged).  The reference's convert,
// cvt.rn.satfinite.e2m1x2.f32, maps a NaN of EITHER sign to +6 = 0x7 (epilogue_quant.h:77-97; oracle orc_e2m1_encode); v_cvt_scalef32_pk_fp4_f32 keeps the NaN's
// sign (0x7 or 0xf) -- and the NaNs an MFMA rotation makes of a NaN / inf activation come out negative (tests/test_gpu_round5.py, tools/dbg_special_quant.py).
#ifndef QAMD_Q_NANFIX
#define QAMD_Q_NANFIX 1
#endif
__device__ __forceinline__ float nan_to_pinf(float v) {
#if QAMD_Q_NANFIX
  float r;
  asm("v_min_f32 %0, 0x7f800000, %1" : "=v"(r) : "v"(v));
  return r;
#else
  return v;
#endif
}

// 8 values -> one dword.  `scale` (a power of two; HWCVT only) divides the values inside the convert.  NANFIX: the forward quantizers' exact NaN code (above).
template <bool HWCVT, bool NANFIX = false>
__device__ __forceinline__ uint32_t e2m1_pack8(const float* t, float scale = 1.0f) {
  if (HWCVT) {
    uint32_t r = 0;
    if constexpr (NANFIX) {
      r = e2m1_pack2_hw<0>(r, nan_to_pinf(t[0]), nan_to_pinf(t[1]), scale);
      r = e2m1_pack2_hw<1>(r, nan_to_pinf(t[2]), nan_to_pinf(t[3]), scale);
      r = e2m1_pack2_hw<2>(r, nan_to_pinf(t[4]), nan_to_pinf(t[5]), scale);
      r = e2m1_pack2_hw<3>(r, nan_to_pinf(t[6]), nan_to_pinf(t[7]), scale);
      return r;
    }
    r = e2m1_pack2_hw<0>(r, t[0], t[1], scale);
    r = e2m1_pack2_hw<1>(r, t[2], t[3], scale);
    r = e2m1_pack2_hw<2>(r, t[4], t[5], scale);
    r = e2m1_pack2_hw<3>(r, t[6], t[7], scale);
    return r;
  } else {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r |= e2m1_encode_sw(t[i]) << (4 * i);
    return r;
  }
}

// Four fp32 -> four e4m3fn (FMT = QF_E4M3) or e5m2 (QF_E5M2) bytes, t[0] in the low byte: v_cvt_scalef32_pk_{fp8,bf8}_f32, round-to-nearest-even, NaN stays NaN.
// The converter's scale operand is left at 1.0 -- see the FP8 arm of the epilogue for why the block scale is applied by a multiply instead.
template <int FMT>
__device__ __forceinline__ uint32_t fp8_pack4(const float* t) {
  typedef short v2s_ __attribute__((ext_vector_type(2)));
  v2s_ w = {0, 0};
  if constexpr (FMT == QF_E4M3) {
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, t[0], t[1], 1.0f, false);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, t[2], t[3], 1.0f, true);
  } else {
    w = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(w, t[0], t[1], 1.0f, false);
    w = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(w, t[2], t[3], 1.0f, true);
  }
  return __builtin_bit_cast(uint32_t, w);
}

// t[0..N) = a[0..N) * s as N/2 v_pk_mul_f32 (4 cycles per wave for two products, the same issue cost as one v_mul_f32:
// tests/native/valu_probe.hip; the streaming quantisers are VALU-issue-bound at small rotation sizes)
typedef float v2f __attribute__((ext_vector_type(2)));
template <int N, typename V>
__device__ __forceinline__ void scale_pk(const V& a, int a0, float s, float* t) {
#pragma unroll
  for (int i = 0; i < N; i += 2) {
    const v2f r = v2f{a[a0 + i], a[a0 + i + 1]} * v2f{s, s};
    t[i] = r[0];
    t[i + 1] = r[1];
  }
}

// combine a per-lane partial with the partner lane l^32 (one v_permlane32_swap + one op)
__device__ __forceinline__ float xhalf_max(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_add(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ uint32_t xhalf_or(uint32_t v) {
  auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return r[0] | r[1];
}

// [r6] Quest sums of one group in the REFERENCE's order: one thread adds elements 0, 1, 2, ... in turn (epilogue_quant.h:521-528 MX, :1621-1628 NV; nvcc contracts
// `c_sum2 += c_val * c_val` into an fma).  The kernel's own order (a lane's values, then the partner half) gives sums that differ from those in the last bits -- which
// decides the SIGN of the variance of a (nearly) constant group, i.e. whether the reference takes its `var >= 0` arm (MX: scale 1.0 otherwise) or stores a NaN scale
// byte (NV).  Such groups (variance below 2^-10 of the mean square, NaN included; never on real activations) are re-summed here; NQ quads per lane, a lane holds
// elements 8 q + 4 half + e of the group (v_permlane32_swap of a value with itself leaves {half 0's, half 1's} in both lanes).
template <int NQ, typename V>
__device__ __forceinline__ void quest_sums_in_reference_order(const V& a, int a0, float& s1, float& s2) {
  s1 = 0.f;
  s2 = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    float lo[4], hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t b = __float_as_uint(a[a0 + 4 * q + e]);
      auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
      lo[e] = __uint_as_float(r[0]);
      hi[e] = __uint_as_float(r[1]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { s1 += lo[e]; s2 = fmaf(lo[e], lo[e], s2); }
#pragma unroll
    for (int e = 0; e < 4; ++e) { s1 += hi[e]; s2 = fmaf(hi[e], hi[e], s2); }
  }
}

// OCP e4m3fn encode of a non-negative finite fp32, RNE, saturating at 448 (oracle: orc_e4m3_encode).
__device__ __forceinline__ uint32_t e4m3_encode_pos(float a) {
  if (!(a < 448.0f)) return (a != a) ? 0x7Fu : 0x7Eu;
  // quantum 2^(max(e,-6)-3): add-magic rounding at that binade
  uint32_t u = __float_as_uint(a);
  int e = (int)(u >> 23) - 127;
  e = e < -6 ? -6 : e;
  const float magic = __uint_as_float((uint32_t)(e + 20 + 127) << 23);   // 2^(e+20): ulp = 2^(e-3)
  const float r = (a + magic) - magic;                                   // RNE to the e4m3 grid
  if (r < 0.015625f) return (uint32_t)(r * 512.0f);                      // subnormal: m * 2^-9
  const uint32_t ru = __float_as_uint(r);
  return (((ru >> 23) - 120u) << 3) | ((ru >> 20) & 7u);
}
__device__ __forceinline__ float e4m3_decode_pos(uint32_t b) {
  const uint32_t e = b >> 3, m = b & 7;
  if (b == 0x7Fu) return __uint_as_float(0x7fc00000u);   // [r5] the format's NaN (a NaN group statistic): `SF > 0` is then false and the group's multiplier 0, as in the reference
  return e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
}

// --- gated-MLP activation --------------------------------------------------------------------------
// act = bf16_rne(float(s) * float(u)), s = bf16_rne(g / (1 + exp(-g))): what a model that runs `silu(gate) * up` in bf16 computes.  s is the CORRECTLY rounded bf16 of
// silu(g): a mis-rounded s (fp32 arithmetic misses a bf16 tie about once in 2^11 values) is off by up to 2^-8 of its value, which can come out as TWO bf16 steps of
// act -- and would make the result depend on the accuracy of one chip's v_exp_f32.  So:
//   fast path  fp32.  exp(-g) = v_exp_f32(-g * c_hi) * (1 - ln 2 * c_lo * g) with log2 e = c_hi + c_lo, c_hi of 16 bits: g has 8, the product is exact, and the
//              rest (|ln 2 c_lo g| < 2^-13 for |g| <= 16) enters to first order.  v_exp_f32, v_rcp_f32: 1 ulp each; in all s is within 2^-21.2 of silu(g), 7 fp32 ulp.
//   slow path  the values whose fast result lies within 12 fp32 ulp of a bf16 tie (2^-11.4 of them), and g < -16, where a relative bound on exp no longer gives one
//              on s (and fp32's exp overflows from -88.7 on, where silu(g) is still a bf16 number; it rounds to -0 below about -97, as fp32's g / inf does): fp64, rounded to bf16 once.
// The product float(s) * float(u) is exact in fp32 (8 x 8 bits), so its one rounding is the definition's.
__device__ __forceinline__ float silu_f32(float g) {
  const float e0 = __builtin_amdgcn_exp2f(g * -1.44268798828125f);             // c_hi = 0x3FB8AA00: exact product
  const float e = fmaf(e0, g * -4.8884952e-06f, e0);                          // ln 2 * c_lo, c_lo = log2 e - c_hi = 7.0526077e-06
  return g * __builtin_amdgcn_rcpf(1.0f + e);
}
// fp64 -> bf16 bits, round-to-nearest-even in ONE rounding: through fp32, and where that lands exactly on a bf16 tie the fp64 value says which side it came from
__device__ __forceinline__ uint32_t f64_to_bf16_bits(double v) {
  const float f = (float)v;
  uint32_t b = __float_as_uint(f);
  if ((b & 0xffffu) == 0x8000u) {
    const double d = fabs(v) - fabs((double)f);
    b += d > 0.0 ? 1u : (d < 0.0 ? 0xffffffffu : 0u);
  }
  return (f != f) ? ((b >> 16) | 0x40u) : ((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ bool silu_needs_fp64(float g, float s) {
  return ((__float_as_uint(s) & 0xffffu) - (0x8000u - 12u) <= 24u) || g < -16.0f;
}
// 8 gate bf16 + 8 up bf16 (one 16-byte load each) -> 8 packed act bf16.  The ONE definition of the activation: silu_mul_bf16_kernel stores its result, the gated
// quantizers feed it to the rotation MFMA -- which is what makes fusedSiluMulQuantize* bit-equal to silu_and_mul followed by fusedQuantize*.
__device__ __forceinline__ v4i silu_mul8(const v4i g, const v4i u) {
  uint32_t sw[4], need = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t gw = (uint32_t)g[i];
    const float g0 = __uint_as_float(gw << 16), g1 = __uint_as_float(gw & 0xffff0000u);
    const float s0 = silu_f32(g0), s1 = silu_f32(g1);
    sw[i] = pack_bf16x2(s0, s1);
    need |= (silu_needs_fp64(g0, s0) ? 1u : 0u) << (2 * i) | (silu_needs_fp64(g1, s1) ? 1u : 0u) << (2 * i + 1);
  }
  if (__builtin_expect(need != 0, 0)) {
    // one copy of the fp64 code: a loop over the eight positions, taken by the lanes that flagged that position
#pragma nounroll
    for (int i = 0; i < 8; ++i) {
      if (need & (1u << i)) {
        const int w = i >> 1;
        const uint32_t gw = (uint32_t)(w == 0 ? g[0] : w == 1 ? g[1] : w == 2 ? g[2] : g[3]);
        const double gd = (double)__uint_as_float((i & 1) ? (gw & 0xffff0000u) : (gw << 16));
        const uint32_t r = f64_to_bf16_bits(gd / (1.0 + exp(-gd)));
        const uint32_t keep = (i & 1) ? 0x0000ffffu : 0xffff0000u, val = (i & 1) ? (r << 16) : r;
#pragma unroll
        for (int k = 0; k < 4; ++k) sw[k] = (k == w) ? ((sw[k] & keep) | val) : sw[k];
      }
    }
  }
  v4i r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t uw = (uint32_t)u[i];
    r[i] = (int)pack_bf16x2(__uint_as_float(sw[i] << 16) * __uint_as_float(uw << 16), __uint_as_float(sw[i] & 0xffff0000u) * __uint_as_float(uw & 0xffff0000u));
  }
  return r;
}

// --- clamped SwiGLU (gpt-oss) ------------------------------------------------------------------------
// Per element, g, u, bg, bu bf16, alpha an fp32 value > 0, limit a bf16 value > 0:
//   g1 = bias ? bf16_rne(float(g) + float(bg)) : g,  u1 likewise          (one fp32 add, then RNE: a bf16 tensor add)
//   gc = min(g1, limit),  uc = min(max(u1, -limit), limit)                 (exact)
//   s  = the CORRECTLY rounded bf16 of the real number gc / (1 + exp(-alpha * gc))   (the product alpha * gc not rounded)
//   act = bf16_rne(float(s) * (float(uc) + 1.0f))                          (one fp32 add, one fp32 multiply, no fma, then RNE)
// s by silu's mechanism, the error analysis redone for a runtime alpha.  With T = alpha * log2 e * gc:
//   fast path  |fl(alpha * gc)| <= 16, i.e. |T| <= 23.1 -- silu's own domain.  The host splits alpha * log2 e = c_hi + c_lo in fp64 with c_hi of 16 significant
//              bits: gc has 8, so c_hi * gc is an exact fp32 product whatever alpha is, and |c_lo| <= 2^-16 c.  exp(-alpha gc) = 2^(-c_hi gc) * exp(-x),
//              x = ln 2 c_lo gc, |x| <= ln 2 * 2^-16 * 23.1 = 2^-12.  Relative errors: v_exp_f32 2^-23; exp(-x) against 1 - x at most x^2 / 2 = 2^-25 (silu's
//              fixed 15-bit c_hi happens to leave 2^-27); the rounding of klo and of gc * klo 2^-35; the fma 2^-24: e within 2^-22.19.  1 + e: that times
//              e / (1 + e) <= 1, plus its rounding 2^-24: 2^-21.85.  v_rcp_f32 2^-23, the last product 2^-24: s within 3.72 * 2^-23 = 2^-21.1 of the true
//              value, at most 7.5 fp32 ulp (silu: 7).  The tie window is widened from silu's 12 to 16 fp32 ulp either side.
//   slow path  results within 16 fp32 ulp of a bf16 tie (2^-11 of the values), and |fl(alpha * gc)| > 16 or NaN -- the large-negative threshold is -16 / alpha,
//              and the positive side joins it because limit and alpha are the caller's (gc * klo must not overflow against e0 = 0): fp64,
//              gd / (1 + exp(-(double)alpha * gd)) with the product exact, rounded to bf16 once.  tmax = -1 (the host: alpha * log2 e outside
//              [2^-100, 2^100], where c_hi or klo would leave fp32's normal range) sends every element here.
// For |gc| < 2^-120 the true value lies within 2^-130 (relative) of a tie between bf16 subnormals, which fp64 does not resolve either: s is then within one
// bf16 step.  A zero gate gives s = gate (signed), so zero gate, up and bias give +0 * 1 = +0.  NaN / inf: unspecified bytes for their own element.
__device__ __forceinline__ float swiglu_oai_f32(float g, const SwigluOaiAct& a) {
  const float e0 = __builtin_amdgcn_exp2f(g * a.nch);   // exact product
  const float e = fmaf(e0, g * a.klo, e0);
  return g * __builtin_amdgcn_rcpf(1.0f + e);
}
__device__ __forceinline__ bool swiglu_oai_needs_fp64(float g, float s, const SwigluOaiAct& a) {
  return ((__float_as_uint(s) & 0xffffu) - (0x8000u - 16u) <= 32u) || !(fabsf(g * a.alpha) <= a.tmax);
}
// 8 gate + 8 up bf16 (one 16-byte load each) [+ 8 + 8 bias bf16 of the row's expert] -> 8 packed act bf16.  The ONE definition of the activation, as silu_mul8 is:
// swiglu_oai_mul_bf16_kernel stores its result, the OAI arm of the quantizer feeds it to the rotation MFMA.
template <bool BIAS>
__device__ __forceinline__ v4i swiglu_oai_mul8(const v4i g, const v4i u, const v4i bg, const v4i bu, const SwigluOaiAct& a) {
#pragma clang fp contract(off)
  uint32_t gc[4], sw[4], need = 0;
  float up1[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t gw = (uint32_t)g[i], uw = (uint32_t)u[i];
    if constexpr (BIAS) {
      const uint32_t bgw = (uint32_t)bg[i], buw = (uint32_t)bu[i];
      gw = pack_bf16x2(__uint_as_float(gw << 16) + __uint_as_float(bgw << 16), __uint_as_float(gw & 0xffff0000u) + __uint_as_float(bgw & 0xffff0000u));
      uw = pack_bf16x2(__uint_as_float(uw << 16) + __uint_as_float(buw << 16), __uint_as_float(uw & 0xffff0000u) + __uint_as_float(buw & 0xffff0000u));
    }
    // the clamps as compare + select: the values stay the bf16 values they were, subnormals included
    const float gl = __uint_as_float(gw << 16), gh = __uint_as_float(gw & 0xffff0000u), ul = __uint_as_float(uw << 16), uh = __uint_as_float(uw & 0xffff0000u);
    const float g0 = gl > a.limit ? a.limit : gl, g1 = gh > a.limit ? a.limit : gh;
    gc[i] = (__float_as_uint(g0) >> 16) | (__float_as_uint(g1) & 0xffff0000u);
    up1[2 * i] = (ul < -a.limit ? -a.limit : (ul > a.limit ? a.limit : ul)) + 1.0f;
    up1[2 * i + 1] = (uh < -a.limit ? -a.limit : (uh > a.limit ? a.limit : uh)) + 1.0f;
    const float s0 = swiglu_oai_f32(g0, a), s1 = swiglu_oai_f32(g1, a);
    sw[i] = pack_bf16x2(s0, s1);
    need |= (swiglu_oai_needs_fp64(g0, s0, a) ? 1u : 0u) << (2 * i) | (swiglu_oai_needs_fp64(g1, s1, a) ? 1u : 0u) << (2 * i + 1);
  }
  if (__builtin_expect(need != 0, 0)) {
    // one copy of the fp64 code: a loop over the eight positions, taken by the lanes that flagged that position (as in silu_mul8)
#pragma nounroll
    for (int i = 0; i < 8; ++i) {
      if (need & (1u << i)) {
        const int w = i >> 1;
        const uint32_t gw = w == 0 ? gc[0] : w == 1 ? gc[1] : w == 2 ? gc[2] : gc[3];
        const double gd = (double)__uint_as_float((i & 1) ? (gw & 0xffff0000u) : (gw << 16));
        const uint32_t r = f64_to_bf16_bits(gd / (1.0 + exp(-(double)a.alpha * gd)));
        const uint32_t keep = (i & 1) ? 0x0000ffffu : 0xffff0000u, val = (i & 1) ? (r << 16) : r;
#pragma unroll
        for (int k = 0; k < 4; ++k) sw[k] = (k == w) ? ((sw[k] & keep) | val) : sw[k];
      }
    }
  }
  v4i r;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = (int)pack_bf16x2(__uint_as_float(sw[i] << 16) * up1[2 * i], __uint_as_float(sw[i] & 0xffff0000u) * up1[2 * i + 1]);
  return r;
}

// -------------------------------------------------------------------------------------------------
// Kernel.  One wave owns one 32-row tile at a time (grid-stride over tiles).
//   R      : rotation size (MX: 32/64/128, NV: 16/32/64/128)
//   NV     : false = MX (e8m0 per 32), true = NV (e4m3 per 16)
//   METHOD : METHOD_QUEST / METHOD_ABSMAX
//   MASK   : MX quest only: also emit the clip mask
//   HWCVT  : use v_cvt_scalef32_pk_fp4_f32 for the final RTNE
//   BLK    : scale bytes are written in the to_blocked() layout (GEMM-ready: no separate swizzle launch) instead of flat
//   GATED  : the operand is act = silu(gate) * up of an x that holds (rows, 2 I): the tile's loads fetch gate and up (two 16-byte loads where the plain kernel has
//            one) and silu_mul8 turns them into the bf16 the plain kernel would have loaded; everything after that is the plain kernel.  The input is addressed with
//            32-bit offsets from one descriptor: x must stay below 2 GiB (rows * I < 2^29; the host checks).
//   GATHER : the operand is xg = x[src_row], (M, K): RP-row (m, c) of a tile is read from row src_row[m] of x = (T, K) -- again only the tile loads' address differs, the
//            rest is the plain kernel, so the result is fusedQuantize*(x.index_select(0, src_row)) byte for byte.  A tile spans at most 32 logical rows; lane l of the
//            wave fetches src_row[first row of the tile + (l & 31)] and every chunk load picks its row's index out of that register with a cross-lane read
//            (ds_bpermute: no LDS memory, one per chunk load).  The x loads depend on the indices, so the indices run one tile ahead of the x loads, which
//            run one tile ahead of the MFMAs: gather_loads(t) issues tile t's x loads from the indices fetched a tile earlier, then tile t + nwaves' index load.  The
//            first tile's index load goes out before H's loads and its x loads before H's LDS writes.  An index is compared with T before any offset is formed from
//            it; out of range (or an RP-row past the end) the offset is 2^31, off the descriptor (x stays below 2 GiB; the host checks): the load returns zeros.
//   GSCALE : (NV abs-max, flat scales, on top of GATHER or of GATED) one global scale per EXPERT: logical row m of the operand is quantized with
//            global_scale[quant_group_of_row(offs, E, m)].  Only `gscale` changes in the epilogue -- from a wave-uniform scalar to the value of the logical row the
//            lane's RP-row belongs to; the three operations that use it (gscale * (m / 6), rcp(gscale), rcp(sf * ...)) are the same operations in the same order, so
//            a row's bytes are those of the single-scale kernel called with its expert's scale, by construction.  The lookup stays off the critical path and off the
//            vector-memory queue: the workgroup copies offs into LDS once (loads issued with the first tile's, written with H), a tile spans at most 32 logical
//            rows, lane l searches the LDS copy for row (first row of the tile) + (l & 31) and loads that expert's scale (index clamped to [0, E)) -- ONE TILE AHEAD,
//            right after the next tile's x loads, so the one global load has that tile's wait and this tile's MFMAs and epilogue to land -- and the epilogue lane
//            picks its own row's value with a cross-lane read (ds_bpermute by (rem + row) / rpr, the split gather_off does).  Two registers: this tile's values and
//            the next tile's.  There is no METHOD_QUEST instantiation: the NV Quest arm never reads gscale, so the grouped entries launch the single-scale Quest kernel.
//   ACT    : (GATED, MX e2m1 or -- abs-max -- e4m3, flat scales) ACT_OAI / ACT_OAI_BIAS: the activation is the clamped SwiGLU, swiglu_oai_mul8, in place of silu_mul8 --
//            nothing else changes.
//            ACT_OAI_BIAS adds the gate/up bias of the row's expert: a tile's loads fetch, next to gate and up, the two bias chunks at the same columns of row
//            quant_group_of_row(offs, E, logical row) of bias = (E, 2 I), through a descriptor of their own (bias stays below 2 GiB; the host checks; the expert is
//            clamped to [0, E), so malformed offs cannot address outside it).  The lookup is GSCALE's: offs in LDS, lane l searches for logical row (first row of
//            the tile) + (l & 31), a chunk load picks its row's expert with a cross-lane read -- and it runs AHEAD of the loads that depend on it, as GATHER's indices
//            do: the experts of tile t + nwaves are looked up right after the bias loads of tile t went out (the first tile's after the barrier that publishes
//            offs).  The bias loads themselves go out at the top of the tile that uses them, behind that tile's gate / up loads, which have been in flight for a
//            whole tile: they are L2 hits (every row of an expert shares them), and holding a tile's bias chunks in registers across a tile as well (24-34 more
//            VGPRs, a wave per SIMD) measured 2-6 % slower.
//   FMT    : QF_E2M1 (the default: everything above) or QF_E4M3 / QF_E5M2 -- the MXFP8 quantizers (MX abs-max without a clip mask; plain, BLK, GATED or GATHER):
//            everything up to and including the MFMAs is the MX kernel, the epilogue is the FP8 arm below (one byte per element, a 32-byte run per group).  With ACT_OAI /
//            ACT_OAI_BIAS (e4m3, flat scales, R = 32 / 64) the two meet: the activation arm ends with the bf16 tile in xnext, the FP8 arm starts after the MFMAs and
//            reads only acc, the tile's group index and the two output pointers, none of which the activation arm touches -- fusedSwigluOaiQuantizeMxf8.
// -------------------------------------------------------------------------------------------------
// The kernel's body as a device function of (workgroup index, workgroup count): fused_quantize_kernel below is its plain launch; [r6] the one-launch decode layer
// (gemm_mx_os.hip.h gemm_mx_os16_fq_kernel) runs it on its first few workgroups.  PAD = false: the zero padding of the blocked scale layout is left out (a reader that
// only looks at the rows it wrote).
template <int R, bool NV, int METHOD, bool MASK, bool HWCVT, bool BLK = false, bool PAD = true, bool GATED = false, bool GATHER = false, bool GSCALE = false,
          int FMT = QF_E2M1, int ACT = ACT_SILU>
__device__ __forceinline__ void fused_quantize_body(const QuantParams& p, const int bid, const int nblk) {
  constexpr int RP = (R < 32) ? 32 : R;         // rotation padded to one MFMA j-tile (R=16: block-diag)
  constexpr int KC = RP / 16;                   // 16-wide k chunks per row
  constexpr int JT = RP / 32;                   // 32-wide j tiles per row = MX groups per row
  // [r4] R >= 64: H sits in LDS as it is in memory (row k, column j; staged with 16-byte copies) and the MFMA fragments come out of it with
  // transposing reads (ds_read_b64_tr_b16, the addressing of quartet_bwd.hip.h) -- the transposed image cost every thread R*R/256 two-byte loads
  // and as many two-byte LDS writes before the first tile could be rotated (R = 128: ~2 us of a 10 us kernel at 4096^2).  Row stride = 16 or 48
  // dwords (mod 64) keeps the transposing reads of a half wave on 64 different banks.
  constexpr bool HTR = RP >= 64;
  constexpr int HROW = HTR ? RP * 2 + 64 : RP * 2 + 16;   // H (HTR) / H^T row stride in LDS (bytes)
  __shared__ __attribute__((aligned(16))) char hT[RP * HROW];
  // R >= 64: a tile's rows are 128 / 256 bytes apart, and a load in MFMA layout (lane = row, 16 bytes) touches 32 lines
  // for 32 bytes each -- every line four to eight times over the tile's loads, from an L1 that the other waves' tiles
  // have long flushed (R = 128: 11.6 us for 4096^2 against 6.9 us at R = 32).  Those sizes load their tile as ONE
  // contiguous run (64 lanes x 16 bytes = 1 KiB per instruction), stage it in a wave-private LDS area and read the MFMA
  // fragments from there.
  constexpr bool STAGED = RP >= 64;
  constexpr int XROW = RP * 2 + 16;              // staged row stride (bytes)
  __shared__ __attribute__((aligned(16))) char xs_all[STAGED ? 4 * 32 * XROW : 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
  const int row = lane & 31, half = lane >> 5;

  // x as rows of RP elements (for R = 16 two rotation rows share one 32-element "row")
  const int64_t ngroups = p.numel / (NV ? 16 : 32);
  static_assert(!(GATED && GATHER) && !(GATHER && (BLK || MASK)), "the gathering form: plain operand, flat scales, no clip mask");
  static_assert(FMT == QF_E2M1 || ((FMT == QF_E4M3 || FMT == QF_E5M2 || FMT == QF_E2M3) && !NV && METHOD == METHOD_ABSMAX && !MASK && !GSCALE && R >= 32),
                "the MXFP8 / MXFP6 arms: MX scales (so no R = 16), abs-max, no clip mask");
  static_assert(FMT != QF_E2M3 || (!BLK && !GATED), "the MXFP6 arm: plain or gathering, flat scales");
  static_assert(!GSCALE || (NV && METHOD == METHOD_ABSMAX && !BLK && !MASK && (GATED || GATHER)), "per-expert global scales: NV abs-max, flat scales, gathering or gated");
  static_assert(ACT == ACT_SILU || (GATED && !NV && !BLK && !MASK && !GSCALE && (FMT == QF_E2M1 || FMT == QF_E4M3) && R >= 32 && R <= 64),
                "the clamped SwiGLU: gated MX e2m1 or e4m3, flat scales, R = 32 / 64");
  constexpr bool OAIB = ACT == ACT_OAI_BIAS;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, GATHER ? (uint32_t)p.src_n * (uint32_t)p.inter * 2u : (uint32_t)(p.numel * (GATED ? 4 : 2)));

  const int wave_global = bid * 4 + wave, nwaves = nblk * 4;
  v4i xnext[RP / 16];
  v4i unext[GATED ? RP / 16 : 1];   // GATED: xnext holds the gate chunks, unext the up chunks of the same elements
  v4i bgnext[OAIB ? RP / 16 : 1], bunext[OAIB ? RP / 16 : 1];   // ACT_OAI_BIAS: the bias chunks that go with them (loaded at the top of the tile that uses them)
  // per-lane byte offset inside a tile and the step between a lane's loads: MFMA layout (row, half; 32 bytes apart) or,
  // staged, chunk lane + 64 i of the tile's contiguous 32 * RP * 2 bytes
  const int lane_off = STAGED ? lane * 16 : row * RP * 2 + half * 16;
  constexpr int LSTEP = STAGED ? 1024 : 32;
  char* xs = xs_all + (STAGED ? wave * 32 * XROW : 0);
  // GATED: the act tile is the plain kernel's tile -- 32 "rows" of RP elements, contiguous in act -- but its RP-element rows sit 2 I elements apart in x where
  // they belong to different logical rows.  (g_row, g_rem) = logical row and RP-row within it of the first RP-row of the NEXT tile this wave loads: wave-uniform,
  // one division here and a carry-propagating add per tile.  A lane's chunk is RP-row `lrow` of the tile (the MFMA layout: lane & 31; staged: chunk / CPR, so that
  // consecutive lanes walk along a row -- whole lines -- before stepping to the next): x = g_rem + lrow < I / RP + 32 is split into (rows to carry, RP-row) with a
  // reciprocal multiply and a fix-up of one either way.
  uint32_t g_row = 0, g_rem = 0, g_qstep = 0, g_rstep = 0, g_rpr = 1, g_nrows = 0;
  float g_rc = 1.0f;
  // GSCALE: a second walk over the same tiles, (s_row, s_rem) = the tile whose scales are looked up next; n_rem = the rem of the tile gs_next belongs to
  // (ACT_OAI_BIAS: the same walk for the experts, e_next = the expert of logical row (first row of that tile) + (lane & 31))
  uint32_t s_row = 0, s_rem = 0, n_rem = 0;
  float gs_next = 1.0f;
  int e_next = 0;
  if constexpr (GATED || GATHER) {
    g_rpr = (uint32_t)p.inter / RP;
    g_rc = __builtin_amdgcn_rcpf((float)g_rpr);
    g_nrows = (uint32_t)(p.numel / RP);
    const uint32_t r0 = (uint32_t)wave_global * 32u, step = (uint32_t)nwaves * 32u;
    g_row = r0 / g_rpr;
    g_rem = r0 - g_row * g_rpr;
    g_qstep = step / g_rpr;
    g_rstep = step - g_qstep * g_rpr;
    if constexpr (GSCALE || OAIB) { s_row = g_row; s_rem = g_rem; }
  }
  // byte offset of the gate chunk (RP-row lrow of the tile at (g_row, g_rem), byte cb of that RP-row); up sits 2 I bytes further.  RP-rows past the end of act
  // (the last tile's tail, tiles past the end) get an offset off the descriptor: they read 0, as in the plain kernel.
  auto gated_off = [&](const int t, const uint32_t lrow, const uint32_t cb) -> int {
    const uint32_t x = g_rem + lrow;
    uint32_t q = (uint32_t)((float)x * g_rc);
    int32_t r = (int32_t)(x - q * g_rpr);
    if (r < 0) { q -= 1; r += (int32_t)g_rpr; }
    if (r >= (int32_t)g_rpr) { q += 1; r -= (int32_t)g_rpr; }
    const uint32_t off = (g_row + q) * ((uint32_t)p.inter * 4u) + (uint32_t)r * (RP * 2u) + cb;
    return ((uint32_t)t * 32u + lrow < g_nrows) ? (int)off : (int)0xfffffff0u;
  };
  auto gated_loads = [&](const int t) {   // issue tile t's loads (the tile (g_row, g_rem) stands at), then advance to this wave's next tile
    if constexpr (STAGED) {
      constexpr int CPR = RP / 8;
#pragma unroll
      for (int i = 0; i < RP / 16; ++i) {
        const int q = i * 64 + lane;
        const int off = gated_off(t, (uint32_t)(q / CPR), (uint32_t)(q % CPR) * 16u);
        xnext[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0);
        unext[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, off, p.inter * 2, 0);
      }
    } else {
      const int off = gated_off(t, (uint32_t)row, (uint32_t)half * 16u);
#pragma unroll
      for (int kc = 0; kc < RP / 16; ++kc) {
        xnext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, off + kc * 32, 0, 0);
        unext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, off + kc * 32, p.inter * 2, 0);
      }
    }
    g_rem += g_rstep;
    const uint32_t carry = g_rem >= g_rpr ? 1u : 0u;
    g_rem -= carry ? g_rpr : 0u;
    g_row += g_qstep + carry;
  };
  // GATHER: the same walk over (g_row, g_rem); gidx = src_row[g_row + (lane & 31)] of the tile the walk stands at (rows past the end of src_row read 0: only RP-rows
  // past the end of the operand name them, and those get the off-descriptor offset)
  const __amdgpu_buffer_rsrc_t ri = make_rsrc(GATHER ? (const void*)p.src_row : (const void*)p.x, GATHER ? (uint32_t)(p.numel / p.inter) * 4u : 0u);
  int gidx = 0;
  auto gather_index_load = [&]() { gidx = __builtin_amdgcn_raw_buffer_load_b32(ri, (int)((g_row + (uint32_t)row) * 4u), 0, 0); };
  auto gather_off = [&](const int t, const uint32_t lrow, const uint32_t cb) -> int {
    const uint32_t x = g_rem + lrow;
    uint32_t q = (uint32_t)((float)x * g_rc);
    int32_t r = (int32_t)(x - q * g_rpr);
    if (r < 0) { q -= 1; r += (int32_t)g_rpr; }
    if (r >= (int32_t)g_rpr) { q += 1; r -= (int32_t)g_rpr; }
    const uint32_t idx = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(q * 4u), gidx);   // q <= lrow <= 31: the lane that fetched src_row[g_row + q]
    const bool ok = idx < (uint32_t)p.src_n && (uint32_t)t * 32u + lrow < g_nrows;       // the range check comes first: no offset is formed from a bad index
    return ok ? (int)(idx * ((uint32_t)p.inter * 2u) + (uint32_t)r * (RP * 2u) + cb) : (int)0x80000000u;
  };
  auto gather_loads = [&](const int t) {   // tile t's x loads (gidx holds its indices), advance, then the index load of this wave's next tile
    if constexpr (STAGED) {
      constexpr int CPR = RP / 8;
#pragma unroll
      for (int i = 0; i < RP / 16; ++i) {
        const int q = i * 64 + lane;
        xnext[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, gather_off(t, (uint32_t)(q / CPR), (uint32_t)(q % CPR) * 16u), 0, 0);
      }
    } else {
      const int off = gather_off(t, (uint32_t)row, (uint32_t)half * 16u);
#pragma unroll
      for (int kc = 0; kc < RP / 16; ++kc) xnext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, off + kc * 32, 0, 0);
    }
    g_rem += g_rstep;
    const uint32_t carry = g_rem >= g_rpr ? 1u : 0u;
    g_rem -= carry ? g_rpr : 0u;
    g_row += g_qstep + carry;
    gather_index_load();
  };
  if constexpr (GATHER) {
    gather_index_load();        // the x loads that depend on it go out between H's loads and H's LDS writes, below
  } else if constexpr (GATED) {
    gated_loads(wave_global);   // (before H is staged, as below)
  } else {   // [r2] the first tile's loads go out BEFORE H is staged: the two memory round trips overlap (4096^2 cold: 9.03 -> 8.46 us at
      // R = 32, 10.08 -> 9.31 at R = 64, 13.18 -> 12.54 at R = 128; profiles/ab_stream_ops_r2.txt)
    const int xoff0 = (wave_global < p.ntiles) ? (int)((int64_t)wave_global * 32 * RP * 2) + lane_off : 0x7f000000;
#pragma unroll
    for (int kc = 0; kc < RP / 16; ++kc) xnext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, xoff0 + kc * LSTEP, 0, 0);
  }
  // GSCALE: this thread's share of offs for the workgroup's LDS copy (entry tid + 256 i; the index is clamped to [0, E)), in flight with the first tile's loads
  int32_t ov[(GSCALE || OAIB) ? QUANT_MAX_E / 256 : 1];
  if constexpr (GSCALE) {
#pragma unroll
    for (int i = 0; i < QUANT_MAX_E / 256; ++i) {
      const int idx = i * 256 + tid;
      if (i * 256 < p.E) ov[i] = p.offs[idx < p.E ? idx : p.E - 1];
    }
  }
  if constexpr (OAIB) {   // (one expert: the search reads nothing, and offs may be null)
#pragma unroll
    for (int i = 0; i < QUANT_MAX_E / 256; ++i) {
      const int idx = i * 256 + tid;
      if (i * 256 < p.E && p.E > 1) ov[i] = p.offs[idx < p.E ? idx : p.E - 1];
    }
  }
  const float gscale = (NV && !GSCALE) ? *p.global_scale : 1.0f;
  const uint32_t sfCB = BLK ? ((uint32_t)p.sf_cols + 3u) >> 2 : 0u;
  if (BLK && PAD) {
    // zero padding of the blocked layout (rows up to a multiple of 128, columns up to a multiple of 4), as to_blocked writes it
    const uint32_t prow = ((uint32_t)p.sf_rows + 127u) & ~127u, pcol = sfCB * 4u;
    const uint32_t n1 = (prow - (uint32_t)p.sf_rows) * pcol, cpad = pcol - (uint32_t)p.sf_cols, n2 = (uint32_t)p.sf_rows * cpad;
    // padding rows: one dword (the four columns of a column tile) per store; padding columns of real rows: bytes
    const uint32_t nd = n1 >> 2;
    for (uint32_t i = (uint32_t)bid * 256u + tid; i < nd + n2; i += (uint32_t)nblk * 256u) {
      if (i < nd) {
        const uint32_t r = (uint32_t)p.sf_rows + i / sfCB, cb = i % sfCB;
        *(uint32_t*)(p.out_sf + blocked_sf_offset(r, 4u * cb, sfCB)) = 0u;
      } else {
        const uint32_t j = i - nd, r = j / cpad, c = (uint32_t)p.sf_cols + j % cpad;
        p.out_sf[blocked_sf_offset(r, c, sfCB)] = 0;
      }
    }
  }

  // ---- H^T image in LDS: hT[j][k] = h[k][j]; R = 16 becomes blockdiag(h, h) so that one 32-wide
  //      MFMA tile rotates two adjacent 16-element rows at once
  if (R < 32) {
    // [r4] as below: all four loads of a thread before the first LDS write (the conditional load -> write loop made four trips to memory one after
    // the other: NV R = 16 paid ~3 us more than MX R = 32 per launch -- 4096^2 cold 11.0 against 8.5 us for the same bytes)
    constexpr int NE = RP * RP / 256;
    uint16_t hv[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int idx = i * 256 + tid, k = idx / RP, j = idx % RP;
      hv[i] = p.h[(k & 15) * R + (j & 15)];                      // (always in range: R x R entries)
    }
    if constexpr (GATHER) gather_loads(wave_global);
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int idx = i * 256 + tid, k = idx / RP, j = idx % RP;
      *(uint16_t*)(hT + j * HROW + k * 2) = ((k >> 4) == (j >> 4)) ? hv[i] : (uint16_t)0;
    }
  } else {
    // ALL loads of a thread issued before the first LDS write (with load -> write per element a thread of the R = 128
    // kernel made its 64 trips to memory one after the other: 12.0 us for 4096^2 against 7.7 us at R = 32, and 7.8 us for a
    // 16-row input).  Consecutive lanes take consecutive j: 2-byte loads coalesce to whole lines, and the transposed
    // writes hT[j][k] land HROW = 2 RP + 16 bytes apart, 16 distinct banks per 16 lanes.  (16-byte loads with 8
    // transposed 2-byte writes each were tried: the writes of a wave then fall on 2 banks, 15.7 us.)
    if constexpr (HTR) {
      constexpr int NCH = RP * RP / 8 / 256, CPRH = RP / 8;          // 16-byte chunks per thread, chunks per row of h
      v4i hc[NCH];
#pragma unroll
      for (int i = 0; i < NCH; ++i) hc[i] = *(const v4i*)(p.h + (i * 256 + tid) * 8);
      if constexpr (GATHER) gather_loads(wave_global);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = i * 256 + tid;
        *(v4i*)(hT + (c / CPRH) * HROW + (c % CPRH) * 16) = hc[i];
      }
    } else {
      constexpr int NE = RP * RP / 256;
      uint16_t hv[NE];
#pragma unroll
      for (int i = 0; i < NE; ++i) hv[i] = p.h[i * 256 + tid];           // idx = i * 256 + tid = k * RP + j, R == RP here
      if constexpr (GATHER) gather_loads(wave_global);
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int idx = i * 256 + tid, k = idx / RP, j = idx % RP;
        *(uint16_t*)(hT + j * HROW + k * 2) = hv[i];
      }
    }
  }
  if constexpr (GSCALE) {
    int32_t* so = quant_offs_lds();
#pragma unroll
    for (int i = 0; i < QUANT_MAX_E / 256; ++i)
      if (i * 256 < p.E) so[i * 256 + tid] = ov[i];
  }
  if constexpr (OAIB) {
    int32_t* so = quant_offs_lds();
#pragma unroll
    for (int i = 0; i < QUANT_MAX_E / 256; ++i)
      if (i * 256 < p.E && p.E > 1) so[i * 256 + tid] = ov[i];
  }
  __syncthreads();
  // GSCALE: gs_next = the scale of logical row s_row + (lane & 31) of the tile the second walk stands at, then that walk's step.  The search reads the LDS copy of
  // offs; its result lies in [0, E) whatever offs holds, and the one global load is clamped to that range once more.
  auto gscale_lookup = [&]() {
    if constexpr (GSCALE) {
      const int g = quant_group_of_row(quant_offs_lds(), p.E, (int)(s_row + (uint32_t)row));
      gs_next = p.global_scale[g < 0 ? 0 : (g < p.E ? g : p.E - 1)];
      n_rem = s_rem;
      s_rem += g_rstep;
      const uint32_t carry = s_rem >= g_rpr ? 1u : 0u;
      s_rem -= carry ? g_rpr : 0u;
      s_row += g_qstep + carry;
    }
  };
  gscale_lookup();   // the first tile's
  // ACT_OAI_BIAS: oai_lookup() = e_next for the tile the second walk stands at (its rem in n_rem), then that walk's step; oai_bias_loads() = the bias loads of the tile
  // e_next belongs to (issued at the top of that tile): the chunk mapping of gated_loads, the row's expert picked across lanes as GSCALE picks its scale, then the
  // lookup for this wave's next tile.
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(OAIB ? (const void*)p.bias : (const void*)p.x, OAIB ? (uint32_t)p.E * (uint32_t)p.inter * 4u : 0u);
  auto oai_lookup = [&]() {
    if constexpr (OAIB) {
      const int g = quant_group_of_row(quant_offs_lds(), p.E, (int)(s_row + (uint32_t)row));
      e_next = g < 0 ? 0 : (g < p.E ? g : p.E - 1);
      n_rem = s_rem;
      s_rem += g_rstep;
      const uint32_t carry = s_rem >= g_rpr ? 1u : 0u;
      s_rem -= carry ? g_rpr : 0u;
      s_row += g_qstep + carry;
    }
  };
  auto oai_bias_off = [&](const uint32_t lrow, const uint32_t cb) -> int {
    const uint32_t x = n_rem + lrow;
    uint32_t q = (uint32_t)((float)x * g_rc);
    int32_t r = (int32_t)(x - q * g_rpr);
    if (r < 0) { q -= 1; r += (int32_t)g_rpr; }
    if (r >= (int32_t)g_rpr) { q += 1; r -= (int32_t)g_rpr; }
    const uint32_t e = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(q * 4u), e_next);   // q <= lrow <= 31: the lane that looked that row up; e in [0, E)
    return (int)(e * ((uint32_t)p.inter * 4u) + (uint32_t)r * (RP * 2u) + cb);
  };
  auto oai_bias_loads = [&]() {
    if constexpr (OAIB) {
      if constexpr (STAGED) {
        constexpr int CPR = RP / 8;
#pragma unroll
        for (int i = 0; i < RP / 16; ++i) {
          const int q = i * 64 + lane;
          const int off = oai_bias_off((uint32_t)(q / CPR), (uint32_t)(q % CPR) * 16u);
          bgnext[i] = __builtin_amdgcn_raw_buffer_load_b128(rb, off, 0, 0);
          bunext[i] = __builtin_amdgcn_raw_buffer_load_b128(rb, off, p.inter * 2, 0);
        }
      } else {
        const int off = oai_bias_off((uint32_t)row, (uint32_t)half * 16u);
#pragma unroll
        for (int kc = 0; kc < RP / 16; ++kc) {
          bgnext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rb, off + kc * 32, 0, 0);
          bunext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rb, off + kc * 32, p.inter * 2, 0);
        }
      }
      oai_lookup();
    }
  };
  oai_lookup();   // the first tile's experts

  // BLK: (sf_row, sf_rem) = this lane's RP-element row r_abs = tile * 32 + row as (logical row, RP-row within it); one division
  // here, then a carry-propagating add per tile
  constexpr uint32_t SF_GPR = NV ? 2 * JT : JT;                       // scale groups per RP-element row
  uint32_t sf_row = 0, sf_rem = 0, sf_qstep = 0, sf_rstep = 0, sf_rpr = 1;
  if (BLK) {
    sf_rpr = (uint32_t)p.sf_cols / SF_GPR;                            // RP-element rows per logical row (K / RP)
    const uint32_t r0 = (uint32_t)wave_global * 32u + (uint32_t)row, step = (uint32_t)nwaves * 32u;
    sf_row = r0 / sf_rpr;
    sf_rem = r0 - sf_row * sf_rpr;
    sf_qstep = step / sf_rpr;
    sf_rstep = step - sf_qstep * sf_rpr;
  }
  for (int tile = wave_global; tile < p.ntiles; tile += nwaves) {
    // R >= 64: keep H^T in LDS instead of letting the compiler hoist its R*R/256 fragments into registers across the
    // tile loop (R = 128: 128 VGPRs, 204 in total -> 2 waves per SIMD and no latency hiding; re-reading 32 KiB of LDS
    // per 8-KiB tile is nowhere near a limit).  The opaque offset makes the address loop-variant for the optimiser.
    int hoist_guard = 0;
    if (RP >= 64) asm volatile("" : "+v"(hoist_guard));
    const int64_t r_abs = (int64_t)tile * 32 + row;
    // BLK: position of this lane's RP-element row in the logical scale matrix; advanced incrementally at the end of the loop body
    // (a division per tile cost a third more VALU instructions in a kernel that is issue-bound at small R)
    const uint32_t sf_col0 = BLK ? sf_rem * SF_GPR : 0u;
    // X^T operand: lane (row, half), chunk kc -> x[r_abs][16 kc + 8 half .. +8)  (16 bytes).  Software pipeline: the
    // loads of the wave's NEXT tile are issued before this tile is computed (tiles past the end fall off the buffer
    // descriptor and read 0), so the HBM latency of tile i+1 hides behind the MFMAs / epilogue of tile i.
    v8bf xf[KC];
    const float gs_cur = gs_next;     // GSCALE: this tile's scales (lane l: logical row l & 31 of the tile) and its rem, before the lookup below moves on
    const uint32_t c_rem = n_rem;
    if constexpr (GATED) {   // gate, up -> the act chunk the plain kernel would have loaded
      oai_bias_loads();   // ACT_OAI_BIAS: this tile's bias chunks (its experts were looked up a tile ago), then the lookup for the next tile
#pragma unroll
      for (int i = 0; i < KC; ++i) {
        if constexpr (ACT == ACT_SILU) xnext[i] = silu_mul8(xnext[i], unext[i]);
        else if constexpr (OAIB) xnext[i] = swiglu_oai_mul8<true>(xnext[i], unext[i], bgnext[i], bunext[i], p.oai);
        else xnext[i] = swiglu_oai_mul8<false>(xnext[i], unext[i], xnext[i], unext[i], p.oai);   // (no bias: the last two are not read)
      }
    }
    if (STAGED) {
      constexpr int CPR = RP / 8;                // 16-byte chunks per row
#pragma unroll
      for (int i = 0; i < KC; ++i) {
        const int q = i * 64 + lane;             // chunk of the tile held in xnext[i]
        *(v4i*)(xs + (q / CPR) * XROW + (q % CPR) * 16) = xnext[i];
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): the wave's own writes landed (wave-private area)
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) xf[kc] = *(const v8bf*)(xs + row * XROW + (2 * kc + half) * 16);
    } else {
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) xf[kc] = __builtin_bit_cast(v8bf, xnext[kc]);
    }
    if constexpr (GATHER) {
      gather_loads(tile + nwaves);
    } else if constexpr (GATED) {
      gated_loads(tile + nwaves);
    } else {
      const int64_t on = (int64_t)(tile + nwaves) * 32 * RP * 2 + lane_off;
      const int xoffn = (tile + nwaves < p.ntiles) ? (int)on : 0x7f000000;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) xnext[kc] = __builtin_amdgcn_raw_buffer_load_b128(rx, xoffn + kc * LSTEP, 0, 0);
    }
    gscale_lookup();   // GSCALE: the next tile's, behind its x loads
    float gs = gscale;   // the global scale of this lane's RP-row
    if constexpr (GSCALE) {   // the logical row of RP-row `row` within the tile: (c_rem + row) / rpr, as in gather_off
      const uint32_t x = c_rem + (uint32_t)row;
      uint32_t q = (uint32_t)((float)x * g_rc);
      const int32_t r = (int32_t)(x - q * g_rpr);
      q += r < 0 ? 0xffffffffu : (r >= (int32_t)g_rpr ? 1u : 0u);
      gs = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)(q * 4u), (int)__float_as_uint(gs_cur)));   // q <= row <= 31: the lane that looked that row up
    }
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      v16f acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        v8bf hf;
        if constexpr (HTR) {   // column j = 32 jt + row of h, rows k = 16 kc + 8 half .. + 7: two transposing reads of 4 rows each
          typedef short v4s_ __attribute__((ext_vector_type(4)));
          typedef __attribute__((address_space(3))) v4s_* lds_v4s_t;
          const char* tp = hT + hoist_guard + (8 * half + ((lane & 15) >> 2) + 16 * kc) * HROW + (((lane & 31) >> 4) * 16 + (lane & 3) * 4) * 2 + jt * 64;
          const v4s_ lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t)tp);
          const v4s_ hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t)(tp + 4 * HROW));
          const v8u16 hv8 = {(uint16_t)lo[0], (uint16_t)lo[1], (uint16_t)lo[2], (uint16_t)lo[3], (uint16_t)hi[0], (uint16_t)hi[1], (uint16_t)hi[2], (uint16_t)hi[3]};
          hf = __builtin_bit_cast(v8bf, hv8);
        } else {
          hf = *(const v8bf*)(hT + hoist_guard + (jt * 32 + row) * HROW + (kc * 16 + half * 8) * 2);
        }
        if constexpr (R < 32) {
          // [r5] R = 16: the two 16-element rows that share this 32-wide tile get an accumulator EACH.  Summed into one (rounds 1-4), the zero blocks of
          // blockdiag(h, h) met the OTHER row's inputs -- 0 x NaN / 0 x inf = NaN: one non-finite activation poisoned its neighbour's whole group, which the
          // reference's per-row GEMM cannot do (tests/test_gpu_round5.py).  Step kc feeds columns j = 16 kc .. + 15 only = registers 8 kc .. + 7 of a lane.
          const v16f z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          const v16f part = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hf, xf[kc], z, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 8; ++r) acc[8 * kc + r] = part[8 * kc + r];
        } else {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(hf, xf[kc], acc, 0, 0, 0);
        }
      }
      // acc[4q+e] = y[r_abs][32 jt + 8q + 4 half + e]
      const int64_t grp32 = r_abs * JT + jt;   // 32-element group index in the flat output

      if constexpr (FMT == QF_E2M3) {
        // ------------------------------ MXFP6: e8m0 per 32, e2m3 codes, 24 bytes per group -----
        // amax = max |y| over the group (v_max_f32 drops NaNs), E = the exponent field of the FP32 amax, and
        //   e8 = 255 if any y of the group is NaN or infinite (all 32 codes 0: the format has no NaN code, the scale byte carries it and the GEMM honours it),
        //   e8 = 127 if amax == 0, else clamp(E - 2, 0, 254)
        // -- the OCP MX rule: the scaled maximum lies in [4, 8), and (7.5, 8) saturates to 7.5, the largest e2m3 value.  A NaN input makes every output of its
        // rotation NaN, an infinite one +-inf or NaN, so a group that holds either has amax 0 (all NaN) or inf: the test for them (nan_risk, as in the e2m1 arm)
        // runs only behind amax == 0 || amax == inf, which -- all-zero groups aside -- real activations never meet.
        float m = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(acc[r]));
        m = xhalf_max(m);
        const int ex = (int)(__float_as_uint(m) >> 23) - 2;   // m >= +0: no sign bit above the exponent field; E <= 254 for a finite m, so e8 <= 252
        uint32_t e8 = m == 0.f ? 127u : (uint32_t)(ex < 0 ? 0 : ex);
        bool poison = false;
        if (__builtin_expect(m == 0.f || !(m < __builtin_inff()), 0)) {
          uint32_t bad = 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) bad |= (__float_as_uint(acc[r]) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
          bad |= (uint32_t)__shfl_xor((int)bad, 32, 64);   // the other half of the group
          poison = bad != 0;
          if (poison) e8 = 255u;
        }
        // t = y * 2^(127 - e8), an fp32 MULTIPLY by a normal power of two as in the MXFP8 arm and for its reason (e8 = 0 would make the converters' scale operand
        // a denormal); exact unless it falls below 2^-126, far under half the smallest e2m3 step (2^-4), where it rounds to (signed) zero either way.
        // Codes by integer arithmetic: a = min(|t|, 7.5); its e2m3 step is 2^(max(E_a, 127) - 130) -- 1/8 below 2, 1/4 below 4, 1/2 below 8 -- and adding
        // 1.5 * 2^23 steps rounds a to a whole number n of steps in the sum's low mantissa bits, to nearest, ties to even (the adder's own rounding; n even <=> code
        // even).  n = 0 .. 16 below 2, 8 .. 16 above: code = n + 8 (max(E_a, 127) - 127), where n = 16 carries into the next exponent as it should.
        float t[16];
        scale_pk<16>(acc, 0, __uint_as_float((254u - (poison ? 127u : e8)) << 23), t);
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t c4 = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t tb = __float_as_uint(t[4 * q + e]);
            const float a = fminf(__uint_as_float(tb & 0x7fffffffu), 7.5f);
            const uint32_t er = __float_as_uint(a) >> 23, ea = er < 127u ? 127u : er;
            const uint32_t magic = ((ea + 20u) << 23) | 0x400000u;
            const uint32_t n = __float_as_uint(a + __uint_as_float(magic)) - magic;
            uint32_t code = (n + ((ea - 127u) << 3)) | ((tb >> 31) << 5);
            code = poison ? 0u : code;
            c4 |= code << (6 * e);
          }
          w[q] = c4;   // elements 8 q + 4 half .. + 3: bytes 6 q + 3 half .. + 2 of the group's 24
        }
        // The 24 bytes are eight 3-byte runs that alternate between the lane halves.  One v_permlane32_swap pair, as in the MXFP8 arm: half 0 ends up with
        // {own w0, partner w0, own w1, partner w1} = bytes 0 .. 11, half 1 with {partner w2, own w2, partner w3, own w3} = bytes 12 .. 23 -- three dwords per lane.
        auto s0 = __builtin_amdgcn_permlane32_swap(w[0], w[2], false, false);
        auto s1 = __builtin_amdgcn_permlane32_swap(w[1], w[3], false, false);
        const uint32_t x0 = s0[0], x1 = s0[1], x2 = s1[0], x3 = s1[1];
        if (grp32 < ngroups) {
          uint32_t* o = (uint32_t*)(p.out + grp32 * 24 + half * 12);
          o[0] = x0 | (x1 << 24);
          o[1] = (x1 >> 8) | (x2 << 16);
          o[2] = (x2 >> 16) | (x3 << 8);
          if (half == 0) p.out_sf[grp32] = (uint8_t)e8;
        }
      } else if constexpr (FMT != QF_E2M1) {
        // ------------------------------ MXFP8: e8m0 per 32, e4m3 / e5m2 codes ------------------
        // amax = max |y| over the group (v_max_f32 drops NaNs: a group that is all NaN has amax 0), E = the exponent field of the FP32 amax, and
        //   e8 = 127 if amax == 0, else clamp(E - SH, 0, 254),  SH = 7 (e4m3) / 14 (e5m2)
        // -- the scaled maximum lies in [128, 256) / [2^14, 2^15), below the formats' largest finite values 448 / 57344: no finite input saturates, whatever
        // the converter does on overflow.  Integer arithmetic on the exponent field; E <= 255 makes the upper clamp vacuous (e8 <= 248).
        float m = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(acc[r]));
        m = xhalf_max(m);
        constexpr int SH = FMT == QF_E4M3 ? 7 : 14;
        const int ex = (int)(__float_as_uint(m) >> 23) - SH;   // m >= +0: no sign bit above the exponent field
        const uint32_t e8 = m == 0.f ? 127u : (uint32_t)(ex < 0 ? 0 : ex);
        // q = RNE(y * 2^(127 - e8)).  The scaling is an fp32 MULTIPLY in front of a unit-scale convert, not the converter's scale operand: that operand would be
        // 2^(e8 - 127), which for e8 = 0 (a group whose maximum is below 2^-120 / 2^-113) is 2^-127, an fp32 DENORMAL -- and what the converter makes of a
        // denormal scale is not pinned by anything in this tree (tests/native/cvt_scale_probe.hip covers the fp4 converter with normal scales only).  The
        // multiplier 2^(127 - e8) is a normal number for every e8 the rule can give (e8 in [0, 248]: 2^127 ... 2^-121), so the product is exact unless it
        // falls below 2^-126 -- far under half the formats' smallest subnormals (2^-10, 2^-17), where it rounds to (signed) zero either way.  -0 keeps its sign.
        float t[16];
        scale_pk<16>(acc, 0, __uint_as_float((254u - e8) << 23), t);
        // acc[4 q + e] = element 8 q + 4 half + e of the group: dword 2 q + half of its 32 bytes.  Half 0 keeps its dwords 0 and 2 and takes 1 and 3 from the
        // partner lane, half 1 keeps 5 and 7 and takes 4 and 6: 8 of a lane's 16 bytes change hands, 4 per v_permlane32_swap each way -- two swaps (the e2m1 arm
        // moves 4 of 8 bytes and needs one), then one 16-byte store per lane: the group is one 32-byte run.
        const uint32_t w0 = fp8_pack4<FMT>(t), w1 = fp8_pack4<FMT>(t + 4), w2 = fp8_pack4<FMT>(t + 8), w3 = fp8_pack4<FMT>(t + 12);
        auto s0 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);   // half 0: {own w0 = D0, partner w0 = D1}; half 1: {partner w2 = D4, own w2 = D5}
        auto s1 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);   // half 0: {D2, D3}; half 1: {D6, D7}
        v4i o;
        o[0] = (int)s0[0];
        o[1] = (int)s0[1];
        o[2] = (int)s1[0];
        o[3] = (int)s1[1];
        if (grp32 < ngroups) {
          *(v4i*)(p.out + grp32 * 32 + half * 16) = o;
          if (half == 0) p.out_sf[BLK ? (int64_t)blocked_sf_offset(sf_row, sf_col0 + jt, sfCB) : grp32] = (uint8_t)e8;
        }
      } else if (!NV) {
        // ------------------------------ MX: e8m0 per 32 ----------------------------------------
        float scale;
        // nan_risk: the group may hold NaNs.  A NaN activation makes ALL outputs of its rotation NaN (0 x NaN included), an inf makes them +-inf or NaN: the
        // maximum (which ignores NaNs) is then exactly 0 or inf, the variance NaN or inf -- conditions that are free to test and (all-zero groups aside) never
        // true on real activations.  Only such groups pay for the NaN -> 0x7 fix-up below (1-5 % of the kernel when done unconditionally, profiles/ab_stream_r5n_*).
        bool nan_risk;
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
          if (__builtin_expect(!(var > s2 * (0.03125f * 0.0009765625f)), 0)) {   // [r6] sign of the variance at stake: the reference's summation order
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
        // [r5] an infinite scale (a group that holds +-inf, or whose sum of squares overflows): the reference divides by it -- finite / inf = 0, inf / inf = NaN -> 0x7
        // (epilogue_quant.h:546-550, :565-569).  Neither the pre-scaled multiply (inf * 2^-128 = inf -> +-6) nor the convert's own scale operand (2^128 = inf:
        // every code comes out 7) does that, so this rare arm multiplies by 0 first (0 or NaN, the same two outcomes) and converts with unit scale.
        const bool inf_scale = e8 == 255u;
        if (__builtin_expect(inf_scale, 0)) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = acc[r] * 0.0f;
          sh = 0;
        }
        if (__builtin_expect(inf_scale || nan_risk, 0)) {   // NaN -> +inf -> code 0x7 (nan_to_pinf above; a NaN never passes the clip test either way)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = nan_to_pinf(acc[r]);
        }
        float t[16];
        uint32_t mbits = 0;
        float cs = 1.0f;   // scale operand of the hardware convert
        if (METHOD == METHOD_ABSMAX && !MASK) {
          // (y * 2^sh) * 3 == y * (3 * 2^sh): the power-of-two scaling is exact, so one multiply by the pre-scaled
          // constant rounds exactly like the reference's two steps (scale >= 1e-8 keeps 3 * 2^sh finite; results in the
          // denormal range quantise to 0 either way)
          scale_pk<16>(acc, 0, ldexpf(3.0f, sh), t);
        } else if (HWCVT) {
          // [r3] y / 2^(e8-127) happens inside the convert (see e2m1_pack2_hw): no v_ldexp_f32 per element.  The clip test
          // |y * 2^sh| < 6 is |y| < 6 * 2^-sh (power-of-two scaling of either side is exact).
          cs = inf_scale ? 1.0f : __uint_as_float(e8 << 23);   // e8 >= 100: scale >= 1e-8
          if (MASK) {
            const float lim = 6.0f * cs;
#pragma unroll
            for (int r = 0; r < 16; ++r) mbits |= (fabsf(acc[r]) < lim ? 1u : 0u) << (8 * (r >> 2) + 4 * half + (r & 3));
          }
          if (METHOD == METHOD_ABSMAX) {
            scale_pk<16>(acc, 0, 3.0f, t);
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = acc[r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = ldexpf(acc[r], sh);
            if (MASK) mbits |= (fabsf(v) < 6.0f ? 1u : 0u) << (8 * (r >> 2) + 4 * half + (r & 3));
            if (METHOD == METHOD_ABSMAX) v = v * 3.0f;
            t[r] = v;
          }
        }
        // bytes: q-th group of 4 values -> group bytes 4q + 2 half, 4q + 2 half + 1
        const uint32_t P = e2m1_pack8<HWCVT>(t, cs);       // halfwords H[0+half], H[2+half]
        const uint32_t Q = e2m1_pack8<HWCVT>(t + 8, cs);   // halfwords H[4+half], H[6+half]
        auto sw = __builtin_amdgcn_permlane32_swap(P, Q, false, false);
        const uint32_t X = sw[0], Y = sw[1];
        // half 0: X = own P, Y = partner P ; half 1: X = partner Q, Y = own Q
        v2i o;
        o[0] = (int)((X & 0xffffu) | (Y << 16));
        o[1] = (int)((X >> 16) | (Y & 0xffff0000u));
        const bool ok = grp32 < ngroups;
        if (ok) {
          *(v2i*)(p.out + grp32 * 16 + half * 8) = o;
          if (half == 0) p.out_sf[BLK ? (int64_t)blocked_sf_offset(sf_row, sf_col0 + jt, sfCB) : grp32] = (uint8_t)e8;
        }
        if (MASK) {
          const uint32_t mm = xhalf_or(mbits);
          if (ok && half == 0) p.out_mask[grp32] = mm;
        }
      } else {
        // ------------------------------ NV: e4m3 per 16 ----------------------------------------
        // lane holds j = 8q + 4 half + e: q in {0,1} belong to 16-group 2*grp32, q in {2,3} to +1
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          float v8[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v8[r] = acc[sub * 8 + r];
          float out_scale;
          uint32_t sfb;
          bool nan_risk;   // (as in the MX arm)
          if (METHOD == METHOD_ABSMAX) {
            float m = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) m = fmaxf(m, fabsf(v8[r]));
            m = xhalf_max(m);
            nan_risk = m == 0.f || !(m < __builtin_inff());
            float sf = gs * (m * (1.0f / 6.0f));
            sfb = e4m3_encode_pos(sf);
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
            // var < 0 can only come from fp32 rounding on a (nearly) constant group.  [r6] The reference takes sqrt of it and stores the NaN it
            // gets as the scale byte 0x7f (epilogue_quant.h:1631-1640: no guard; `scale_q > 0` is then false, the multiplier 0 and every code +-0):
            // so does this kernel -- rounds 1-5 clamped the variance at 0.  A NaN variance (NaN / inf activations) takes the same path.
            float var = fmaf(-mean, mean, s2 * 0.0625f);
            if (__builtin_expect(!(var > s2 * (0.0625f * 0.0009765625f)), 0)) {   // whether it is negative depends on the order of the additions: the reference's
              quest_sums_in_reference_order<2>(v8, 0, s1, s2);
              mean = s1 * 0.0625f;
              var = fmaf(-mean, mean, s2 * 0.0625f);
            }
            nan_risk = !(var >= 0.f);
            const float sc = (float)((double)sqrtf(var) * (2.92247856 / 6.) + 1e-8);
            sfb = e4m3_encode_pos(sc);
            const float sq = e4m3_decode_pos(sfb);
            out_scale = (sq > 0.f) ? __frcp_rn(sq) : 0.0f;
          }
          float t[8];
          scale_pk<8>(v8, 0, out_scale, t);
          if (__builtin_expect(nan_risk, 0)) {
#pragma unroll
            for (int r = 0; r < 8; ++r) t[r] = nan_to_pinf(t[r]);
          }
          // 8 values = bytes {0,1,4,5} + 2*half of the 8-byte group: halfwords H[half], H[2+half]
          const uint32_t P = e2m1_pack8<HWCVT>(t);
          auto sw = __builtin_amdgcn_permlane32_swap(P, P, false, false);
          // half 0: sw[0] = own P (H0,H2), sw[1] = partner P (H1,H3)
          // half 1: sw[0] = partner P (H0,H2), sw[1] = own P (H1,H3)
          const uint32_t X = sw[0], Y = sw[1];
          const uint32_t d0 = (X & 0xffffu) | (Y << 16);          // bytes 0..3
          const uint32_t d1 = (X >> 16) | (Y & 0xffff0000u);      // bytes 4..7
          const int64_t grp16 = grp32 * 2 + sub;
          if (grp16 < ngroups) {
            *(uint32_t*)(p.out + grp16 * 8 + half * 4) = half ? d1 : d0;
            if (half == 0) p.out_sf[BLK ? (int64_t)blocked_sf_offset(sf_row, sf_col0 + 2 * jt + sub, sfCB) : grp16] = (uint8_t)sfb;
          }
        }
      }
    }
    if (BLK) {   // next tile of this wave: r_abs += nwaves * 32
      sf_rem += sf_rstep;
      const uint32_t carry = sf_rem >= sf_rpr ? 1u : 0u;
      sf_rem -= carry ? sf_rpr : 0u;
      sf_row += sf_qstep + carry;
    }
  }
}

template <int R, bool NV, int METHOD, bool MASK, bool HWCVT, bool BLK = false>
__global__ __launch_bounds__(256) void fused_quantize_kernel(const QuantParams p) {
  fused_quantize_body<R, NV, METHOD, MASK, HWCVT, BLK>(p, (int)blockIdx.x, (int)gridDim.x);
}

// the gated quantizers (fusedSiluMulQuantize{Mx,Nv}[Blocked]): the hardware e2m1 convert only, no clip mask
template <int R, bool NV, int METHOD, bool BLK>
__global__ __launch_bounds__(256) void fused_silu_mul_quantize_kernel(const QuantParams p) {
  fused_quantize_body<R, NV, METHOD, false, true, BLK, true, true>(p, (int)blockIdx.x, (int)gridDim.x);
}

// the clamped-SwiGLU quantizer (fusedSwigluOaiQuantizeMx): MX e2m1 with flat scales, R = 32 / 64, with or without the per-expert gate/up bias
template <int R, int METHOD, bool BIAS>
__global__ __launch_bounds__(256) void fused_swiglu_oai_quantize_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD, false, true, false, true, true, false, false, QF_E2M1, BIAS ? ACT_OAI_BIAS : ACT_OAI>(p, (int)blockIdx.x, (int)gridDim.x);
}

// the gathering quantizers (fusedGatherQuantize{Mx,Nv}): the hardware e2m1 convert only, flat scales, no clip mask
template <int R, bool NV, int METHOD>
__global__ __launch_bounds__(256) void fused_gather_quantize_kernel(const QuantParams p) {
  fused_quantize_body<R, NV, METHOD, false, true, false, true, false, true>(p, (int)blockIdx.x, (int)gridDim.x);
}

// the grouped-scale forms (fused{Gather,SiluMul}QuantizeNvGrouped): NV abs-max with one global scale per expert (GSCALE above); method quest runs the kernels above
template <int R>
__global__ __launch_bounds__(256) void fused_gather_quantize_gscale_kernel(const QuantParams p) {
  fused_quantize_body<R, true, METHOD_ABSMAX, false, true, false, true, false, true, true>(p, (int)blockIdx.x, (int)gridDim.x);
}
template <int R>
__global__ __launch_bounds__(256) void fused_silu_mul_quantize_gscale_kernel(const QuantParams p) {
  fused_quantize_body<R, true, METHOD_ABSMAX, false, true, false, true, true, false, true>(p, (int)blockIdx.x, (int)gridDim.x);
}

// the MXFP8 quantizers (fusedQuantizeMxf8[Blocked], fusedSiluMulQuantizeMxf8[Blocked], fusedGatherQuantizeMxf8): FMT = QF_E4M3 / QF_E5M2, abs-max
template <int R, int FMT, bool BLK>
__global__ __launch_bounds__(256) void fused_quantize_mxf8_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD_ABSMAX, false, true, BLK, true, false, false, false, FMT>(p, (int)blockIdx.x, (int)gridDim.x);
}
template <int R, int FMT, bool BLK>
__global__ __launch_bounds__(256) void fused_silu_mul_quantize_mxf8_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD_ABSMAX, false, true, BLK, true, true, false, false, FMT>(p, (int)blockIdx.x, (int)gridDim.x);
}
template <int R, int FMT>
__global__ __launch_bounds__(256) void fused_gather_quantize_mxf8_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD_ABSMAX, false, true, false, true, false, true, false, FMT>(p, (int)blockIdx.x, (int)gridDim.x);
}
// the MXFP6 quantizers (fusedQuantizeMxf6, fusedGatherQuantizeMxf6): FMT = QF_E2M3, abs-max, flat scales
template <int R>
__global__ __launch_bounds__(256) void fused_quantize_mxf6_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD_ABSMAX, false, true, false, true, false, false, false, QF_E2M3>(p, (int)blockIdx.x, (int)gridDim.x);
}
template <int R>
__global__ __launch_bounds__(256) void fused_gather_quantize_mxf6_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD_ABSMAX, false, true, false, true, false, true, false, QF_E2M3>(p, (int)blockIdx.x, (int)gridDim.x);
}
// the clamped-SwiGLU form (fusedSwigluOaiQuantizeMxf8): e4m3 with flat scales, R = 32 / 64, with or without the per-expert gate/up bias
template <int R, bool BIAS>
__global__ __launch_bounds__(256) void fused_swiglu_oai_quantize_mxf8_kernel(const QuantParams p) {
  fused_quantize_body<R, false, METHOD_ABSMAX, false, true, false, true, true, false, false, QF_E4M3, BIAS ? ACT_OAI_BIAS : ACT_OAI>(p, (int)blockIdx.x, (int)gridDim.x);
}

// The launch of the four row-stream ops below (silu_and_mul, swiglu_oai_and_mul, moe_combine with and without a bias): a pure function of the 16-byte chunks to write and
// the CU count (capi.hip chip_cus; the debug entry passes its own).  A thread per chunk until ROW_STREAM_WG_PER_CU workgroups per CU are out; the kernels stride over the rest.
constexpr int ROW_STREAM_WG_PER_CU = 8;   struct RowStreamLaunch { int grid, threads; };
inline RowStreamLaunch row_stream_plan(int64_t chunks, int64_t cus) { return {(int)std::min<int64_t>((chunks + 255) / 256, cus * ROW_STREAM_WG_PER_CU), 256}; }

// silu_and_mul: x (rows, 2 I) bf16 -> out (rows, I) bf16, out[r][c] = act(x[r][c], x[r][I + c]) (silu_mul8 above).  Streaming, 4 B in + 2 B out per element: a
// thread takes 16-byte chunks (8 elements; I % 8 == 0) chunk = first + k * step, kept as (row, chunk within the row) with a carry-propagating add -- no division in
// the loop -- and 64-bit addresses, so neither operand has a size limit below rows, I < 2^31.
struct SiluMulParams {
  const uint16_t* x;
  uint16_t* out;
  int64_t chunks;    // rows * I / 8
  uint32_t cpr;      // chunks per row, I / 8
};
template <int UNUSED = 0>   // (a template so that only the unit that launches it holds a copy)
__global__ __launch_bounds__(256) void silu_mul_bf16_kernel(const SiluMulParams p) {
  const uint32_t first = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
  uint32_t row = first / p.cpr, cc = first - row * p.cpr;
  const uint32_t qstep = step / p.cpr, rstep = step - qstep * p.cpr;
  for (int64_t c = first; c < p.chunks; c += step) {
    const uint16_t* g = p.x + ((int64_t)row * 2 * p.cpr + cc) * 8;
    const v4i gv = *(const v4i*)g, uv = *(const v4i*)(g + (int64_t)p.cpr * 8);
    *(v4i*)(p.out + c * 8) = silu_mul8(gv, uv);
    cc += rstep;
    const uint32_t carry = cc >= p.cpr ? 1u : 0u;
    cc -= carry ? p.cpr : 0u;
    row += qstep + carry;
  }
}

// swiglu_oai_and_mul: silu_mul_bf16_kernel with the clamped SwiGLU (swiglu_oai_mul8 above), out[r][c] = act(x[r][c], x[r][I + c] [, bias[g(r)][c], bias[g(r)][I + c]]).
// BIAS: bias is (E, 2 I) bf16 in the same halves and g(r) = quant_group_of_row(offs, E, r) -- the workgroup copies offs into LDS once (E > 1; one expert reads no
// offs), a thread searches the copy once per chunk it visits (at most 11 LDS reads) and fetches the two bias chunks, which every row of the expert shares, from L2.
// The expert is clamped to [0, E): malformed offs cannot address outside bias.  64-bit addresses throughout.
struct SwigluOaiParams {
  const uint16_t* x;
  uint16_t* out;
  const uint16_t* bias;   // (E, 2 I) bf16 or null
  const int32_t* offs;    // (E) or null (E == 1)
  int64_t chunks;         // rows * I / 8
  uint32_t cpr;           // chunks per row, I / 8
  int E;
  SwigluOaiAct act;
};
// the workgroup's LDS copy of offs for the streaming kernels (E > 1), published by a barrier
__device__ __forceinline__ const int32_t* stream_offs_lds(const int32_t* offs, int E) {
  int32_t* so = quant_offs_lds();
  if (E > 1)
    for (int i = threadIdx.x; i < E; i += 256) so[i] = offs[i];
  __syncthreads();
  return so;
}
template <bool BIAS>
__global__ __launch_bounds__(256) void swiglu_oai_mul_bf16_kernel(const SwigluOaiParams p) {
  const int32_t* so = nullptr;
  if constexpr (BIAS) so = stream_offs_lds(p.offs, p.E);
  const uint32_t first = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
  uint32_t row = first / p.cpr, cc = first - row * p.cpr;
  const uint32_t qstep = step / p.cpr, rstep = step - qstep * p.cpr;
  for (int64_t c = first; c < p.chunks; c += step) {
    const uint16_t* g = p.x + ((int64_t)row * 2 * p.cpr + cc) * 8;
    const v4i gv = *(const v4i*)g, uv = *(const v4i*)(g + (int64_t)p.cpr * 8);
    if constexpr (BIAS) {
      int e = quant_group_of_row(so, p.E, (int)row);
      e = e < 0 ? 0 : (e < p.E ? e : p.E - 1);
      const uint16_t* b = p.bias + ((int64_t)e * 2 * p.cpr + cc) * 8;
      const v4i bg = *(const v4i*)b, bu = *(const v4i*)(b + (int64_t)p.cpr * 8);
      *(v4i*)(p.out + c * 8) = swiglu_oai_mul8<true>(gv, uv, bg, bu, p.act);
    } else {
      *(v4i*)(p.out + c * 8) = swiglu_oai_mul8<false>(gv, uv, gv, uv, p.act);
    }
    cc += rstep;
    const uint32_t carry = cc >= p.cpr ? 1u : 0u;
    cc -= carry ? p.cpr : 0u;
    row += qstep + carry;
  }
}

// moe_combine: out[t][c] = bf16_rne(sum over k = 0 .. topk - 1, in that order, of w[t][k] * float(y[pos[t][k]][c])), the sum starting from +0 and every product and every
// sum rounded to fp32 on its own (no fma: numpy.float32 reproduces it bit for bit).  A slot whose pos lies outside [0, M) is SKIPPED -- its load goes to row 0 and the
// loaded value is dropped by a select, never multiplied -- so a NaN in a row that no slot names cannot reach out.  Written as a gather: no atomics, the result does
// not depend on the launch geometry.  Streaming like silu_mul_bf16_kernel: 16-byte chunks (H % 8 == 0), (row, chunk) carried without a division, 64-bit addresses
// (rows, columns < 2^31 is the only limit).  Slots go four at a time so that four row loads are in flight per thread.  y needs one row (the host never launches M == 0).
struct MoeCombineParams {
  const uint16_t* y;     // (M, H) bf16
  const int32_t* pos;    // (T, topk)
  const float* w;        // (T, topk)
  uint16_t* out;         // (T, H) bf16
  int64_t chunks;        // T * H / 8
  uint32_t cpr;          // chunks per row, H / 8
  uint32_t m;            // rows of y
  int topk;
};
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void moe_combine_bf16_kernel(const MoeCombineParams p) {
#pragma clang fp contract(off)
  const uint32_t first = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
  uint32_t row = first / p.cpr, cc = first - row * p.cpr;
  const uint32_t qstep = step / p.cpr, rstep = step - qstep * p.cpr;
  for (int64_t c = first; c < p.chunks; c += step) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const int64_t slot0 = (int64_t)row * p.topk;
    for (int k0 = 0; k0 < p.topk; k0 += 4) {
      float w[4];
      bool ok[4];
      v4i v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j < p.topk ? k0 + j : p.topk - 1;   // (past the last slot: a second read of it, dropped below)
        const uint32_t ps = (uint32_t)p.pos[slot0 + k];
        w[j] = p.w[slot0 + k];
        ok[j] = k0 + j < p.topk && ps < p.m;
        v[j] = *(const v4i*)(p.y + ((int64_t)(ok[j] ? ps : 0u) * p.cpr + cc) * 8);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t yw = (uint32_t)v[j][e];
          const float lo = w[j] * __uint_as_float(yw << 16), hi = w[j] * __uint_as_float(yw & 0xffff0000u);
          const float slo = acc[2 * e] + lo, shi = acc[2 * e + 1] + hi;
          acc[2 * e] = ok[j] ? slo : acc[2 * e];
          acc[2 * e + 1] = ok[j] ? shi : acc[2 * e + 1];
        }
      }
    }
    v4i o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (int)pack_bf16x2(acc[2 * e], acc[2 * e + 1]);
    *(v4i*)(p.out + c * 8) = o;
    cc += rstep;
    const uint32_t carry = cc >= p.cpr ? 1u : 0u;
    cc -= carry ? p.cpr : 0u;
    row += qstep + carry;
  }
}

// moe_combine with the down projection's bias: moe_combine_bf16_kernel with v = bf16_rne(float(y[p][c]) + float(bias[g(p)][c])) (one fp32 add, then RNE: a bf16
// tensor add) in place of y[p][c], g(p) = quant_group_of_row(offs, E, p) from the workgroup's LDS copy of offs -- the group the grouped GEMM computed row p in.  A
// skipped slot reads row 0 of y and the bias row of row 0's expert, and both are dropped by the same select.  bias is (E, H) bf16; the expert is clamped to [0, E).
struct MoeCombineBiasParams {
  MoeCombineParams c;
  const uint16_t* bias;
  const int32_t* offs;
  int E;
};
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void moe_combine_bias_bf16_kernel(const MoeCombineBiasParams pb) {
#pragma clang fp contract(off)
  const MoeCombineParams& p = pb.c;
  const int32_t* so = stream_offs_lds(pb.offs, pb.E);
  const uint32_t first = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
  uint32_t row = first / p.cpr, cc = first - row * p.cpr;
  const uint32_t qstep = step / p.cpr, rstep = step - qstep * p.cpr;
  for (int64_t c = first; c < p.chunks; c += step) {
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const int64_t slot0 = (int64_t)row * p.topk;
    for (int k0 = 0; k0 < p.topk; k0 += 4) {
      float w[4];
      bool ok[4];
      v4i v[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j < p.topk ? k0 + j : p.topk - 1;   // (past the last slot: a second read of it, dropped below)
        const uint32_t ps = (uint32_t)p.pos[slot0 + k];
        w[j] = p.w[slot0 + k];
        ok[j] = k0 + j < p.topk && ps < p.m;
        const uint32_t r = ok[j] ? ps : 0u;
        int g = quant_group_of_row(so, pb.E, (int)r);
        g = g < 0 ? 0 : (g < pb.E ? g : pb.E - 1);
        v[j] = *(const v4i*)(p.y + ((int64_t)r * p.cpr + cc) * 8);
        b[j] = *(const v4i*)(pb.bias + ((int64_t)g * p.cpr + cc) * 8);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t yw = (uint32_t)v[j][e], bw = (uint32_t)b[j][e];
          const uint32_t vw = pack_bf16x2(__uint_as_float(yw << 16) + __uint_as_float(bw << 16), __uint_as_float(yw & 0xffff0000u) + __uint_as_float(bw & 0xffff0000u));
          const float lo = w[j] * __uint_as_float(vw << 16), hi = w[j] * __uint_as_float(vw & 0xffff0000u);
          const float slo = acc[2 * e] + lo, shi = acc[2 * e + 1] + hi;
          acc[2 * e] = ok[j] ? slo : acc[2 * e];
          acc[2 * e + 1] = ok[j] ? shi : acc[2 * e + 1];
        }
      }
    }
    v4i o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (int)pack_bf16x2(acc[2 * e], acc[2 * e + 1]);
    *(v4i*)(p.out + c * 8) = o;
    cc += rstep;
    const uint32_t carry = cc >= p.cpr ? 1u : 0u;
    cc -= carry ? p.cpr : 0u;
    row += qstep + carry;
  }
}

}  // namespace qamd
