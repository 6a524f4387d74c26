// Shared pieces of the exact percentile normalisation (percentile.hip) for kernels that apply it
// on the fly (tiles.hip: normalise inside the tile gather).
//
// The radix select works on order-preserving uint32 keys, most significant digit first.  A row of
// raw integer pixels needs only as many 8-bit digit passes as its type has bytes: the key of a
// uint16 pixel is v << 16 (two passes), of a uint8 pixel v << 24 (one pass), of a float the usual
// sign-flipped bit pattern (four passes).  After the last pass a target's prefix is its full key.
#pragma once
#include "common.h"

namespace be_pct {

constexpr int kT = 6;  // targets: lo(p_lower), hi(p_lower), lo(p_upper), hi(p_upper), min, max

// element type codes of the entry points that take raw pixels
enum { kF32 = 0, kU16 = 1, kU8 = 2 };

__device__ __forceinline__ uint32_t fkey_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// key(): order-preserving key of one element; word_key<e>(): key of element e of a 16-byte vector
// held as four 32-bit words; val(): the element's value as fp32 from its full key.
template <typename T>
struct Elem;
template <>
struct Elem<float> {
  static constexpr int passes = 4, per_vec = 4;
  static __device__ __forceinline__ uint32_t key(float f) { return fkey_bits(__float_as_uint(f)); }
  static __device__ __forceinline__ uint32_t word_key(const u32x4& w, int e) { return fkey_bits(w[e]); }
  static __device__ __forceinline__ float val(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  }
};
template <>
struct Elem<uint16_t> {
  static constexpr int passes = 2, per_vec = 8;
  static __device__ __forceinline__ uint32_t key(uint16_t v) { return (uint32_t)v << 16; }
  static __device__ __forceinline__ uint32_t word_key(const u32x4& w, int e) {
    return (e & 1) ? (w[e >> 1] & 0xffff0000u) : (w[e >> 1] << 16);
  }
  static __device__ __forceinline__ float val(uint32_t k) { return (float)(k >> 16); }
};
template <>
struct Elem<uint8_t> {
  static constexpr int passes = 1, per_vec = 16;
  static __device__ __forceinline__ uint32_t key(uint8_t v) { return (uint32_t)v << 24; }
  static __device__ __forceinline__ uint32_t word_key(const u32x4& w, int e) {
    return (w[e >> 2] >> (8 * (e & 3))) << 24;
  }
  static __device__ __forceinline__ float val(uint32_t k) { return (float)(k >> 24); }
};

// interpolation weights (1 - f) and f of the two percentiles, rounded to fp32 on the host
struct Coef {
  float a_lo, b_lo, a_hi, b_hi;
};

// Per-row constants from the row's six selected keys (st = state + row * kT * 2): x -> cst ? 0 :
// (x - p1) * scale.  Same rounding as the oracle: weights rounded to fp32 on the host, fp32 math.
template <typename T>
__device__ __forceinline__ void row_consts(const uint32_t* __restrict__ st, const Coef cf, float& p1, float& scale,
                                           bool& cst) {
  p1 = Elem<T>::val(st[0]) * cf.a_lo + Elem<T>::val(st[2]) * cf.b_lo;
  const float p99 = Elem<T>::val(st[4]) * cf.a_hi + Elem<T>::val(st[6]) * cf.b_hi;
  const float rng = p99 - p1;
  scale = rng > 1e-3f ? 1.0f / rng : 1.0f;
  cst = Elem<T>::val(st[10]) - Elem<T>::val(st[8]) == 0.0f;
}

// ---- normalisation options beyond the default (cellpose `normalize` dict): fixed bounds, inversion,
// local (tile) normalisation against per-block percentile maps.  One set of per-call constants for
// the normalising gathers (tiles.hip) and the unfused apply (percentile.hip), and one function per
// rule, so both write the same bits.  Every multiply that feeds an add is an explicit fmaf: nothing
// is left to the compiler's contraction, which may differ between two kernels.
struct NormExt {
  const float* lowhigh = nullptr;  // [C_use][2] fixed (lo, hi) per channel: no percentile is taken
  const float* lo_map = nullptr;   // tile normalisation: smoothed maps [B * C_use, ny, nx]
  const float* hi_map = nullptr;
  int ny = 0, nx = 0;
  float sy = 0.f, sx = 0.f;  // ny / H, nx / W, rounded to fp32 on the host
  int invert = 0;            // x -> 1 - x after the normalisation
};

constexpr int kMaxCells = 4096;  // largest block grid (ny * nx) of the tile normalisation

// (v - lo) / den, by a true division as the oracle divides; a constant channel is 0 before inversion
__device__ __forceinline__ float norm_div(float v, float lo, float den, bool cst, bool invert) {
  const float r = cst ? 0.f : (v - lo) / den;
  return invert ? 1.f - r : r;
}

// (lo, den, cst) of channel c for the global rules: fixed bounds, or the row's selected percentiles
template <typename T>
__device__ __forceinline__ void ext_consts(const NormExt& e, const uint32_t* __restrict__ st, const Coef cf, int c, float& lo,
                                           float& den, bool& cst) {
  if (e.lowhigh) {
    lo = e.lowhigh[2 * c];
    den = e.lowhigh[2 * c + 1] - lo;
    cst = false;
    return;
  }
  lo = fmaf(Elem<T>::val(st[0]), cf.a_lo, Elem<T>::val(st[2]) * cf.b_lo);
  const float p99 = fmaf(Elem<T>::val(st[4]), cf.a_hi, Elem<T>::val(st[6]) * cf.b_hi);
  const float rng = p99 - lo;
  den = rng > 1e-3f ? rng : 1.0f;
  cst = Elem<T>::val(st[10]) - Elem<T>::val(st[8]) == 0.0f;
}

// Source coordinate of output index i on an n-cell map axis: half-pixel centres, clamped
// (F.interpolate(align_corners=False)): cells i0, i1 and the weight of i1.
__device__ __forceinline__ void map_coord(int i, float scale, int n, int& i0, int& i1, float& w) {
  float s = fmaf((float)i + 0.5f, scale, -0.5f);
  s = fminf(fmaxf(s, 0.f), (float)(n - 1));
  i0 = (int)s;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  w = s - (float)i0;
}

__device__ __forceinline__ float map_sample(const float* __restrict__ m, int nx, int y0, int y1, float wy, int x0, int x1,
                                            float wx) {
  const float a = m[y0 * nx + x0], b = m[y0 * nx + x1], c = m[y1 * nx + x0], d = m[y1 * nx + x1];
  const float top = fmaf(wx, b - a, a), bot = fmaf(wx, d - c, c);
  return fmaf(wy, bot - top, top);
}

// One pixel of the tile normalisation: both maps of its (image, channel) sampled bilinearly at the
// pixel, then (v - lo) / (hi - lo).  After the fill and the smoothing hi - lo is at least ~1e-3.
__device__ __forceinline__ float tile_norm(float v, const float* __restrict__ lo_m, const float* __restrict__ hi_m, int nx,
                                           int y0, int y1, float wy, int x0, int x1, float wx, bool invert) {
  const float lo = map_sample(lo_m, nx, y0, y1, wy, x0, x1, wx);
  const float hi = map_sample(hi_m, nx, y0, y1, wy, x0, x1, wx);
  return norm_div(v, lo, hi - lo, false, invert);
}

// Queue the select passes for rows (b, c), b < B, c < C_use, of x [B, C_src, n] (element type
// `dtype`) on `s`: row b * C_use + c of the state then holds the six keys.  Validates before it
// launches anything; returns 0, or a negative code with nothing launched.  `state` points into ws.
int select_run(const void* x, int dtype, int B, int C_src, int C_use, long long n, float lower, float upper, void* ws,
               long long ws_bytes, hipStream_t s, Coef* cf, const uint32_t** state);

}  // namespace be_pct
