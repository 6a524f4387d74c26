// 2 x 2 max-pool of a bf16 NHWC tensor, [N, Hs, Ws, C] -> [N, Hs / 2, Ws / 2, C] (even Hs, Ws;
// C % 8 == 0): one 16-byte unit (8 channels of one output pixel) per thread, four 16-byte loads and one
// 16-byte store.  The reduction is the per-layer conv loader's (conv2d_nhwc.hip, INMODE 2),
// fmaxf(fmaxf(r0, r1), fmaxf(q0, q1)) per half-word on the raw values, with r the source row 2 y, q the
// row 2 y + 1 and 0 / 1 the columns 2 x / 2 x + 1, so signed zeros and ties come out as they do there
// and a consumer that reads the pooled tensor sees the bits the loader would have formed.  The maximum
// of bf16 values is a bf16 value: nothing rounds.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t pool_max4(uint32_t r0, uint32_t r1, uint32_t q0, uint32_t q1) {
  const float lo = fmaxf(fmaxf(lo_bf(r0), lo_bf(r1)), fmaxf(lo_bf(q0), lo_bf(q1)));
  const float hi = fmaxf(fmaxf(hi_bf(r0), hi_bf(r1)), fmaxf(hi_bf(q0), hi_bf(q1)));
  return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}

// units: N * H * W * CU output units, CU = C / 8; a row of output pixels is W * CU consecutive units
__global__ __launch_bounds__(256) void pool2_nhwc_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out,
                                                         long long units, int H, int W, int CU) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int c = (int)(u % CU);
  const long long p = u / CU;            // output pixel (n * H + y) * W + x
  const int px = (int)(p % W);
  const long long ny = p / W;            // n * H + y: source row pair 2 ny, 2 ny + 1 of [N * 2 H] rows
  const size_t row = (size_t)2 * W * CU;  // units per source row
  const u32x4* s = reinterpret_cast<const u32x4*>(x) + (size_t)2 * ny * row + (size_t)2 * px * CU + c;
  const u32x4 r0 = s[0], r1 = s[CU], q0 = s[row], q1 = s[row + CU];
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = pool_max4(r0[j], r1[j], q0[j], q1[j]);
  reinterpret_cast<u32x4*>(out)[u] = o;
}

}  // namespace

extern "C" {

// out [N, Hs / 2, Ws / 2, C] = 2 x 2 max-pool of x [N, Hs, Ws, C], both bf16 NHWC and contiguous, on
// `stream`.  -40: a null pointer, an odd source size or C % 8 != 0.
int be_pool2_nhwc(const void* x, void* out, int N, int Hs, int Ws, int C, hipStream_t stream) {
  if (!x || !out || x == out || N <= 0 || Hs <= 0 || Ws <= 0 || C <= 0 || (Hs & 1) || (Ws & 1) || (C & 7)) return -40;
  const long long units = (long long)N * (Hs / 2) * (Ws / 2) * (C / 8);
  const long long blocks = (units + 255) / 256;
  if (blocks >= (1LL << 31)) return -41;
  hipLaunchKernelGGL(pool2_nhwc_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)out, units,
                     Hs / 2, Ws / 2, C / 8);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
