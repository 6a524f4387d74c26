// Cellpose: per-label measurements of label images (gfx950).
//
// Semantics: bioengine_worker_amd/cellpose/reference.py::measure_masks (the CPU oracle; the GPU tests
// compare exactly).  One host entry point, be_cp_measure, queues five launches on one stream:
//
//   init      boxes to (INT_MAX.., -1..)
//   bbox      per-label bounding boxes (integer atomicMin / atomicMax, order independent)
//   plan      one workgroup per image: bands per label, their prefix sum, the (label, band) job list
//   measure   ONE WAVE PER JOB: the wave walks its band of the label's box in row segments
//             (coalesced row reads), accumulates per lane in a fixed order, reduces across the lanes
//             with a fixed xor butterfly and stores one partial record
//   combine   one thread per label adds its partials in band order and writes the result rows
//
// The work is label-centric ("store then sum per destination"): no atomics reach the result rows, so
// every output -- the fp64 intensity sums included -- is bit-identical from run to run.  Cellpose
// labels are compact: the summed box area is a small multiple of the foreground and the label /
// image reads of overlapping boxes are served by L2.
//
// Bands.  A label's box has nrows = lz * ly rows of lx pixels.  A band is br = clamp(band_px / lx,
// 1, nrows) consecutive rows, so a label whose box is the whole image is spread over many waves
// instead of one.  band_px is BAND_PX unless the image's summed box area A is so large that the
// jobs would not fit the partial buffer: band_px = max(BAND_PX, ceil(A / s_half)).  A label then
// has nb <= 2 * area / band_px + 1 bands (floor(q) >= q / 2 for q >= 1), so an image has at most
// K + 2 * s_half jobs: `slots` is sized to that on the host and nothing is read back to plan.
//
// Units.  An "image" is [Z, H, W] labels with [Z, C, H, W] fp32 intensities: a batch of 2-D images
// is B images of depth 1 (4-neighbour boundary, second moments), a volume is one image of depth Z
// (6-neighbour boundary, sum_z, no second moments).  Inside one image offsets fit 32 bits (the
// caller checks Z * H * W < 2^31); image bases are 64-bit.
#include "common.h"

#include <limits.h>

namespace {

constexpr int RL = 16;          // pixels per lane of the box kernel (one set of box updates per label run)
constexpr int BAND_PX = 1024;   // pixels per band: 16 per lane (the walk is latency bound: many short waves)
constexpr int NI = 8;           // int64 fields per row
enum { F_AREA = 0, F_SZ, F_SY, F_SX, F_SYY, F_SXX, F_SXY, F_BND };
constexpr int CG = 4;           // channels per walk of the box

struct Box {
  int z0, y0, x0, lz, ly, lx;
};

// bb = (zmin, ymin, xmin, zmax, ymax, xmax) inclusive; false for a label without pixels
__device__ __forceinline__ bool load_box(const int* __restrict__ bb, Box& q) {
  q.z0 = bb[0];
  q.y0 = bb[1];
  q.x0 = bb[2];
  q.lz = bb[3] - q.z0 + 1;
  q.ly = bb[4] - q.y0 + 1;
  q.lx = bb[5] - q.x0 + 1;
  return bb[3] >= q.z0;
}

__device__ __forceinline__ int band_rows(long long band_px, int lx, int nrows) {
  long long br = band_px / lx;
  if (br < 1) br = 1;
  if (br > nrows) br = nrows;
  return (int)br;
}

__global__ __launch_bounds__(256) void init_kernel(int* __restrict__ bbox, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) bbox[i] = (i % 6) < 3 ? INT_MAX : -1;
}

// M [B, Z, H, W]; labels outside 1..K are not measured
__global__ __launch_bounds__(256) void bbox_kernel(const int* __restrict__ M, int B, int Z, int H, int W, int K,
                                                   int* __restrict__ bbox) {
  const int segs = (W + RL - 1) / RL;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)B * Z * H * segs) return;
  const int seg = (int)(gid % segs);
  const long long row = gid / segs;  // (b * Z + z) * H + y
  const int y = (int)(row % H);
  const long long plane = row / H;
  const int z = (int)(plane % Z), b = (int)(plane / Z);
  const int* Mr = M + row * W;
  const int x0 = seg * RL, x1 = min(x0 + RL, W);
  int cur = 0, xs = x0;
  auto flush = [&](int lab, int a, int e) {
    if (lab <= 0 || lab > K) return;
    // a plain read first: minima only fall and maxima only rise, so a stale value can only ask for
    // an atomic that was not needed
    int* bb = bbox + ((size_t)b * K + (lab - 1)) * 6;
    if (z < bb[0]) atomicMin(bb + 0, z);
    if (y < bb[1]) atomicMin(bb + 1, y);
    if (a < bb[2]) atomicMin(bb + 2, a);
    if (z > bb[3]) atomicMax(bb + 3, z);
    if (y > bb[4]) atomicMax(bb + 4, y);
    if (e > bb[5]) atomicMax(bb + 5, e);
  };
  for (int x = x0; x < x1; ++x) {
    const int lab = Mr[x];
    if (lab != cur) {
      flush(cur, xs, x - 1);
      cur = lab;
      xs = x;
    }
  }
  flush(cur, xs, x1 - 1);
}

// grid B: bands per label, their exclusive prefix sum (label order) and the job list of image b
__global__ __launch_bounds__(256) void plan_kernel(const int* __restrict__ bbox, int K, int slots, int s_half,
                                                   int* __restrict__ off, int* __restrict__ nb, int2* __restrict__ jobs,
                                                   int* __restrict__ njobs, long long* __restrict__ bandpx) {
  __shared__ long long red[256];
  __shared__ int scan[256];
  __shared__ int base_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  long long a = 0;
  for (int l = tid; l < K; l += 256) {
    Box q;
    if (load_box(bbox + ((size_t)b * K + l) * 6, q)) a += (long long)q.lz * q.ly * q.lx;
  }
  red[tid] = a;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  long long band_px = (red[0] + s_half - 1) / s_half;
  if (band_px < BAND_PX) band_px = BAND_PX;
  if (tid == 0) {
    bandpx[b] = band_px;
    base_s = 0;
  }
  __syncthreads();
  for (int l0 = 0; l0 < K; l0 += 256) {
    const int l = l0 + tid;
    int n = 0;
    Box q;
    if (l < K && load_box(bbox + ((size_t)b * K + l) * 6, q)) {
      const int nrows = q.lz * q.ly;
      const int br = band_rows(band_px, q.lx, nrows);
      n = (nrows + br - 1) / br;
    }
    scan[tid] = n;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int v = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int o = base_s + scan[tid] - n;
    if (l < K) {
      off[(size_t)b * K + l] = o;
      nb[(size_t)b * K + l] = n;
      // o + k < slots by the bound in the header; the guard keeps a broken bound inside the buffer
      for (int k = 0; k < n && o + k < slots; ++k) jobs[(size_t)b * slots + o + k] = make_int2(l, k);
    }
    __syncthreads();
    if (tid == 255) base_s += scan[255];
    __syncthreads();
  }
  if (tid == 0) njobs[b] = min(base_s, slots);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// one wave per (image, job slot).  Lanes cover the box as rpp rows x w columns per step (w = lx
// rounded up to a power of two, at most 64), so narrow boxes keep at least half the lanes busy.
template <bool VOL>
__global__ __launch_bounds__(256) void measure_kernel(const int* __restrict__ M, const float* __restrict__ img, int B, int Z,
                                                      int H, int W, int C, int K, int slots, const int* __restrict__ bbox,
                                                      const int2* __restrict__ jobs, const int* __restrict__ njobs,
                                                      const long long* __restrict__ bandpx, long long* __restrict__ part_i,
                                                      double* __restrict__ part_f, float* __restrict__ part_m,
                                                      unsigned char* __restrict__ outline) {
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= (long long)B * slots) return;
  const int b = (int)(wv / slots), s = (int)(wv % slots);
  if (s >= njobs[b]) return;
  const int2 jb = jobs[wv];
  const int lab = jb.x + 1;
  Box q;
  if (!load_box(bbox + ((size_t)b * K + jb.x) * 6, q)) return;
  const int nrows = q.lz * q.ly;
  const int br = band_rows(bandpx[b], q.lx, nrows);
  const long long r0 = (long long)jb.y * br;
  const long long r1 = min(r0 + br, (long long)nrows);
  const int lg = q.lx >= 64 ? 6 : (q.lx <= 1 ? 0 : 32 - __clz(q.lx - 1));
  const int w = 1 << lg, rpp = 64 >> lg;
  const int lr = lane >> lg, lc = lane & (w - 1);
  const int HW = H * W;
  const size_t vol = (size_t)Z * HW;
  const int* __restrict__ Mb = M + (size_t)b * vol;
  const float* __restrict__ Ib = img ? img + (size_t)b * vol * C : nullptr;
  unsigned char* __restrict__ Ob = outline ? outline + (size_t)b * vol : nullptr;
  const int x1 = q.x0 + q.lx;
  const int ngroups = Ib ? (C + CG - 1) / CG : 1;
  for (int g = 0; g < ngroups; ++g) {
    long long acc[NI];
#pragma unroll
    for (int f = 0; f < NI; ++f) acc[f] = 0;
    double fs[CG], fq[CG];
    float mn[CG], mx[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      fs[c] = 0.0;
      fq[c] = 0.0;
      mn[c] = INFINITY;
      mx[c] = -INFINITY;
    }
    for (long long r = r0 + lr; r < r1; r += rpp) {
      const int ri = (int)r, zz = ri / q.ly;  // r < nrows < 2^31
      const int y = q.y0 + (ri - zz * q.ly), z = q.z0 + zz;
      const int rowoff = (z * H + y) * W;  // < Z * H * W < 2^31
      const int* __restrict__ Mr = Mb + rowoff;
      for (int x = q.x0 + lc; x < x1; x += w) {
        // branch free: the centre, its neighbours and the intensities are independent loads (one
        // round of latency per step); a pixel of another label adds zeros.  -1 = outside the array
        const bool in = Mr[x] == lab;
        if (g == 0) {
          const int nl = x > 0 ? Mr[x - 1] : -1, nr = x < W - 1 ? Mr[x + 1] : -1;
          const int nu = y > 0 ? Mr[x - W] : -1, nd = y < H - 1 ? Mr[x + W] : -1;
          bool bd = nl != lab || nr != lab || nu != lab || nd != lab;
          if (VOL) {
            const int nf = z > 0 ? Mr[x - HW] : -1, nb = z < Z - 1 ? Mr[x + HW] : -1;
            bd = bd || nf != lab || nb != lab;
          }
          bd = bd && in;
          const long long one = in ? 1 : 0, yi = in ? y : 0, xi = in ? x : 0;
          acc[F_AREA] += one;
          acc[F_BND] += bd ? 1 : 0;
          acc[F_SY] += yi;
          acc[F_SX] += xi;
          if (VOL) {
            acc[F_SZ] += in ? z : 0;
          } else {
            acc[F_SYY] += yi * y;
            acc[F_SXX] += xi * x;
            acc[F_SXY] += xi * y;
          }
          if (Ob && bd) Ob[rowoff + x] = 1;
        }
        if (Ib) {
#pragma unroll
          for (int c4 = 0; c4 < CG; ++c4) {
            const int c = g * CG + c4;
            if (c < C) {
              const float v = Ib[((size_t)z * C + c) * HW + (size_t)y * W + x];
              const double d = in ? (double)v : 0.0;
              fs[c4] += d;
              fq[c4] += d * d;  // d * d is exact (24-bit mantissa squared), fused or not
              mn[c4] = fminf(mn[c4], in ? v : INFINITY);
              mx[c4] = fmaxf(mx[c4], in ? v : -INFINITY);
            }
          }
        }
      }
    }
    if (g == 0) {
#pragma unroll
      for (int f = 0; f < NI; ++f) {
        const long long v = wave_sum_i64(acc[f]);
        if (lane == 0) part_i[(size_t)wv * NI + f] = v;
      }
    }
    if (Ib) {
#pragma unroll
      for (int c4 = 0; c4 < CG; ++c4) {
        const int c = g * CG + c4;
        if (c < C) {  // wave-uniform
          const double s1 = wave_sum_f64(fs[c4]), s2 = wave_sum_f64(fq[c4]);
          const float lo = wave_min(mn[c4]), hi = wave_max(mx[c4]);
          if (lane == 0) {
            const size_t o = ((size_t)wv * C + c) * 2;
            part_f[o] = s1;
            part_f[o + 1] = s2;
            part_m[o] = lo;
            part_m[o + 1] = hi;
          }
        }
      }
    }
  }
}

// one thread per (image, label): partials added in band order
__global__ __launch_bounds__(256) void combine_kernel(int B, int K, int C, int slots, const int* __restrict__ bbox,
                                                      const int* __restrict__ off, const int* __restrict__ nb,
                                                      const long long* __restrict__ part_i, const double* __restrict__ part_f,
                                                      const float* __restrict__ part_m, long long* __restrict__ out_i,
                                                      int* __restrict__ out_box, double* __restrict__ out_f,
                                                      float* __restrict__ out_m) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * K) return;
  const int b = (int)(t / K);
  const int o = off[t];
  int n = nb[t];
  if (o + n > slots) n = max(0, slots - o);
  const size_t base = (size_t)b * slots + o;
  long long acc[NI];
#pragma unroll
  for (int f = 0; f < NI; ++f) acc[f] = 0;
  for (int k = 0; k < n; ++k) {
#pragma unroll
    for (int f = 0; f < NI; ++f) acc[f] += part_i[(base + k) * NI + f];
  }
#pragma unroll
  for (int f = 0; f < NI; ++f) out_i[t * NI + f] = acc[f];
  const int* bb = bbox + t * 6;
#pragma unroll
  for (int j = 0; j < 6; ++j) out_box[t * 6 + j] = n > 0 ? bb[j] + (j >= 3 ? 1 : 0) : 0;
  for (int c = 0; c < C; ++c) {
    double s1 = 0.0, s2 = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < n; ++k) {
      const size_t p = ((base + k) * C + c) * 2;
      s1 += part_f[p];
      s2 += part_f[p + 1];
      lo = fminf(lo, part_m[p]);
      hi = fmaxf(hi, part_m[p + 1]);
    }
    const size_t p = ((size_t)t * C + c) * 2;
    out_f[p] = s1;
    out_f[p + 1] = s2;
    out_m[p] = n > 0 ? lo : 0.0f;
    out_m[p + 1] = n > 0 ? hi : 0.0f;
  }
}

}  // namespace

extern "C" {

// M [B, Z, H, W] int32, img [B, Z, C, H, W] fp32 or null (then C is ignored), labels 1..K.
// volume != 0: 6-neighbour boundary and sum_z, no second moments.  Workspaces: bbox [B, K, 6] int32,
// off / nb [B, K] int32, jobs [B, slots] int2, njobs [B] int32, bandpx [B] int64, part_i [B, slots, 8]
// int64, part_f [B, slots, C, 2] fp64, part_m [B, slots, C, 2] fp32; slots >= K + 2 * s_half.
// Outputs (every element written): out_i [B, K, 8] int64 (area, sum_z, sum_y, sum_x, sum_yy, sum_xx,
// sum_xy, boundary), out_box [B, K, 6] int32 half-open (z0, y0, x0, z1, y1, x1), out_f [B, K, C, 2]
// fp64 (sum, sum of squares), out_m [B, K, C, 2] fp32 (min, max); outline [B, Z, H, W] uint8 or
// null: zeroed by the caller, set to 1 at boundary pixels.
int be_cp_measure(const int* M, const float* img, int B, int Z, int H, int W, int C, int K, int volume, int slots,
                  int s_half, int* bbox, int* off, int* nb, void* jobs, int* njobs, long long* bandpx, long long* part_i,
                  double* part_f, float* part_m, long long* out_i, int* out_box, double* out_f, float* out_m,
                  unsigned char* outline, hipStream_t s) {
  if (B <= 0 || K <= 0) return 0;
  if (Z <= 0 || H <= 0 || W <= 0 || s_half < 1 || slots < K + 2 * s_half) return (int)hipErrorInvalidValue;
  if ((long long)Z * H * W >= (1LL << 31)) return (int)hipErrorInvalidValue;
  if (!img) C = 0;
  const long long nbox = (long long)B * K * 6;
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((nbox + 255) / 256)), dim3(256), 0, s, bbox, nbox);
  const long long nseg = (long long)B * Z * H * ((W + RL - 1) / RL);
  hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, s, M, B, Z, H, W, K, bbox);
  hipLaunchKernelGGL(plan_kernel, dim3(B), dim3(256), 0, s, bbox, K, slots, s_half, off, nb, (int2*)jobs, njobs, bandpx);
  const long long nwaves = (long long)B * slots;
  const dim3 grid((unsigned)((nwaves + 3) / 4));
  if (volume)
    hipLaunchKernelGGL((measure_kernel<true>), grid, dim3(256), 0, s, M, img, B, Z, H, W, C, K, slots, bbox, (const int2*)jobs,
                       njobs, bandpx, part_i, part_f, part_m, outline);
  else
    hipLaunchKernelGGL((measure_kernel<false>), grid, dim3(256), 0, s, M, img, B, Z, H, W, C, K, slots, bbox, (const int2*)jobs,
                       njobs, bandpx, part_i, part_f, part_m, outline);
  const long long nrow = (long long)B * K;
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, s, B, K, C, slots, bbox, off, nb,
                     part_i, part_f, part_m, out_i, out_box, out_f, out_m);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
