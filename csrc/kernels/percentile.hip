// Exact per-row percentile normalisation (Cellpose normalize99, SURVEY.md §2.5 K7 / K18:
// x -> (x - p1) / (p99 - p1) with np.percentile 'linear' interpolation per image and channel).
//
// The PyTorch formulation sorts every row (64 rows x 262,144 px for a batch of 32 two-channel 512²
// images: a segmented radix sort with ~1 GB of key/index traffic and large temporaries) only to
// read six order statistics.  Here the six ranks (floor/ceil of each percentile's position, plus
// the min and max for the constant-image test) are found by an MSB-first radix SELECT on
// order-preserving uint32 keys: passes of an 8-bit digit histogram + a per-row select step, four
// for fp32 rows, two for raw uint16 pixels and one for uint8 (percentile.h: the key of an integer
// pixel is the pixel itself, left-aligned).
//
//  * pct_hist_kernel<T>: grid (chunks, rows), 256 threads.  Pass 0 builds ONE 256-bin histogram of
//    the top digit (shared by all six targets); later passes count only the elements whose higher
//    digits equal a target's prefix, into that target's 256 bins.  Histograms live in LDS
//    (6 x 256 x 4 B), flushed once per block with global atomics (non-zero bins only).  A lane
//    loads 16 bytes at a time (4 floats, 8 uint16, 16 uint8) where the row is 16-byte aligned;
//    a chunk's tail and unaligned rows take the scalar loop.  Row r = b * C_use + c reads channel
//    c of image b of a [B, C_src, n] tensor, so the first channels of a wider tensor need no copy.
//  * pct_select_kernel: one block per row: exclusive scan of each target's bins, pick the digit
//    holding the remaining rank, extend the prefix, clear the bins for the next pass.
//  * pct_apply_kernel: decode the six keys, interpolate p_lo / p_hi exactly like the oracle
//    (float32 a*(1-f) + b*f), write the normalised row (float4 vectorised).
//
// Traffic: 4 reads of the input + 1 read + 1 write — ~6 x 4 B per element instead of a full sort.
#include "percentile.h"

namespace {

using namespace be_pct;

constexpr int kThreads = 256;

struct Ranks {
  uint32_t k[kT];
};

// Run-length counters of one lane: runs of equal digits are counted in registers and cost one LDS
// atomic per run.  Image rows are smooth, so a lane's successive elements mostly share the digit,
// and one atomic per element serialised every wave on a handful of bins (0.22 ms per 32-image batch).
struct Run0 {
  uint32_t cd = 0, cc = 0;
  __device__ __forceinline__ void add(uint32_t (*h)[256], uint32_t k) {
    const uint32_t d = k >> 24;
    if (d != cd) {
      if (cc) atomicAdd(&h[0][cd], cc);
      cd = d;
      cc = 0;
    }
    ++cc;
  }
  __device__ __forceinline__ void flush(uint32_t (*h)[256]) {
    if (cc) atomicAdd(&h[0][cd], cc);
  }
};
template <int N>
struct RunT {
  uint32_t cd[N], cc[N];
  __device__ __forceinline__ RunT() {
#pragma unroll
    for (int t = 0; t < N; ++t) { cd[t] = 0; cc[t] = 0; }
  }
  __device__ __forceinline__ void add(uint32_t (*h)[256], uint32_t k, const uint32_t* pre, uint32_t hi_mask, int shift) {
    const uint32_t d = (k >> shift) & 255u;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      if (((k ^ pre[t]) & hi_mask) == 0) {
        if (d != cd[t]) {
          if (cc[t]) atomicAdd(&h[t][cd[t]], cc[t]);
          cd[t] = d;
          cc[t] = 0;
        }
        ++cc[t];
      }
    }
  }
  __device__ __forceinline__ void flush(uint32_t (*h)[256]) {
#pragma unroll
    for (int t = 0; t < N; ++t)
      if (cc[t]) atomicAdd(&h[t][cd[t]], cc[t]);
  }
};
using RunN = RunT<kT>;

// state[r][t] = {prefix, remaining rank}.  `chunk` is a multiple of 16 elements, so a chunk starts
// on a 16-byte boundary of every element type whenever its row does.
template <typename T>
__global__ __launch_bounds__(kThreads) void pct_hist_kernel(const T* __restrict__ x, int C_src, int C_use, long long n,
                                                            int chunk, int pass, const uint32_t* __restrict__ state,
                                                            uint32_t* __restrict__ hist) {
  constexpr int E = Elem<T>::per_vec;
  __shared__ uint32_t h[kT][256];
  const int r = blockIdx.y;
  const int ntg = pass == 0 ? 1 : kT;
  for (int i = threadIdx.x; i < ntg * 256; i += kThreads) (&h[0][0])[i] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  uint32_t pre[kT];
#pragma unroll
  for (int t = 0; t < kT; ++t) pre[t] = state[((size_t)r * kT + t) * 2];
  const T* row = x + ((size_t)(r / C_use) * C_src + r % C_use) * n;
  const long long c0 = (long long)blockIdx.x * chunk;
  const long long c1 = c0 + chunk < n ? c0 + chunk : n;
  const int nvec = (reinterpret_cast<uintptr_t>(row) & 15) == 0 ? (int)((c1 - c0) / E) : 0;
  const u32x4* vrow = reinterpret_cast<const u32x4*>(row + c0);
  if (pass == 0) {
    Run0 run;
    for (int v = threadIdx.x; v < nvec; v += kThreads) {
      const u32x4 w = vrow[v];
#pragma unroll
      for (int e = 0; e < E; ++e) run.add(h, Elem<T>::word_key(w, e));
    }
    for (long long i = c0 + (long long)nvec * E + threadIdx.x; i < c1; i += kThreads) run.add(h, Elem<T>::key(row[i]));
    run.flush(h);
  } else {
    RunN run;
    for (int v = threadIdx.x; v < nvec; v += kThreads) {
      const u32x4 w = vrow[v];
#pragma unroll
      for (int e = 0; e < E; ++e) run.add(h, Elem<T>::word_key(w, e), pre, hi_mask, shift);
    }
    for (long long i = c0 + (long long)nvec * E + threadIdx.x; i < c1; i += kThreads)
      run.add(h, Elem<T>::key(row[i]), pre, hi_mask, shift);
    run.flush(h);
  }
  __syncthreads();
  uint32_t* g = hist + (size_t)r * kT * 256;
  for (int i = threadIdx.x; i < ntg * 256; i += kThreads) {
    const uint32_t v = (&h[0][0])[i];
    if (v) atomicAdd(g + i, v);
  }
}

__global__ __launch_bounds__(kThreads) void pct_select_kernel(int pass, Ranks ranks, uint32_t* __restrict__ state,
                                                              uint32_t* __restrict__ hist) {
  __shared__ uint32_t scan[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int shift = 24 - 8 * pass;
  uint32_t* g = hist + (size_t)r * kT * 256;
  for (int t = 0; t < kT; ++t) {
    const uint32_t c = g[(pass == 0 ? 0 : t) * 256 + tid];
    scan[tid] = c;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // Hillis-Steele inclusive scan
      const uint32_t v = tid >= o ? scan[tid - o] : 0u;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    uint32_t* st = state + ((size_t)r * kT + t) * 2;
    const uint32_t rank = pass == 0 ? ranks.k[t] : st[1];
    const uint32_t incl = scan[tid], excl = incl - c;
    __syncthreads();
    if (c > 0 && excl <= rank && rank < incl) {
      st[0] = (pass == 0 ? 0u : st[0]) | ((uint32_t)tid << shift);
      st[1] = rank - excl;
    }
    __syncthreads();
  }
  for (int t = 0; t < kT; ++t) g[t * 256 + tid] = 0;  // ready for the next pass / next call
}

__global__ __launch_bounds__(kThreads) void pct_apply_kernel(const float* __restrict__ x, long long n, int chunk,
                                                             const Coef cf, const uint32_t* __restrict__ state,
                                                             float* __restrict__ out) {
  const int r = blockIdx.y;
  float p1, scale;
  bool cst;
  row_consts<float>(state + (size_t)r * kT * 2, cf, p1, scale, cst);
  const float* row = x + (size_t)r * n;
  float* orow = out + (size_t)r * n;
  const long long c0 = (long long)blockIdx.x * chunk;
  const long long c1 = c0 + chunk < n ? c0 + chunk : n;
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    for (long long i = c0 + 4 * threadIdx.x; i < c1; i += 4 * kThreads) {
      float4 v = *reinterpret_cast<const float4*>(row + i);
      v.x = cst ? 0.f : (v.x - p1) * scale;
      v.y = cst ? 0.f : (v.y - p1) * scale;
      v.z = cst ? 0.f : (v.z - p1) * scale;
      v.w = cst ? 0.f : (v.w - p1) * scale;
      *reinterpret_cast<float4*>(orow + i) = v;
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c1; i += kThreads) orow[i] = cst ? 0.f : (row[i] - p1) * scale;
  }
}

// ~2 k-element chunks per block, at most 64 blocks per row (>= 256 CUs busy for batches >= 4 rows);
// a multiple of 16 elements (pct_hist_kernel's vector loads, pct_apply_kernel's float4)
int chunk_of(long long n) {
  int chunks = (int)((n + 4095) / 4096);
  if (chunks > 64) chunks = 64;
  const int chunk = (int)((n + chunks - 1) / chunks);
  return (chunk + 15) & ~15;
}

template <typename T>
void select_passes(const void* x, int C_src, int C_use, int rows, long long n, const Ranks& rk, uint32_t* state,
                   uint32_t* hist, hipStream_t s) {
  const int chunk = chunk_of(n);
  const dim3 grid((unsigned)((n + chunk - 1) / chunk), rows);
  for (int pass = 0; pass < Elem<T>::passes; ++pass) {
    hipLaunchKernelGGL(pct_hist_kernel<T>, grid, dim3(kThreads), 0, s, static_cast<const T*>(x), C_src, C_use, n, chunk,
                       pass, state, hist);
    hipLaunchKernelGGL(pct_select_kernel, dim3(rows), dim3(kThreads), 0, s, pass, rk, state, hist);
  }
}

// ---- local (tile) normalisation: percentiles of overlapping blocks, the maps they become, the apply
//
//  * pct_block_kernel<T>: one workgroup per (block, image-channel).  A block is a bh x bw rectangle
//    of a plane, so its rows are strided and generally unaligned: scalar loads, a lane on kSeg
//    consecutive pixels of a row per step.  The whole select runs inside the workgroup: per digit pass the rectangle is re-read
//    from global memory (it was just read, it sits in L2), counted into LDS histograms with the
//    run-length counters above, and the four targets are selected in LDS.  No rectangle is ever held
//    in LDS, so one path serves every block size, and no global workspace is needed.
//  * pct_maps_kernel: one workgroup per (image, channel), the block grid in LDS: degenerate blocks
//    take the values of the nearest valid block, then a 9-tap Gaussian (sigma 1, reflect boundary)
//    along each axis, accumulated in fp64 and rounded to fp32 per axis as scipy's filter does.
//  * pct_apply_ext_kernel<T>: the unfused apply of every NormExt rule (percentile.h), raw in, fp32 out.
constexpr int kSeg = 8;  // consecutive pixels per lane and step of the block select
constexpr int kBT = 4;  // lo(p_lower), hi(p_lower), lo(p_upper), hi(p_upper)

struct BlockRanks {
  uint32_t k[kBT];
};

struct Gauss9 {
  double w[5];  // weight at distance |d| <= 4
};

void ranks_of(long long n, float lower, float upper, uint32_t* k, Coef* cf) {
  const double pos_lo = lower / 100.0 * (double)(n - 1), pos_hi = upper / 100.0 * (double)(n - 1);
  const long long lo0 = (long long)pos_lo, lo1 = (long long)pos_hi;
  k[0] = (uint32_t)lo0;
  k[1] = (uint32_t)(lo0 + 1 < n ? lo0 + 1 : n - 1);
  k[2] = (uint32_t)lo1;
  k[3] = (uint32_t)(lo1 + 1 < n ? lo1 + 1 : n - 1);
  const double f_lo = pos_lo - (double)lo0, f_hi = pos_hi - (double)lo1;
  *cf = Coef{(float)(1.0 - f_lo), (float)f_lo, (float)(1.0 - f_hi), (float)f_hi};
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pct_block_kernel(const T* __restrict__ x, int C_src, int C_use, int H, int W,
                                                             const int* __restrict__ ys, const int* __restrict__ xs, int nx,
                                                             int bh, int bw, const BlockRanks ranks, const Coef cf,
                                                             float* __restrict__ lo_out, float* __restrict__ hi_out) {
  __shared__ uint32_t h[kBT][256];
  __shared__ uint32_t scan[kBT][256];
  __shared__ uint32_t s_pre[kBT], s_rank[kBT];
  const int tid = threadIdx.x, r = blockIdx.y;
  const int gy = blockIdx.x / nx, gx = blockIdx.x - gy * nx;
  const T* base = x + ((size_t)(r / C_use) * C_src + r % C_use) * H * W + (size_t)ys[gy] * W + xs[gx];
  // a lane counts kSeg consecutive pixels of one rectangle row at a time (neighbours share their
  // digits, so the run-length counters see runs); consecutive lanes take consecutive segments
  const int segs = (bw + kSeg - 1) / kSeg, items = bh * segs;
  if (tid < kBT) {
    s_pre[tid] = 0;
    s_rank[tid] = ranks.k[tid];
  }
  for (int pass = 0; pass < Elem<T>::passes; ++pass) {
    const int ntg = pass == 0 ? 1 : kBT;
    for (int i = tid; i < ntg * 256; i += kThreads) (&h[0][0])[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    if (pass == 0) {
      Run0 run;
      for (int i = tid; i < items; i += kThreads) {
        const int yy = i / segs, x0 = (i - yy * segs) * kSeg;
        const T* row = base + (size_t)yy * W;
        const int x1 = x0 + kSeg < bw ? x0 + kSeg : bw;
        for (int xx = x0; xx < x1; ++xx) run.add(h, Elem<T>::key(row[xx]));
      }
      run.flush(h);
    } else {
      uint32_t pre[kBT];
#pragma unroll
      for (int t = 0; t < kBT; ++t) pre[t] = s_pre[t];
      RunT<kBT> run;
      for (int i = tid; i < items; i += kThreads) {
        const int yy = i / segs, x0 = (i - yy * segs) * kSeg;
        const T* row = base + (size_t)yy * W;
        const int x1 = x0 + kSeg < bw ? x0 + kSeg : bw;
        for (int xx = x0; xx < x1; ++xx) run.add(h, Elem<T>::key(row[xx]), pre, hi_mask, shift);
      }
      run.flush(h);
    }
    __syncthreads();
    // the four targets are scanned side by side: one set of barriers per pass, not one per target
    uint32_t c[kBT];
#pragma unroll
    for (int t = 0; t < kBT; ++t) {
      c[t] = h[pass == 0 ? 0 : t][tid];
      scan[t][tid] = c[t];
    }
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // Hillis-Steele inclusive scan
      uint32_t v[kBT];
#pragma unroll
      for (int t = 0; t < kBT; ++t) v[t] = tid >= o ? scan[t][tid - o] : 0u;
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kBT; ++t) scan[t][tid] += v[t];
      __syncthreads();
    }
    uint32_t rank[kBT];
#pragma unroll
    for (int t = 0; t < kBT; ++t) rank[t] = s_rank[t];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kBT; ++t) {
      const uint32_t incl = scan[t][tid], excl = incl - c[t];
      if (c[t] > 0 && excl <= rank[t] && rank[t] < incl) {  // exactly one lane per target
        s_pre[t] |= (uint32_t)tid << shift;
        s_rank[t] = rank[t] - excl;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    // a percentile whose two ranks hold one value is that value; otherwise the weights of row_consts
    const float a0 = Elem<T>::val(s_pre[0]), a1 = Elem<T>::val(s_pre[1]);
    const float b0 = Elem<T>::val(s_pre[2]), b1 = Elem<T>::val(s_pre[3]);
    const size_t o = (size_t)r * gridDim.x + blockIdx.x;
    lo_out[o] = a0 == a1 ? a0 : fmaf(a0, cf.a_lo, a1 * cf.b_lo);
    hi_out[o] = b0 == b1 ? b0 : fmaf(b0, cf.a_hi, b1 * cf.b_hi);
  }
}

// scipy's 'reflect' boundary (d c b a | a b c d | d c b a), for any index and any n >= 1
__device__ __forceinline__ int reflect_idx(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// src -> dst, one axis: centre first, then the pairs from the outside in, as scipy's symmetric
// correlate1d sums them
__device__ __forceinline__ void smooth_axis(const float* src, float* dst, int ny, int nx, bool along_y, const Gauss9& g) {
  for (int i = threadIdx.x; i < ny * nx; i += kThreads) {
    const int y = i / nx, xq = i - y * nx;
    double acc = (double)src[i] * g.w[0];
    for (int d = 4; d >= 1; --d) {
      const int ia = along_y ? reflect_idx(y - d, ny) * nx + xq : y * nx + reflect_idx(xq - d, nx);
      const int ib = along_y ? reflect_idx(y + d, ny) * nx + xq : y * nx + reflect_idx(xq + d, nx);
      acc += ((double)src[ia] + (double)src[ib]) * g.w[d];
    }
    dst[i] = (float)acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void pct_maps_kernel(float* __restrict__ lo_g, float* __restrict__ hi_g, int ny, int nx,
                                                            const Gauss9 g) {
  __shared__ float lo[kMaxCells], hi[kMaxCells], tmp[kMaxCells];
  __shared__ unsigned char ok[kMaxCells];
  const int n = ny * nx, tid = threadIdx.x;
  float* lo_r = lo_g + (size_t)blockIdx.x * n;
  float* hi_r = hi_g + (size_t)blockIdx.x * n;
  int any = 0;
  for (int i = tid; i < n; i += kThreads) {
    lo[i] = lo_r[i];
    hi[i] = hi_r[i];
    ok[i] = !(hi[i] - lo[i] < 1e-3f);
    any |= ok[i];
  }
  any = __syncthreads_or(any);
  for (int i = tid; i < n; i += kThreads) {
    if (ok[i]) continue;
    if (!any) {  // no valid block in this channel: the identity
      lo[i] = 0.f;
      hi[i] = 1.f;
      continue;
    }
    // nearest valid block by squared grid distance; raster-first on ties (strict <).  Valid cells
    // are only read and degenerate cells only written, so the search needs no second buffer.
    const int y = i / nx, xq = i - y * nx;
    int best = 0x7fffffff, bj = 0;
    for (int j = 0; j < n; ++j) {
      if (!ok[j]) continue;
      const int ddy = j / nx - y, ddx = j % nx - xq;
      const int d2 = ddy * ddy + ddx * ddx;
      if (d2 < best) { best = d2; bj = j; }
    }
    lo[i] = lo[bj];
    hi[i] = hi[bj];
  }
  __syncthreads();
  smooth_axis(lo, tmp, ny, nx, true, g);
  smooth_axis(tmp, lo, ny, nx, false, g);
  smooth_axis(hi, tmp, ny, nx, true, g);
  smooth_axis(tmp, hi, ny, nx, false, g);
  for (int i = tid; i < n; i += kThreads) {
    lo_r[i] = lo[i];
    hi_r[i] = hi[i];
  }
}

// grid (x blocks, H, B * C_use): x [B, C_src, H, W] raw -> out [B, C_use, H, W] fp32
template <typename T>
__global__ __launch_bounds__(kThreads) void pct_apply_ext_kernel(const T* __restrict__ x, int C_src, int C_use, int H, int W,
                                                                 const Coef cf, const uint32_t* __restrict__ state,
                                                                 const NormExt ext, float* __restrict__ out) {
  const int xx = blockIdx.x * kThreads + threadIdx.x, yy = blockIdx.y, r = blockIdx.z;
  if (xx >= W) return;
  const int c = r % C_use;
  const float v = (float)x[(((size_t)(r / C_use) * C_src + c) * H + yy) * W + xx];
  float res;
  if (ext.lo_map) {
    int y0, y1, x0, x1;
    float wy, wx;
    map_coord(yy, ext.sy, ext.ny, y0, y1, wy);
    map_coord(xx, ext.sx, ext.nx, x0, x1, wx);
    const size_t mo = (size_t)r * ext.ny * ext.nx;
    res = tile_norm(v, ext.lo_map + mo, ext.hi_map + mo, ext.nx, y0, y1, wy, x0, x1, wx, ext.invert != 0);
  } else {
    float lo, den;
    bool cst;
    ext_consts<T>(ext, ext.lowhigh ? nullptr : state + (size_t)r * kT * 2, cf, c, lo, den, cst);
    res = norm_div(v, lo, den, cst, ext.invert != 0);
  }
  out[((size_t)r * H + yy) * W + xx] = res;
}

bool image_args_ok(int dtype, int B, int C_src, int C_use, int H, int W) {
  return (dtype == kF32 || dtype == kU16 || dtype == kU8) && B > 0 && C_use > 0 && C_use <= C_src && H > 0 && W > 0 &&
         H <= 65535 && (long long)B * C_use <= 65535 && (long long)H * W <= 0x7fffffffLL;
}

int apply_ext_launch(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, const Coef cf,
                     const uint32_t* state, const NormExt& ext, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((W + kThreads - 1) / kThreads), H, B * C_use);
  if (dtype == kF32)
    hipLaunchKernelGGL(pct_apply_ext_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<const float*>(x), C_src, C_use, H, W,
                       cf, state, ext, out);
  else if (dtype == kU16)
    hipLaunchKernelGGL(pct_apply_ext_kernel<uint16_t>, grid, dim3(kThreads), 0, s, static_cast<const uint16_t*>(x), C_src, C_use,
                       H, W, cf, state, ext, out);
  else
    hipLaunchKernelGGL(pct_apply_ext_kernel<uint8_t>, grid, dim3(kThreads), 0, s, static_cast<const uint8_t*>(x), C_src, C_use, H,
                       W, cf, state, ext, out);
  return BE_CHECK_LAUNCH();
}

}  // namespace

namespace be_pct {

int select_run(const void* x, int dtype, int B, int C_src, int C_use, long long n, float lower, float upper, void* ws,
               long long ws_bytes, hipStream_t s, Coef* cf, const uint32_t** state_out) {
  if (B <= 0 || C_use <= 0 || C_use > C_src || n <= 0 || n > 0xffffffffLL) return -1;
  const long long rows = (long long)B * C_use;
  if (rows > 65535) return -1;
  if (dtype != kF32 && dtype != kU16 && dtype != kU8) return -3;
  if (ws_bytes < rows * kT * (256 + 2) * 4) return -2;
  uint32_t* hist = static_cast<uint32_t*>(ws);
  uint32_t* state = hist + ws_bytes / 4 - (size_t)rows * kT * 2;
  const double pos_lo = lower / 100.0 * (double)(n - 1), pos_hi = upper / 100.0 * (double)(n - 1);
  const long long lo0 = (long long)pos_lo, lo1 = (long long)pos_hi;
  Ranks rk;
  rk.k[0] = (uint32_t)lo0;
  rk.k[1] = (uint32_t)(lo0 + 1 < n ? lo0 + 1 : n - 1);
  rk.k[2] = (uint32_t)lo1;
  rk.k[3] = (uint32_t)(lo1 + 1 < n ? lo1 + 1 : n - 1);
  rk.k[4] = 0;
  rk.k[5] = (uint32_t)(n - 1);
  const double f_lo = pos_lo - (double)lo0, f_hi = pos_hi - (double)lo1;
  *cf = Coef{(float)(1.0 - f_lo), (float)f_lo, (float)(1.0 - f_hi), (float)f_hi};
  *state_out = state;
  if (dtype == kF32)
    select_passes<float>(x, C_src, C_use, (int)rows, n, rk, state, hist, s);
  else if (dtype == kU16)
    select_passes<uint16_t>(x, C_src, C_use, (int)rows, n, rk, state, hist, s);
  else
    select_passes<uint8_t>(x, C_src, C_use, (int)rows, n, rk, state, hist, s);
  return 0;
}

}  // namespace be_pct

extern "C" {

// Workspace bytes for `rows` rows (hist + state).  The workspace must be zero before its first use;
// histograms live at its start and are left zeroed by every call, the per-row state at its END, so
// calls with different row counts sharing one workspace never see each other's state as counts.
int be_pct_workspace_bytes(int rows, long long* out) {
  if (rows <= 0 || !out) return -1;
  *out = (long long)rows * kT * (256 + 2) * 4;
  return 0;
}

// x, out: [rows, n] float32 (out may alias x).  lower/upper in percent.
int be_pct_normalize(const float* x, int rows, long long n, float lower, float upper, float* out, void* ws,
                     long long ws_bytes, hipStream_t s) {
  be_pct::Coef cf;
  const uint32_t* state;
  const int rc = be_pct::select_run(x, be_pct::kF32, rows, 1, 1, n, lower, upper, ws, ws_bytes, s, &cf, &state);
  if (rc) return rc;
  const int chunk = chunk_of(n);
  hipLaunchKernelGGL(pct_apply_kernel, dim3((unsigned)((n + chunk - 1) / chunk), rows), dim3(kThreads), 0, s, x, n, chunk,
                     cf, state, out);
  return BE_CHECK_LAUNCH();
}

// Percentiles of the ny x nx blocks of every (image, channel): x raw [B, C_src, H, W] of element
// type `dtype`, block (gy, gx) is the bh x bw rectangle at (ys[gy], xs[gx]) (device int arrays; the
// caller guarantees ys[.] + bh <= H, xs[.] + bw <= W).  lo / hi: [B * C_use, ny, nx] fp32.
int be_pct_block_select(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, const int* ys, const int* xs,
                        int ny, int nx, int bh, int bw, float lower, float upper, float* lo, float* hi, hipStream_t s) {
  if (!image_args_ok(dtype, B, C_src, C_use, H, W) || ny <= 0 || nx <= 0 || (long long)ny * nx > be_pct::kMaxCells || bh <= 0 ||
      bw <= 0 || bh > H || bw > W || !(lower >= 0.f && lower < upper && upper <= 100.f))
    return -1;
  BlockRanks rk;
  be_pct::Coef cf;
  ranks_of((long long)bh * bw, lower, upper, rk.k, &cf);
  const dim3 grid(ny * nx, B * C_use);
  if (dtype == be_pct::kF32)
    hipLaunchKernelGGL(pct_block_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<const float*>(x), C_src, C_use, H, W, ys,
                       xs, nx, bh, bw, rk, cf, lo, hi);
  else if (dtype == be_pct::kU16)
    hipLaunchKernelGGL(pct_block_kernel<uint16_t>, grid, dim3(kThreads), 0, s, static_cast<const uint16_t*>(x), C_src, C_use, H,
                       W, ys, xs, nx, bh, bw, rk, cf, lo, hi);
  else
    hipLaunchKernelGGL(pct_block_kernel<uint8_t>, grid, dim3(kThreads), 0, s, static_cast<const uint8_t*>(x), C_src, C_use, H, W,
                       ys, xs, nx, bh, bw, rk, cf, lo, hi);
  return BE_CHECK_LAUNCH();
}

// Block percentiles -> the maps the apply samples, in place: lo / hi [rows, ny, nx] fp32.  w0..w4:
// the Gaussian's weights at distance 0..4 (sigma 1, normalised over the 9 taps), from the host.
int be_pct_tile_maps(float* lo, float* hi, int rows, int ny, int nx, double w0, double w1, double w2, double w3, double w4,
                     hipStream_t s) {
  if (rows <= 0 || ny <= 0 || nx <= 0 || (long long)ny * nx > be_pct::kMaxCells) return -1;
  hipLaunchKernelGGL(pct_maps_kernel, dim3(rows), dim3(kThreads), 0, s, lo, hi, ny, nx, Gauss9{{w0, w1, w2, w3, w4}});
  return BE_CHECK_LAUNCH();
}

// Unfused tile normalisation: x raw [B, C_src, H, W] -> out [B, C_use, H, W] fp32 against the maps
// of be_pct_tile_maps, exactly what be_tiles_gather_tilenorm computes per pixel.
int be_pct_normalize_tile(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, const float* lo_map,
                          const float* hi_map, int ny, int nx, int invert, float* out, hipStream_t s) {
  if (!image_args_ok(dtype, B, C_src, C_use, H, W) || ny <= 0 || nx <= 0 || (long long)ny * nx > be_pct::kMaxCells || !lo_map ||
      !hi_map)
    return -1;
  be_pct::NormExt ext;
  ext.lo_map = lo_map;
  ext.hi_map = hi_map;
  ext.ny = ny;
  ext.nx = nx;
  ext.sy = (float)((double)ny / H);
  ext.sx = (float)((double)nx / W);
  ext.invert = invert;
  return apply_ext_launch(x, dtype, B, C_src, C_use, H, W, be_pct::Coef{}, nullptr, ext, out, s);
}

// Unfused global rules with the options of NormExt: percentiles `lower` / `upper` per (image,
// channel), or the fixed bounds lowhigh [C_use][2] (device; no select runs), then the inversion.
// ws: as be_pct_normalize (unused with lowhigh).
int be_pct_normalize_ext(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, float lower, float upper,
                         const float* lowhigh, int invert, float* out, void* ws, long long ws_bytes, hipStream_t s) {
  if (!image_args_ok(dtype, B, C_src, C_use, H, W)) return -1;
  be_pct::NormExt ext;
  ext.lowhigh = lowhigh;
  ext.invert = invert;
  be_pct::Coef cf{};
  const uint32_t* state = nullptr;
  if (!lowhigh) {
    const int rc = be_pct::select_run(x, dtype, B, C_src, C_use, (long long)H * W, lower, upper, ws, ws_bytes, s, &cf, &state);
    if (rc) return rc;
  }
  return apply_ext_launch(x, dtype, B, C_src, C_use, H, W, cf, state, ext, out, s);
}

}  // extern "C"
