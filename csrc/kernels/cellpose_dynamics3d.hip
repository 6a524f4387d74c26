// Cellpose do_3D on the GPU: orthogonal-view accumulation, 3-D flow following, 5x5x5 histogram seeds
// and 11x11x11 seed expansion.  The 2-D stages of cellpose_dynamics.hip with one more axis; the
// semantics are those of bioengine_worker_amd/cellpose/reference.py (combine_views3d,
// follow_flows3d, get_masks3d), which the GPU tests compare against.
//
// MI355X mapping:
//  * accum_view3d: the network runs on the YX, ZX and ZY planes of a volume in chunks; each chunk is
//    added into one [4, Z, H, W] fp32 accumulator (dZ, dY, dX, cellprob) as soon as it exists, so
//    the three view outputs never live together.  One thread per voxel and call, no atomics.  YX and
//    ZX are contiguous along x on both sides; ZY reads along y and writes along the plane index (x)
//    through a 32 x 33 LDS tile so both sides stay coalesced.
//  * prep_flow3d: the field the dynamics read is float4 (dz, dy, dx, 0) * fg / 5 -- one 16-byte
//    gather per trilinear corner.
//  * follow_flows3d: one lane per foreground voxel, position in registers for all niter steps, eight
//    float4 corner gathers per step, the end point binned into the padded histogram with one integer
//    atomic.  A workgroup compacts the foreground of its 256 consecutive voxels in LDS so the Euler
//    loop runs on full waves, and workgroups are ordered so one XCD walks one contiguous z-slab
//    (its L2 then holds that slab's field).  An LDS-staged window as in the 2-D kernel does not
//    fit: an 8^3 tile with an 8-voxel margin is 24^3 x 16 B = 221 KB against 160 KiB of LDS per CU.
//    The gathers stay in L2: measured on a 64 x 256 x 256 volume (298k foreground voxels, niter 200)
//    they run at 8.8 TB/s, above the HBM rate, so the stage is bound by the latency of its 200
//    dependent steps and not by traffic (tools/cellpose3d_bench.py; 0.87 ms, plain launch 0.93 ms).
//  * seeds3d: 5x5x5 local-max test only for voxels with h > 10 (a handful per cell), compacted into
//    count << 32 | raster index keys that torch.sort orders like the oracle's lexsort.
//  * expand3d: one wave per seed; the 11^3 window is 121 rows of 11 bits, two rows per lane, in LDS.
//    A 3x3x3 dilation is (r | r << 1 | r >> 1) or-ed over the 3x3 neighbouring rows, and-ed with the
//    support row.  Commit with atomicMax of rank + 1 (later seeds overwrite earlier ones).
// No kernel here waits on another workgroup; every loop is bounded by niter, the window or the grid.
#include "common.h"

namespace {

constexpr int RPAD = 20;

// ------------------------------------------------------------------ views -> accumulator

// view 0 (YX): y [n, 3, H, W], plane p0 + i is z.  Writes dY, dX, cellprob and zeroes dZ.
__global__ __launch_bounds__(256) void accum_yx_kernel(const float* __restrict__ y, int p0, int n, int Z, int H, int W,
                                                       float* __restrict__ acc) {
  const size_t HW = (size_t)H * W, N = (size_t)Z * HW;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * HW) return;
  const size_t i = e / HW, q = e - i * HW;
  const float* src = y + i * 3 * HW + q;
  const size_t v = (size_t)(p0 + i) * HW + q;
  acc[v] = 0.f;
  acc[N + v] = src[0];
  acc[2 * N + v] = src[HW];
  acc[3 * N + v] = src[2 * HW];
}

// view 1 (ZX): y [n, 3, Z, W], plane p0 + i is y.  Adds dZ (rows), dX (columns), cellprob.
__global__ __launch_bounds__(256) void accum_zx_kernel(const float* __restrict__ y, int p0, int n, int Z, int H, int W,
                                                       float* __restrict__ acc) {
  const size_t ZW = (size_t)Z * W, N = (size_t)Z * H * W;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * ZW) return;
  const size_t i = e / ZW, q = e - i * ZW;
  const size_t z = q / W, x = q - z * W;
  const float* src = y + i * 3 * ZW + q;
  const size_t v = (z * H + (size_t)(p0 + i)) * W + x;
  acc[v] += src[0];
  acc[2 * N + v] += src[ZW];
  acc[3 * N + v] += src[2 * ZW];
}

// view 2 (ZY): y [n, 3, Z, H], plane p0 + i is x.  Adds dZ (rows), dY (columns), cellprob.  A
// 32 (planes) x 32 (y) tile per (z, channel) goes through LDS: read along y, written along x.
__global__ __launch_bounds__(256) void accum_zy_kernel(const float* __restrict__ y, int p0, int n, int Z, int H, int W,
                                                       float* __restrict__ acc) {
  __shared__ float tile[3][32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int yb = blockIdx.x * 32, ib = blockIdx.y * 32, z = blockIdx.z;
  const size_t ZH = (size_t)Z * H, N = ZH * W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = ib + ty + 8 * k, yy = yb + tx;
    if (i < n && yy < H) {
      const float* src = y + (size_t)i * 3 * ZH + (size_t)z * H + yy;
      tile[0][ty + 8 * k][tx] = src[0];
      tile[1][ty + 8 * k][tx] = src[ZH];
      tile[2][ty + 8 * k][tx] = src[2 * ZH];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = yb + ty + 8 * k, i = ib + tx;
    if (i < n && yy < H) {
      const size_t v = ((size_t)z * H + yy) * W + (size_t)(p0 + i);
      acc[v] += tile[0][tx][ty + 8 * k];
      acc[N + v] += tile[1][tx][ty + 8 * k];
      acc[3 * N + v] += tile[2][tx][ty + 8 * k];
    }
  }
}

// acc [4, N] (dZ, dY, dX, cellprob) -> flow4 [N] = (dz, dy, dx, 0) * fg / 5, fg [N] uint8.
__global__ __launch_bounds__(256) void prep_flow3d_kernel(const float* __restrict__ acc, long long N, float thr,
                                                          float4* __restrict__ flow4, uint8_t* __restrict__ fg) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= N) return;
  const bool f = acc[3 * N + v] > thr;
  fg[v] = f;
  flow4[v] = f ? make_float4(acc[v] / 5.0f, acc[N + v] / 5.0f, acc[2 * N + v] / 5.0f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------ dynamics

struct Vol {
  int Z, H, W;
  float sz, sy, sx;  // sample position = p * s - o  (L / (L - 1) and 0.5; 0 and 0 for an axis of length 1)
  float oz, oy, ox;
};

__device__ __forceinline__ Vol make_vol(int Z, int H, int W) {
  Vol g;
  g.Z = Z; g.H = H; g.W = W;
  g.sz = Z > 1 ? (float)Z / (float)(Z - 1) : 0.f;
  g.sy = H > 1 ? (float)H / (float)(H - 1) : 0.f;
  g.sx = W > 1 ? (float)W / (float)(W - 1) : 0.f;
  g.oz = Z > 1 ? 0.5f : 0.f;
  g.oy = H > 1 ? 0.5f : 0.f;
  g.ox = W > 1 ? 0.5f : 0.f;
  return g;
}

__device__ __forceinline__ float4 ldflow3(const float4* __restrict__ f, const Vol& g, int z, int y, int x) {
  if ((unsigned)z >= (unsigned)g.Z || (unsigned)y >= (unsigned)g.H || (unsigned)x >= (unsigned)g.W)
    return make_float4(0.f, 0.f, 0.f, 0.f);
  return f[((size_t)z * g.H + y) * g.W + x];
}

// The dynamics of one voxel: every float operation and its order is fixed here (explicit fmaf, so the
// compiler has nothing left to contract differently between launch variants).  Returns the padded
// linear index of the end point's bin.
__device__ __forceinline__ int follow_one3d(const float4* __restrict__ f, const Vol& g, int vz, int vy, int vx, int niter) {
  float pz = (float)vz, py = (float)vy, px = (float)vx;
  const float zmax = (float)(g.Z - 1), ymax = (float)(g.H - 1), xmax = (float)(g.W - 1);
  for (int t = 0; t < niter; ++t) {
    const float qz = fmaf(pz, g.sz, -g.oz), qy = fmaf(py, g.sy, -g.oy), qx = fmaf(px, g.sx, -g.ox);
    const float fz = floorf(qz), fy = floorf(qy), fx = floorf(qx);
    const int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
    const float wz = qz - fz, wy = qy - fy, wx = qx - fx;
    const float uz = 1.f - wz, uy = 1.f - wy, ux = 1.f - wx;
    const float4 c000 = ldflow3(f, g, z0, y0, x0), c001 = ldflow3(f, g, z0, y0, x0 + 1);
    const float4 c010 = ldflow3(f, g, z0, y0 + 1, x0), c011 = ldflow3(f, g, z0, y0 + 1, x0 + 1);
    const float4 c100 = ldflow3(f, g, z0 + 1, y0, x0), c101 = ldflow3(f, g, z0 + 1, y0, x0 + 1);
    const float4 c110 = ldflow3(f, g, z0 + 1, y0 + 1, x0), c111 = ldflow3(f, g, z0 + 1, y0 + 1, x0 + 1);
    const float a00 = uz * uy, a01 = uz * wy, a10 = wz * uy, a11 = wz * wy;
    const float w000 = a00 * ux, w001 = a00 * wx, w010 = a01 * ux, w011 = a01 * wx;
    const float w100 = a10 * ux, w101 = a10 * wx, w110 = a11 * ux, w111 = a11 * wx;
    float dz = c000.x * w000, dy = c000.y * w000, dx = c000.z * w000;
    dz = fmaf(c001.x, w001, dz); dy = fmaf(c001.y, w001, dy); dx = fmaf(c001.z, w001, dx);
    dz = fmaf(c010.x, w010, dz); dy = fmaf(c010.y, w010, dy); dx = fmaf(c010.z, w010, dx);
    dz = fmaf(c011.x, w011, dz); dy = fmaf(c011.y, w011, dy); dx = fmaf(c011.z, w011, dx);
    dz = fmaf(c100.x, w100, dz); dy = fmaf(c100.y, w100, dy); dx = fmaf(c100.z, w100, dx);
    dz = fmaf(c101.x, w101, dz); dy = fmaf(c101.y, w101, dy); dx = fmaf(c101.z, w101, dx);
    dz = fmaf(c110.x, w110, dz); dy = fmaf(c110.y, w110, dy); dx = fmaf(c110.z, w110, dx);
    dz = fmaf(c111.x, w111, dz); dy = fmaf(c111.y, w111, dy); dx = fmaf(c111.z, w111, dx);
    pz = fminf(fmaxf(pz + dz, 0.f), zmax);
    py = fminf(fmaxf(py + dy, 0.f), ymax);
    px = fminf(fmaxf(px + dx, 0.f), xmax);
  }
  const int Hp = g.H + 2 * RPAD, Wp = g.W + 2 * RPAD;
  const int iz = min(max((int)pz + RPAD, 0), g.Z + RPAD - 1);
  const int iy = min(max((int)py + RPAD, 0), g.H + RPAD - 1);
  const int ix = min(max((int)px + RPAD, 0), g.W + RPAD - 1);
  return (iz * Hp + iy) * Wp + ix;  // < (Z+40)(H+40)(W+40) < 2^31 (checked by the caller)
}

__device__ __forceinline__ void follow_voxel3d(const float4* __restrict__ f, const Vol& g, int v, int niter,
                                               int* __restrict__ hist, int* __restrict__ pos) {
  const int HW = g.H * g.W;
  const int vz = v / HW, r = v - vz * HW;
  const int lin = follow_one3d(f, g, vz, r / g.W, r % g.W, niter);
  pos[v] = lin;
  atomicAdd(hist + lin, 1);
}

// Plain launch: one lane per voxel, background lanes idle through the Euler loop.
__global__ __launch_bounds__(256) void follow_flows3d_plain_kernel(const float4* __restrict__ flow4,
                                                                   const uint8_t* __restrict__ fg, int* __restrict__ hist,
                                                                   int* __restrict__ pos, int Z, int H, int W, int niter) {
  const long long n = (long long)Z * H * W;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  if (!fg[v]) {
    pos[v] = -1;
    return;
  }
  const Vol g = make_vol(Z, H, W);
  follow_voxel3d(flow4, g, (int)v, niter, hist, pos);
}

// Default launch: XCD-ordered workgroups (an XCD walks one contiguous z-slab), the workgroup's
// foreground voxels compacted in LDS so the Euler loop runs on full waves.
__global__ __launch_bounds__(256) void follow_flows3d_xcd_kernel(const float4* __restrict__ flow4,
                                                                 const uint8_t* __restrict__ fg, int* __restrict__ hist,
                                                                 int* __restrict__ pos, int Z, int H, int W, int niter) {
  __shared__ int list[256];
  __shared__ int wcount[4];
  const long long n = (long long)Z * H * W;
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  const long long v0 = (long long)blk * 256;
  const long long v = v0 + threadIdx.x;
  const bool in = v < n;
  const bool f = in && fg[v];
  if (in && !f) pos[v] = -1;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  if (lane == 0) wcount[wv] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int i = 0; i < wv; ++i) base += wcount[i];
  const int total = wcount[0] + wcount[1] + wcount[2] + wcount[3];
  if (f) list[base + __popcll(m & ((1ull << lane) - 1ull))] = threadIdx.x;
  __syncthreads();
  if ((int)threadIdx.x >= total) return;
  const Vol g = make_vol(Z, H, W);
  follow_voxel3d(flow4, g, (int)(v0 + list[threadIdx.x]), niter, hist, pos);
}

// ------------------------------------------------------------------ seeds / expansion

// Seeds: h > 10 and h >= max over the 5x5x5 neighbourhood (zero outside).
__global__ __launch_bounds__(256) void seeds3d_kernel(const int* __restrict__ hist, int Zp, int Hp, int Wp,
                                                      long long* __restrict__ keys, int* __restrict__ nseeds, int cap) {
  const long long n = (long long)Zp * Hp * Wp;
  const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
  if (lin >= n) return;
  const int v = hist[lin];
  if (v <= 10) return;
  const int HWp = Hp * Wp;
  const int z = (int)(lin / HWp), r = (int)(lin - (long long)z * HWp);
  const int y = r / Wp, x = r % Wp;
  int m = 0;
  for (int dz = -2; dz <= 2; ++dz) {
    const int zz = z + dz;
    if (zz < 0 || zz >= Zp) continue;
    for (int dy = -2; dy <= 2; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= Hp) continue;
      const int* row = hist + ((size_t)zz * Hp + yy) * Wp;
      for (int dx = -2; dx <= 2; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= Wp) continue;
        m = max(m, row[xx]);
      }
    }
  }
  if (v < m) return;
  const int k = atomicAdd(nseeds, 1);
  if (k < cap) keys[k] = ((long long)v << 32) | lin;
}

// One wave per seed.  Window rows r = wz * 11 + wy (121 of them), bit wx of a row word = voxel
// (sz - 5 + wz, sy - 5 + wy, sx - 5 + wx); lane l owns rows l and l + 64.
__global__ __launch_bounds__(256) void expand3d_kernel(const int* __restrict__ hist, const long long* __restrict__ keys_sorted,
                                                       int nseeds, int Zp, int Hp, int Wp, int* __restrict__ M1) {
  __shared__ unsigned sup[4][128];
  __shared__ unsigned rows[4][2][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + wave;
  const bool active = k < nseeds;
  int sz = 0, sy = 0, sx = 0;
  if (active) {
    const int lin = (int)(keys_sorted[k] & 0xffffffffLL);
    const int HWp = Hp * Wp;
    sz = lin / HWp;
    const int r = lin - sz * HWp;
    sy = r / Wp;
    sx = r % Wp;
  }
  unsigned* s = sup[wave];
  unsigned* cur = rows[wave][0];
  unsigned* nxt = rows[wave][1];
  for (int c = lane; c < 128; c += 64) {
    s[c] = 0u;
    cur[c] = (c == 60) ? (1u << 5) : 0u;  // centre (5, 5, 5): row 5 * 11 + 5
    nxt[c] = 0u;
  }
  __syncthreads();
  if (active) {
    for (int i = lane; i < 1331; i += 64) {
      const int r = i / 11, wx = i - r * 11;
      const int zz = sz - 5 + r / 11, yy = sy - 5 + r % 11, xx = sx - 5 + wx;
      if ((unsigned)zz < (unsigned)Zp && (unsigned)yy < (unsigned)Hp && (unsigned)xx < (unsigned)Wp &&
          hist[((size_t)zz * Hp + yy) * Wp + xx] > 2)
        atomicOr(s + r, 1u << wx);
    }
  }
  __syncthreads();
  for (int it = 0; it < 5; ++it) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = lane + 64 * h;
      if (r < 121) {
        const int wz = r / 11, wy = r - wz * 11;
        unsigned any = 0u;
        for (int dz = -1; dz <= 1; ++dz) {
          const int zz = wz + dz;
          if (zz < 0 || zz > 10) continue;
          for (int dy = -1; dy <= 1; ++dy) {
            const int yy = wy + dy;
            if (yy < 0 || yy > 10) continue;
            any |= cur[zz * 11 + yy];
          }
        }
        nxt[r] = (any | (any << 1) | (any >> 1)) & s[r] & 0x7ffu;
      }
    }
    __syncthreads();
    unsigned* t = cur; cur = nxt; nxt = t;
  }
  if (active) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = lane + 64 * h;
      if (r < 121) {
        unsigned bits = cur[r];
        const int zz = sz - 5 + r / 11, yy = sy - 5 + r % 11;
        while (bits) {  // at most 11 set bits; every set bit is inside the volume (support is 0 outside)
          const int wx = __ffs(bits) - 1;
          bits &= bits - 1;
          atomicMax(M1 + ((size_t)zz * Hp + yy) * Wp + (sx - 5 + wx), k + 1);
        }
      }
    }
  }
}

bool sizes_ok(int Z, int H, int W) {
  if (Z < 0 || H < 0 || W < 0) return false;
  return (long long)(Z + 2 * RPAD) * (H + 2 * RPAD) * (W + 2 * RPAD) < (1ll << 31);
}

}  // namespace

extern "C" {

// One chunk of one view's network output y [n, 3, h, w] (planes p0 .. p0 + n - 1 of the view) into
// acc [4, Z, H, W].  view 0 = YX (h, w = H, W; writes), 1 = ZX (Z, W; adds), 2 = ZY (Z, H; adds).
int be_cp_accum_view3d(const float* y, int view, int p0, int n, int Z, int H, int W, float* acc, hipStream_t s) {
  if (!sizes_ok(Z, H, W) || view < 0 || view > 2 || p0 < 0 || n < 0) return (int)hipErrorInvalidValue;
  const int planes = view == 0 ? Z : view == 1 ? H : W;
  if (p0 + n > planes) return (int)hipErrorInvalidValue;
  if (n == 0 || (long long)Z * H * W == 0) return 0;
  if (view == 0) {
    const long long e = (long long)n * H * W;
    hipLaunchKernelGGL(accum_yx_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, y, p0, n, Z, H, W, acc);
  } else if (view == 1) {
    const long long e = (long long)n * Z * W;
    hipLaunchKernelGGL(accum_zx_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, y, p0, n, Z, H, W, acc);
  } else {
    if (Z > 65535 || (n + 31) / 32 > 65535) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(accum_zy_kernel, dim3((unsigned)((H + 31) / 32), (unsigned)((n + 31) / 32), (unsigned)Z), dim3(256), 0,
                       s, y, p0, n, Z, H, W, acc);
  }
  return BE_CHECK_LAUNCH();
}

int be_cp_prep_flow3d(const float* acc, int Z, int H, int W, float thr, void* flow4, void* fg, hipStream_t s) {
  if (!sizes_ok(Z, H, W)) return (int)hipErrorInvalidValue;
  const long long n = (long long)Z * H * W;
  if (n == 0) return 0;
  hipLaunchKernelGGL(prep_flow3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, acc, n, thr, (float4*)flow4,
                     (uint8_t*)fg);
  return BE_CHECK_LAUNCH();
}

// flow4 [Z, H, W] float4, fg [Z, H, W] uint8, hist [Z+2R, H+2R, W+2R] int32 (zeroed), pos [Z, H, W]
// int32 (-1 for background).  variant 0 = XCD-ordered compacted launch, 1 = plain; same results.
int be_cp_follow_flows3d(const void* flow4, const void* fg, int* hist, int* pos, int Z, int H, int W, int niter,
                         int variant, hipStream_t s) {
  if (!sizes_ok(Z, H, W) || niter < 0) return (int)hipErrorInvalidValue;
  const long long n = (long long)Z * H * W;
  if (n == 0) return 0;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (variant == 1)
    hipLaunchKernelGGL(follow_flows3d_plain_kernel, grid, dim3(256), 0, s, (const float4*)flow4, (const uint8_t*)fg, hist,
                       pos, Z, H, W, niter);
  else
    hipLaunchKernelGGL(follow_flows3d_xcd_kernel, grid, dim3(256), 0, s, (const float4*)flow4, (const uint8_t*)fg, hist, pos,
                       Z, H, W, niter);
  return BE_CHECK_LAUNCH();
}

// hist [Zp, Hp, Wp] -> keys[0 .. min(*nseeds, cap)) = count << 32 | raster index, *nseeds (zeroed by the caller).
int be_cp_seeds3d(const int* hist, int Zp, int Hp, int Wp, long long* keys, int* nseeds, int cap, hipStream_t s) {
  const long long n = (long long)Zp * Hp * Wp;
  if (Zp < 0 || Hp < 0 || Wp < 0 || n >= (1ll << 31)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(seeds3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hist, Zp, Hp, Wp, keys, nseeds, cap);
  return BE_CHECK_LAUNCH();
}

// keys_sorted[0 .. nseeds): ascending; M1 [Zp, Hp, Wp] int32 (zeroed) gets max(rank + 1) per voxel.
int be_cp_expand3d(const int* hist, const long long* keys_sorted, int nseeds, int Zp, int Hp, int Wp, int* M1,
                   hipStream_t s) {
  const long long n = (long long)Zp * Hp * Wp;
  if (Zp < 0 || Hp < 0 || Wp < 0 || n >= (1ll << 31) || nseeds < 0) return (int)hipErrorInvalidValue;
  if (nseeds == 0 || n == 0) return 0;
  hipLaunchKernelGGL(expand3d_kernel, dim3((unsigned)((nseeds + 3) / 4)), dim3(256), 0, s, hist, keys_sorted, nseeds, Zp, Hp,
                     Wp, M1);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
