// Tile gather / tapered blend for tiled 2D inference (Cellpose run_net tiling, BioImage.IO blocked
// prediction, fibsem 2D tiles).  SURVEY.md §2.5 K2, K7, K14.
//
// be_tiles_gather: normalised image [B, C, H, W] fp32 (or bf16 when src_bf16) -> NHWC bf16 tiles
//   [B*nty*ntx, by, bx, cpad].  The image is implicitly zero-padded by (pad_y, pad_x) on the
//   top/left (cellpose pad_image_ND), so padding, channel padding, layout change and bf16 cast all
//   happen in one pass; tiles never exist in fp32 NCHW.
// be_tiles_blend: tile outputs [B*nt, nout, by, bx] fp32 -> [B, nout, H, W] fp32 by the separable
//   taper mask wy[ty] * wx[tx] (cellpose _taper_mask), normalised by the summed weights.  Output-
//   centric gather (each output pixel walks only the tiles that cover it), so there are no atomics
//   and the result is bit-deterministic.
// be_tiles_gather_norm: the same gather straight from the RAW image (float32, uint16 or uint8) with
//   the percentile normalisation of percentile.hip applied in the load: the select passes run on the
//   raw pixels, then each pixel is read once, normalised with its row's constants and stored as
//   bf16 -- neither an fp32 copy of the input nor a normalised fp32 image ever exists.
// be_tiles_gather_aug / be_tiles_gather_norm_aug / be_tiles_blend_aug: the three calls under test-time
//   augmentation.  Tile (ti, tj) of the grid reaches the network with its rows reversed when tj is odd
//   and its columns reversed when ti is odd; the blend reads the tile output back at the reversed
//   offset and negates dY / dX of a reversed axis.  The mirroring is an index reversal in loads that
//   happen anyway: no mirrored copy of the tiles or of their outputs exists.
#include "percentile.h"

namespace {

#ifndef TILES_GATHER_ROWS
#define TILES_GATHER_ROWS 4
#endif
constexpr int kRows = TILES_GATHER_ROWS;  // tile rows per block: independent loads in flight per lane
constexpr int kMaxGridYZ = 65535;

// One kernel for both gathers.  Grid (x-blocks, row groups, tiles): the tile, its image b and its
// ys / xs entries are per block, so the only division left is the split of a lane's index into
// (pixel, 8-channel group), by a small 32-bit number.  A lane owns one pixel's 8-channel group
// (one 16-byte store) in kRows consecutive tile rows; consecutive lanes take consecutive groups of
// consecutive pixels, so the loads from an image row and the stores are contiguous.
// NORM: img holds raw pixels and row b * C_use + c of `state` that row's selected keys
// (percentile.h); channels >= C_use of a wider image (C_src) are ignored.
// AUG (test-time augmentation): the tile of grid row ti, grid column tj is stored with its rows
// reversed when tj is odd and its columns reversed when ti is odd, i.e. tile row ty holds image row
// ys[ti] + (by - 1 - ty).  Both flags are per block, the stores stay ascending; only the load index
// runs backwards.
// XM (the options of be_pct::NormExt, percentile.h): 1 = the global rules with fixed bounds and / or
// inversion, 2 = tile normalisation against the sampled maps; 0 compiles exactly the kernels above.
template <typename T, bool NORM, bool AUG = false, int XM = 0>
__global__ __launch_bounds__(256) void tiles_gather_kernel(const T* __restrict__ img, int tile0, int C_src, int C_use, int H,
                                                           int W, int pad_y, int pad_x, const int* __restrict__ ys,
                                                           const int* __restrict__ xs, int nty, int ntx, int by, int bx,
                                                           int cpad, const be_pct::Coef cf,
                                                           const uint32_t* __restrict__ state, bf16_t* __restrict__ out,
                                                           const be_pct::NormExt ext) {
  const int ngrp = cpad >> 3;
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int tx = ngrp == 1 ? q : q / ngrp;
  const int g = ngrp == 1 ? 0 : q - tx * ngrp;
  if (tx >= bx) return;
  const int tile = tile0 + blockIdx.z;
  const int nt = nty * ntx;
  const int b = tile / nt, t = tile - b * nt;
  const int ti = t / ntx;
  const int tj = t - ti * ntx;
  const int ty0 = blockIdx.y * kRows;
  const bool fy = AUG && (tj & 1), fx = AUG && (ti & 1);
  const int yy0 = ys[ti] + (fy ? by - 1 - ty0 : ty0) - pad_y;
  const int xx = xs[tj] + (fx ? bx - 1 - tx : tx) - pad_x;
  const bool inx = xx >= 0 && xx < W;
  float f[kRows][8];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) f[r][j] = 0.f;
  int mx0 = 0, mx1 = 0;
  float mwx = 0.f;
  if (XM == 2 && inx) be_pct::map_coord(xx, ext.sx, ext.nx, mx0, mx1, mwx);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * g + j;
    if (c < C_use) {
      float p1 = 0.f, scale = 1.f;
      bool cst = false;
      if (NORM && XM == 0) be_pct::row_consts<T>(state + ((size_t)b * C_use + c) * be_pct::kT * 2, cf, p1, scale, cst);
      if (XM == 1)
        be_pct::ext_consts<T>(ext, ext.lowhigh ? nullptr : state + ((size_t)b * C_use + c) * be_pct::kT * 2, cf, c, p1, scale, cst);
      const size_t mo = XM == 2 ? ((size_t)b * C_use + c) * ext.ny * ext.nx : 0;
      const T* plane = img + ((size_t)b * C_src + c) * H * W;
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int yy = fy ? yy0 - r : yy0 + r;
        if (inx && yy >= 0 && yy < H && ty0 + r < by) {
          const float v = (float)plane[(size_t)yy * W + xx];
          if (XM == 2) {
            int my0, my1;
            float mwy;
            be_pct::map_coord(yy, ext.sy, ext.ny, my0, my1, mwy);
            f[r][j] = be_pct::tile_norm(v, ext.lo_map + mo, ext.hi_map + mo, ext.nx, my0, my1, mwy, mx0, mx1, mwx, ext.invert != 0);
          } else if (XM == 1) {
            f[r][j] = be_pct::norm_div(v, p1, scale, cst, ext.invert != 0);  // scale holds the denominator here
          } else {
            f[r][j] = NORM ? (cst ? 0.f : (v - p1) * scale) : v;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    if (ty0 + r < by) {
      u32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = pack2bf(f[r][2 * j], f[r][2 * j + 1]);
      *reinterpret_cast<u32x4*>(out + (((size_t)tile * by + ty0 + r) * bx + tx) * cpad + 8 * g) = v;
    }
  }
}

template <typename T, bool NORM, bool AUG = false, int XM = 0>
int gather_launch(const void* img, int B, int C_src, int C_use, int H, int W, int pad_y, int pad_x, const int* ys,
                  const int* xs, int nty, int ntx, int by, int bx, int cpad, be_pct::Coef cf, const uint32_t* state,
                  void* out, hipStream_t s, const be_pct::NormExt ext = be_pct::NormExt{}) {
  const long long tiles = (long long)B * nty * ntx;
  const unsigned gx = (unsigned)(((long long)bx * (cpad >> 3) + 255) / 256), gy = (unsigned)((by + kRows - 1) / kRows);
  for (long long t0 = 0; t0 < tiles; t0 += kMaxGridYZ) {  // one launch unless a call has more tiles than grid.z holds
    const unsigned gz = (unsigned)(tiles - t0 < kMaxGridYZ ? tiles - t0 : kMaxGridYZ);
    hipLaunchKernelGGL((tiles_gather_kernel<T, NORM, AUG, XM>), dim3(gx, gy, gz), dim3(256), 0, s, static_cast<const T*>(img),
                       (int)t0, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, (bf16_t*)out, ext);
  }
  return BE_CHECK_LAUNCH();
}

bool gather_args_ok(int B, int C, int H, int W, int nty, int ntx, int by, int bx, int cpad) {
  return B > 0 && C > 0 && H > 0 && W > 0 && nty > 0 && ntx > 0 && by > 0 && bx > 0 && cpad > 0 && cpad % 8 == 0 &&
         (by + kRows - 1) / kRows <= kMaxGridYZ && (long long)B * nty * ntx <= 0x7fffffffLL &&
         (long long)bx * (cpad >> 3) <= 0x7fffffffLL - 256;
}

// AUG: the tile outputs are still mirrored as the gather stored them.  The taper weight is taken at
// the un-mirrored offset (ty, tx); the value is read at the mirrored one and the flow component along
// a mirrored axis (channel 0 = dY, channel 1 = dX) changes its sign.  Every (i, j) is one tile, so
// equal starts contribute once per tile.
template <bool AUG>
__global__ __launch_bounds__(256) void tiles_blend_kernel(const float* __restrict__ yt, int B, int nout, int H, int W,
                                                          int pad_y, int pad_x, const int* __restrict__ ys,
                                                          const int* __restrict__ xs, int nty, int ntx, int by, int bx,
                                                          const float* __restrict__ wy, const float* __restrict__ wx,
                                                          float* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)B * H * W;
  if (gid >= n) return;
  const int x = (int)(gid % W);
  const int y = (int)((gid / W) % H);
  const int b = (int)(gid / ((long long)H * W));
  const int yp = y + pad_y, xp = x + pad_x;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float wsum = 0.f;
  for (int i = 0; i < nty; ++i) {
    const int ty = yp - ys[i];
    if (ty < 0 || ty >= by) continue;
    for (int j = 0; j < ntx; ++j) {
      const int tx = xp - xs[j];
      if (tx < 0 || tx >= bx) continue;
      const float w = wy[ty] * wx[tx];
      wsum += w;
      const bool fy = AUG && (j & 1), fx = AUG && (i & 1);
      const int sy = fy ? by - 1 - ty : ty, sx = fx ? bx - 1 - tx : tx;
      const float* src = yt + (((size_t)b * nty * ntx + i * ntx + j) * nout) * by * bx + (size_t)sy * bx + sx;
      for (int c = 0; c < nout && c < 4; ++c) {
        const float v = src[(size_t)c * by * bx];
        acc[c] += w * (((c == 0 && fy) || (c == 1 && fx)) ? -v : v);
      }
    }
  }
  const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
  for (int c = 0; c < nout && c < 4; ++c) out[(((size_t)b * nout + c) * H + y) * W + x] = acc[c] * inv;
}

// the element type and the mirroring of one extended gather (XM = 1, 2) -> its instantiation
template <int XM>
int gather_ext(bool aug, const void* x, int dtype, int B, int C_src, int C_use, int H, int W, int pad_y, int pad_x,
               const int* ys, const int* xs, int nty, int ntx, int by, int bx, int cpad, be_pct::Coef cf, const uint32_t* state,
               void* out, hipStream_t s, const be_pct::NormExt& ext) {
#define BE_GATHER_EXT(T, A) \
  gather_launch<T, true, A, XM>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s, ext)
  if (dtype == be_pct::kF32) return aug ? BE_GATHER_EXT(float, true) : BE_GATHER_EXT(float, false);
  if (dtype == be_pct::kU16) return aug ? BE_GATHER_EXT(uint16_t, true) : BE_GATHER_EXT(uint16_t, false);
  if (dtype == be_pct::kU8) return aug ? BE_GATHER_EXT(uint8_t, true) : BE_GATHER_EXT(uint8_t, false);
#undef BE_GATHER_EXT
  return -3;
}

int gather_normx(bool aug, const void* x, int dtype, int B, int C_src, int C_use, int H, int W, float lower, float upper,
                 const float* lowhigh, int invert, int pad_y, int pad_x, const int* ys, const int* xs, int nty, int ntx, int by,
                 int bx, int cpad, void* out, void* ws, long long ws_bytes, hipStream_t s) {
  if (!gather_args_ok(B, C_src, H, W, nty, ntx, by, bx, cpad) || C_use <= 0 || C_use > C_src) return -1;
  if (dtype != be_pct::kF32 && dtype != be_pct::kU16 && dtype != be_pct::kU8) return -3;
  be_pct::NormExt ext;
  ext.lowhigh = lowhigh;
  ext.invert = invert;
  be_pct::Coef cf{};
  const uint32_t* state = nullptr;
  if (!lowhigh) {
    const int rc = be_pct::select_run(x, dtype, B, C_src, C_use, (long long)H * W, lower, upper, ws, ws_bytes, s, &cf, &state);
    if (rc) return rc;
  }
  return gather_ext<1>(aug, x, dtype, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s, ext);
}

int gather_tilenorm(bool aug, const void* x, int dtype, int B, int C_src, int C_use, int H, int W, const float* lo_map,
                    const float* hi_map, int ny, int nx, int invert, int pad_y, int pad_x, const int* ys, const int* xs, int nty,
                    int ntx, int by, int bx, int cpad, void* out, hipStream_t s) {
  if (!gather_args_ok(B, C_src, H, W, nty, ntx, by, bx, cpad) || C_use <= 0 || C_use > C_src || !lo_map || !hi_map || ny <= 0 ||
      nx <= 0 || (long long)ny * nx > be_pct::kMaxCells)
    return -1;
  be_pct::NormExt ext;
  ext.lo_map = lo_map;
  ext.hi_map = hi_map;
  ext.ny = ny;
  ext.nx = nx;
  ext.sy = (float)((double)ny / H);
  ext.sx = (float)((double)nx / W);
  ext.invert = invert;
  return gather_ext<2>(aug, x, dtype, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, be_pct::Coef{}, nullptr,
                       out, s, ext);
}

}  // namespace

extern "C" {

int be_tiles_gather(const float* img, int B, int C, int H, int W, int pad_y, int pad_x, const int* ys, const int* xs,
                    int nty, int ntx, int by, int bx, int cpad, void* out, hipStream_t s) {
  if (!gather_args_ok(B, C, H, W, nty, ntx, by, bx, cpad)) return -1;
  return gather_launch<float, false>(img, B, C, C, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, be_pct::Coef{},
                                     nullptr, out, s);
}

// x: raw image [B, C_src, H, W] of element type `dtype` (0 float32, 1 uint16, 2 uint8).  The first
// C_use channels are normalised per (image, channel) between the `lower` / `upper` percentiles
// (exactly be_pct_normalize on the pixels converted to fp32) and gathered like be_tiles_gather;
// channels >= C_use of `out` are zero.  ws: a be_pct_workspace_bytes(B * C_use) workspace, same
// rules as be_pct_normalize.  Non-zero return: nothing was launched.
int be_tiles_gather_norm(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, float lower, float upper,
                         int pad_y, int pad_x, const int* ys, const int* xs, int nty, int ntx, int by, int bx, int cpad,
                         void* out, void* ws, long long ws_bytes, hipStream_t s) {
  if (!gather_args_ok(B, C_src, H, W, nty, ntx, by, bx, cpad)) return -1;
  be_pct::Coef cf;
  const uint32_t* state;
  const int rc = be_pct::select_run(x, dtype, B, C_src, C_use, (long long)H * W, lower, upper, ws, ws_bytes, s, &cf, &state);
  if (rc) return rc;
  if (dtype == be_pct::kF32)
    return gather_launch<float, true>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s);
  if (dtype == be_pct::kU16)
    return gather_launch<uint16_t, true>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s);
  return gather_launch<uint8_t, true>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s);
}

int be_tiles_blend(const float* yt, int B, int nout, int H, int W, int pad_y, int pad_x, const int* ys, const int* xs, int nty,
                   int ntx, int by, int bx, const float* wy, const float* wx, float* out, hipStream_t s) {
  if (nout > 4) return -1;
  const long long n = (long long)B * H * W;
  hipLaunchKernelGGL(tiles_blend_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, yt, B, nout, H, W, pad_y, pad_x,
                     ys, xs, nty, ntx, by, bx, wy, wx, out);
  return BE_CHECK_LAUNCH();
}

// ---- test-time augmentation (cellpose augment=True): the same three calls on half-overlapping
// by x bx tiles, every tile mirrored by its grid position (see tiles_gather_kernel / tiles_blend_kernel).
// Their own instantiations: the entry points above compile exactly as without them.

int be_tiles_gather_aug(const float* img, int B, int C, int H, int W, int pad_y, int pad_x, const int* ys, const int* xs,
                        int nty, int ntx, int by, int bx, int cpad, void* out, hipStream_t s) {
  if (!gather_args_ok(B, C, H, W, nty, ntx, by, bx, cpad)) return -1;
  return gather_launch<float, false, true>(img, B, C, C, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, be_pct::Coef{},
                                           nullptr, out, s);
}

int be_tiles_gather_norm_aug(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, float lower, float upper,
                             int pad_y, int pad_x, const int* ys, const int* xs, int nty, int ntx, int by, int bx,
                             int cpad, void* out, void* ws, long long ws_bytes, hipStream_t s) {
  if (!gather_args_ok(B, C_src, H, W, nty, ntx, by, bx, cpad)) return -1;
  be_pct::Coef cf;
  const uint32_t* state;
  const int rc = be_pct::select_run(x, dtype, B, C_src, C_use, (long long)H * W, lower, upper, ws, ws_bytes, s, &cf, &state);
  if (rc) return rc;
  if (dtype == be_pct::kF32)
    return gather_launch<float, true, true>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s);
  if (dtype == be_pct::kU16)
    return gather_launch<uint16_t, true, true>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s);
  return gather_launch<uint8_t, true, true>(x, B, C_src, C_use, H, W, pad_y, pad_x, ys, xs, nty, ntx, by, bx, cpad, cf, state, out, s);
}

int be_tiles_blend_aug(const float* yt, int B, int nout, int H, int W, int pad_y, int pad_x, const int* ys, const int* xs,
                       int nty, int ntx, int by, int bx, const float* wy, const float* wx, float* out, hipStream_t s) {
  if (nout > 4) return -1;
  const long long n = (long long)B * H * W;
  hipLaunchKernelGGL(tiles_blend_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, yt, B, nout, H, W, pad_y,
                     pad_x, ys, xs, nty, ntx, by, bx, wy, wx, out);
  return BE_CHECK_LAUNCH();
}

// ---- the options of the cellpose `normalize` dict in the gather (be_pct::NormExt): the global rules
// with fixed bounds `lowhigh` ([C_use][2] on the device, no select runs; null: the percentiles) and /
// or inversion, and tile normalisation against the maps of be_pct_tile_maps.  Each pixel is what
// be_pct_normalize_ext / be_pct_normalize_tile give, rounded to bf16.

int be_tiles_gather_normx(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, float lower, float upper,
                          const float* lowhigh, int invert, int pad_y, int pad_x, const int* ys, const int* xs, int nty, int ntx,
                          int by, int bx, int cpad, void* out, void* ws, long long ws_bytes, hipStream_t s) {
  return gather_normx(false, x, dtype, B, C_src, C_use, H, W, lower, upper, lowhigh, invert, pad_y, pad_x, ys, xs, nty, ntx, by, bx,
                      cpad, out, ws, ws_bytes, s);
}

int be_tiles_gather_normx_aug(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, float lower, float upper,
                              const float* lowhigh, int invert, int pad_y, int pad_x, const int* ys, const int* xs, int nty,
                              int ntx, int by, int bx, int cpad, void* out, void* ws, long long ws_bytes, hipStream_t s) {
  return gather_normx(true, x, dtype, B, C_src, C_use, H, W, lower, upper, lowhigh, invert, pad_y, pad_x, ys, xs, nty, ntx, by, bx,
                      cpad, out, ws, ws_bytes, s);
}

int be_tiles_gather_tilenorm(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, const float* lo_map,
                             const float* hi_map, int ny, int nx, int invert, int pad_y, int pad_x, const int* ys, const int* xs,
                             int nty, int ntx, int by, int bx, int cpad, void* out, hipStream_t s) {
  return gather_tilenorm(false, x, dtype, B, C_src, C_use, H, W, lo_map, hi_map, ny, nx, invert, pad_y, pad_x, ys, xs, nty, ntx, by,
                         bx, cpad, out, s);
}

int be_tiles_gather_tilenorm_aug(const void* x, int dtype, int B, int C_src, int C_use, int H, int W, const float* lo_map,
                                 const float* hi_map, int ny, int nx, int invert, int pad_y, int pad_x, const int* ys,
                                 const int* xs, int nty, int ntx, int by, int bx, int cpad, void* out, hipStream_t s) {
  return gather_tilenorm(true, x, dtype, B, C_src, C_use, H, W, lo_map, hi_map, ny, nx, invert, pad_y, pad_x, ys, xs, nty, ntx, by,
                         bx, cpad, out, s);
}

}  // extern "C"
