// Tile gather / blend for a batch whose images each have their own scale (Cellpose per-image
// `diameter`): the ragged counterpart of tiles.hip.  Image b of [B, C, H, W] is resampled to
// (Hs_b, Ws_b), zero-padded, tiled, and its blended flows are resampled back to (H, W); neither the
// resized image nor (with the raw source forms) a normalised or fp32 copy of the input ever exists.
//
// Two tables, uploaded once per plan (cellpose/gpu.py ScaledTilePlan):
//   tile table  int32 [T][4]:  image index, y0, x0 (tile start on the padded scaled canvas), mirror
//                              flags (bit 0: rows reversed, bit 1: columns reversed)
//   image table int64 [B][kI]: Hs, Ws, pad_y, pad_x, nty, ntx, first tile, offset into the flat ys
//                              and xs arrays, pixel offset of the image in the flat scaled-flow buffer,
//                              by, bx, offset of its taper factors (wy[by] then wx[bx]), pixel offset
//                              of its first tile in the flat tile-output buffer
// Tiles of one shape (by, bx) are contiguous in the tile table; the gather runs once per shape.
//
// The bilinear rule is that of resize_bilinear_f32 (imageproc.hip): half-pixel centres, source
// coordinate clamped at 0, upper neighbour clamped at the edge, no antialiasing.  Every multiply
// that feeds an add is an explicit fmaf, so all instantiations (and the fp32 and raw source forms)
// round alike whatever the compiler would contract.
#include "percentile.h"

namespace {

constexpr int kRows = 4;  // tile rows per block, as tiles_gather_kernel
constexpr int kMaxGridYZ = 65535;
constexpr int kI = 16;  // int64 fields per image-table row
enum { iHs = 0, iWs, iPadY, iPadX, iNty, iNtx, iTile0, iYsOff, iXsOff, iFlowPix, iBy, iBx, iTaper, iYtPix };

// source coordinate of index i of an axis resampled from n_in to n_out: taps i0, i0 + step, weight of the upper
__device__ __forceinline__ void src_coord(int i, float ratio, int n_in, int& i0, int& step, float& w1) {
  float s = fmaf(ratio, (float)i + 0.5f, -0.5f);
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 < n_in - 1 ? i0 : n_in - 1;
  step = i0 < n_in - 1 ? 1 : 0;
  w1 = s - (float)i0;
}

__device__ __forceinline__ float lerp4(float a, float b, float c, float d, float lx1, float ly1) {
  const float lx0 = 1.f - lx1, ly0 = 1.f - ly1;
  const float top = fmaf(lx0, a, lx1 * b), bot = fmaf(lx0, c, lx1 * d);
  return fmaf(ly0, top, ly1 * bot);
}

// MODE 0: img is fp32 and taken as it is.  1: raw pixels, the percentile rule of row_consts (what
// be_tiles_gather_norm applies).  2: raw pixels, fixed bounds and / or inversion (ext_consts /
// norm_div, what be_tiles_gather_normx applies).  Each of the four taps is normalised, then lerped.
// Grid (x-blocks, row groups, tiles of this launch); a lane owns one pixel's 8-channel group in
// kRows consecutive tile rows: one 16-byte store per row.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void gather_scaled_kernel(const T* __restrict__ img, const int* __restrict__ tiles,
                                                            const long long* __restrict__ itab, int tile0, int group0,
                                                            int C_src, int C_use, int H, int W, int by, int bx, int cpad,
                                                            const be_pct::Coef cf, const uint32_t* __restrict__ state,
                                                            bf16_t* __restrict__ out, const be_pct::NormExt ext) {
  const int ngrp = cpad >> 3;
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int tx = ngrp == 1 ? q : q / ngrp;
  const int g = ngrp == 1 ? 0 : q - tx * ngrp;
  if (tx >= bx) return;
  const int tile = tile0 + blockIdx.z;
  const int* trow = tiles + (size_t)tile * 4;
  const int b = trow[0];
  const bool fy = trow[3] & 1, fx = trow[3] & 2;
  const long long* im = itab + (size_t)b * kI;
  const int Hs = (int)im[iHs], Ws = (int)im[iWs];
  const int ty0 = blockIdx.y * kRows;
  const int yy0 = trow[1] + (fy ? by - 1 - ty0 : ty0) - (int)im[iPadY];
  const int xx = trow[2] + (fx ? bx - 1 - tx : tx) - (int)im[iPadX];
  const bool inx = xx >= 0 && xx < Ws;
  const float ry = (float)H / (float)Hs, rx = (float)W / (float)Ws;
  int x0 = 0, xp = 0;
  float lx1 = 0.f;
  if (inx) src_coord(xx, rx, W, x0, xp, lx1);
  int y0[kRows], yp[kRows];
  float ly1[kRows];
  bool ok[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int yy = fy ? yy0 - r : yy0 + r;
    ok[r] = inx && yy >= 0 && yy < Hs && ty0 + r < by;
    y0[r] = yp[r] = 0;
    ly1[r] = 0.f;
    if (ok[r]) src_coord(yy, ry, H, y0[r], yp[r], ly1[r]);
  }
  float f[kRows][8];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) f[r][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * g + j;
    if (c < C_use) {
      float p1 = 0.f, scale = 1.f;
      bool cst = false;
      if (MODE == 1) be_pct::row_consts<T>(state + ((size_t)b * C_use + c) * be_pct::kT * 2, cf, p1, scale, cst);
      if (MODE == 2)
        be_pct::ext_consts<T>(ext, ext.lowhigh ? nullptr : state + ((size_t)b * C_use + c) * be_pct::kT * 2, cf, c, p1, scale, cst);
      const T* plane = img + ((size_t)b * C_src + c) * H * W;
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (ok[r]) {
          const T* r0 = plane + (size_t)y0[r] * W + x0;
          const T* r1 = r0 + (size_t)yp[r] * W;
          float v[4] = {(float)r0[0], (float)r0[xp], (float)r1[0], (float)r1[xp]};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (MODE == 1) v[k] = cst ? 0.f : (v[k] - p1) * scale;
            if (MODE == 2) v[k] = be_pct::norm_div(v[k], p1, scale, cst, ext.invert != 0);  // scale holds the denominator here
          }
          f[r][j] = lerp4(v[0], v[1], v[2], v[3], lx1, ly1[r]);
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
      *reinterpret_cast<u32x4*>(out + (((size_t)(tile - group0) * by + ty0 + r) * bx + tx) * cpad + 8 * g) = v;
    }
  }
}

template <typename T, int MODE>
int gather_scaled_launch(const void* img, const int* tiles, const long long* itab, int group0, int ntiles, int C_src, int C_use,
                         int H, int W, int by, int bx, int cpad, be_pct::Coef cf, const uint32_t* state, void* out,
                         hipStream_t s, const be_pct::NormExt ext) {
  const unsigned gx = (unsigned)(((long long)bx * (cpad >> 3) + 255) / 256), gy = (unsigned)((by + kRows - 1) / kRows);
  for (int t0 = 0; t0 < ntiles; t0 += kMaxGridYZ) {  // one launch unless the group has more tiles than grid.z holds
    const unsigned gz = (unsigned)(ntiles - t0 < kMaxGridYZ ? ntiles - t0 : kMaxGridYZ);
    hipLaunchKernelGGL((gather_scaled_kernel<T, MODE>), dim3(gx, gy, gz), dim3(256), 0, s, static_cast<const T*>(img), tiles, itab,
                       group0 + t0, group0, C_src, C_use, H, W, by, bx, cpad, cf, state, (bf16_t*)out, ext);
  }
  return BE_CHECK_LAUNCH();
}

bool scaled_args_ok(const void* tiles, const void* itab, int B, int C_src, int C_use, int H, int W, int group0, int ntiles, int by,
                    int bx, int cpad) {
  return tiles && itab && B > 0 && C_src > 0 && C_use > 0 && C_use <= C_src && H > 0 && W > 0 && group0 >= 0 && ntiles > 0 &&
         (long long)group0 + ntiles <= 0x7fffffffLL && by > 0 && bx > 0 && cpad > 0 && cpad % 8 == 0 &&
         (by + kRows - 1) / kRows <= kMaxGridYZ && (long long)bx * (cpad >> 3) <= 0x7fffffffLL - 256;
}

// Output-centric, atomic-free blend of image blockIdx.y: every pixel of its scaled image walks the
// tiles that cover it (tiles_blend_kernel), reads the tile output at the offset the tile's mirror
// flags give and negates dY / dX of a reversed axis.
__global__ __launch_bounds__(256) void blend_scaled_kernel(const float* __restrict__ yt, const int* __restrict__ tiles,
                                                           const long long* __restrict__ itab, const int* __restrict__ ys,
                                                           const int* __restrict__ xs, const float* __restrict__ taper, int nout,
                                                           int unmirror, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long* im = itab + (size_t)b * kI;
  const int Hs = (int)im[iHs], Ws = (int)im[iWs];
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (long long)Hs * Ws) return;
  const int y = (int)(pix / Ws), x = (int)(pix - (long long)y * Ws);
  const int yp = y + (int)im[iPadY], xp = x + (int)im[iPadX];
  const int nty = (int)im[iNty], ntx = (int)im[iNtx], by = (int)im[iBy], bx = (int)im[iBx];
  const int* iys = ys + im[iYsOff];
  const int* ixs = xs + im[iXsOff];
  const float* wy = taper + im[iTaper];
  const float* wx = wy + by;
  const int* trow = tiles + (size_t)im[iTile0] * 4;
  const float* ytb = yt + (size_t)im[iYtPix] * nout;
  const size_t tpix = (size_t)by * bx;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float wsum = 0.f;
  for (int i = 0; i < nty; ++i) {
    const int ty = yp - iys[i];
    if (ty < 0 || ty >= by) continue;
    for (int j = 0; j < ntx; ++j) {
      const int tx = xp - ixs[j];
      if (tx < 0 || tx >= bx) continue;
      const float w = wy[ty] * wx[tx];
      wsum += w;
      const int t = i * ntx + j;
      const int fl = unmirror ? trow[(size_t)t * 4 + 3] : 0;
      const bool fy = fl & 1, fx = fl & 2;
      const int sy = fy ? by - 1 - ty : ty, sx = fx ? bx - 1 - tx : tx;
      const float* src = ytb + (size_t)t * nout * tpix + (size_t)sy * bx + sx;
      for (int c = 0; c < nout && c < 4; ++c) {
        const float v = src[(size_t)c * tpix];
        acc[c] += w * (((c == 0 && fy) || (c == 1 && fx)) ? -v : v);
      }
    }
  }
  const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
  float* o = out + (size_t)im[iFlowPix] * nout + (size_t)y * Ws + x;
  for (int c = 0; c < nout && c < 4; ++c) o[(size_t)c * Hs * Ws] = acc[c] * inv;
}

// One lane per output pixel of [B, nout, H, W]: the bilinear sample of image b's [nout, Hs_b, Ws_b] blend.
__global__ __launch_bounds__(256) void resize_ragged_kernel(const float* __restrict__ in, const long long* __restrict__ itab, int B,
                                                            int nout, int H, int W, float* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)B * nout * H * W) return;
  const int ox = (int)(gid % W);
  const int oy = (int)((gid / W) % H);
  const long long pl = gid / ((long long)H * W);
  const int b = (int)(pl / nout), c = (int)(pl - (long long)b * nout);
  const long long* im = itab + (size_t)b * kI;
  const int Hs = (int)im[iHs], Ws = (int)im[iWs];
  int y0, yp, x0, xp;
  float ly1, lx1;
  src_coord(oy, (float)Hs / (float)H, Hs, y0, yp, ly1);
  src_coord(ox, (float)Ws / (float)W, Ws, x0, xp, lx1);
  const float* r0 = in + ((size_t)im[iFlowPix] * nout + (size_t)c * Hs * Ws) + (size_t)y0 * Ws + x0;
  const float* r1 = r0 + (size_t)yp * Ws;
  out[gid] = lerp4(r0[0], r0[xp], r1[0], r1[xp], lx1, ly1);
}

}  // namespace

extern "C" {

// One tile-shape group of a ragged plan: rows [group0, group0 + ntiles) of the tile table ->
// out [ntiles, by, bx, cpad] bf16.  img: [B, C_src, H, W]; dtype 0 float32, 1 uint16, 2 uint8
// (percentile.h).  mode 0: float32 pixels as they are (already normalised, or normalisation off).
// mode 1: normalise between the `lower` / `upper` percentiles of the raw pixels; mode 2: the global
// rules with fixed bounds `lowhigh` ([C_use][2] on the device, or null for the percentiles) and / or
// inversion.  The percentile select of modes 1 and 2 runs in every call (ws: a
// be_pct_workspace_bytes(B * C_use) workspace, the rules of be_pct_normalize): one group is the normal
// case, and a further group exists only for images smaller than a tile.  Non-zero return: nothing
// was launched.
int be_tiles_gather_scaled(const void* img, int dtype, int mode, int B, int C_src, int C_use, int H, int W, float lower,
                           float upper, const float* lowhigh, int invert, const int* tiles, const long long* itab, int group0,
                           int ntiles, int by, int bx, int cpad, void* out, void* ws, long long ws_bytes, hipStream_t s) {
  if (!img || !out || !scaled_args_ok(tiles, itab, B, C_src, C_use, H, W, group0, ntiles, by, bx, cpad)) return -1;
  if (mode < 0 || mode > 2 || (mode == 0 && dtype != be_pct::kF32)) return -1;
  if (dtype != be_pct::kF32 && dtype != be_pct::kU16 && dtype != be_pct::kU8) return -3;
  be_pct::NormExt ext;
  ext.lowhigh = mode == 2 ? lowhigh : nullptr;
  ext.invert = mode == 2 ? invert : 0;
  be_pct::Coef cf{};
  const uint32_t* state = nullptr;
  if (mode != 0 && !ext.lowhigh) {
    const int rc = be_pct::select_run(img, dtype, B, C_src, C_use, (long long)H * W, lower, upper, ws, ws_bytes, s, &cf, &state);
    if (rc) return rc;
  }
#define BE_GS(T, M) \
  gather_scaled_launch<T, M>(img, tiles, itab, group0, ntiles, C_src, C_use, H, W, by, bx, cpad, cf, state, out, s, ext)
  if (mode == 0) return BE_GS(float, 0);
  if (dtype == be_pct::kF32) return mode == 1 ? BE_GS(float, 1) : BE_GS(float, 2);
  if (dtype == be_pct::kU16) return mode == 1 ? BE_GS(uint16_t, 1) : BE_GS(uint16_t, 2);
  return mode == 1 ? BE_GS(uint8_t, 1) : BE_GS(uint8_t, 2);
#undef BE_GS
}

// yt: the tile outputs of all groups, flat ([ntiles, nout, by, bx] fp32 per group, in table order)
// -> out: flat fp32, image b's [nout, Hs_b, Ws_b] blend at its table offset.  max_pix: the largest
// Hs_b * Ws_b.  unmirror 0 blends the tiles as they lie (for tests of the flags).
int be_tiles_blend_scaled(const float* yt, const int* tiles, const long long* itab, const int* ys, const int* xs,
                          const float* taper, int B, int nout, long long max_pix, int unmirror, float* out, hipStream_t s) {
  if (!yt || !tiles || !itab || !ys || !xs || !taper || !out || B <= 0 || B > kMaxGridYZ || nout <= 0 || nout > 4 || max_pix <= 0 ||
      (max_pix + 255) / 256 > 0x7fffffffLL)
    return -1;
  hipLaunchKernelGGL(blend_scaled_kernel, dim3((unsigned)((max_pix + 255) / 256), (unsigned)B), dim3(256), 0, s, yt, tiles, itab, ys,
                     xs, taper, nout, unmirror, out);
  return BE_CHECK_LAUNCH();
}

// in: the flat buffer be_tiles_blend_scaled wrote -> out [B, nout, H, W] fp32, each image
// resampled from its own (Hs_b, Ws_b) by the rule of be_resize_bilinear.
int be_resize_bilinear_ragged(const float* in, const long long* itab, int B, int nout, int H, int W, float* out, hipStream_t s) {
  if (!in || !itab || !out || B <= 0 || nout <= 0 || H <= 0 || W <= 0) return -1;
  const long long n = (long long)B * nout * H * W;
  if ((n + 255) / 256 > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(resize_ragged_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, itab, B, nout, H, W, out);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
