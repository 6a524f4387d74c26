// Two-group ping-pong 3x3 conv with fused pre-activation for Cin = Cout = 128 (the plain level-2
// convs of CPnet at 56^2): be_conv2d_nhwc's INMODE 0 / no-x2 / bf16-NHWC semantics,
//
//   out = conv3x3( relu?( x * scale[c] + shift[n, c] ) ) + bias [+ residual]
//
// in the scheme of conv_pair_pp64.inc.  One workgroup computes ALL 128 output channels of its pixel
// tile, so the input is loaded, activated and written to LDS once (the per-layer kernel does it once
// per 64-channel block).  The 8 waves are two groups of 4 that own alternate tiles of the
// workgroup's range and run ONE PHASE APART on the same workgroup barriers, so one group's VALU /
// LDS-store phase runs beside the other group's MFMA phase on every SIMD:
//     per 32-channel input chunk c = 0..3:   P1 commit(c)   P2 MFMA(c), s_setprio 1
//     then                                   P3 residual + bias + stores
// Nine phases per tile: every MFMA phase of one group meets a VALU phase of the other; the one
// VALU / VALU slot per tile is a group's epilogue beside the other's first commit.
//
// Geometry: an 8 x 28 pixel tile per group (7 x 2 tiles cover 56^2 exactly; 16-wide row fragments
// would compute 64 columns per 56).  The MFMA's 16 pixels are a 4 x 4 patch: lane lrow is pixel
// (lrow >> 2, lrow & 3) of its fragment, a wave owns 2 channel tiles (ct = 2 cp, 2 cp + 1; cp = wave
// of the group) x all 14 fragments (2 rows x 7 columns of patches) = 112 accumulator VGPRs, so each
// pixel-fragment read feeds 2 MFMAs and each weight fragment 14.
//
// LDS: per group ONE 10 x 30 image of the current chunk, 64-byte pixels (19,200 B; 38,400 B per
// workgroup).  A group's commit of chunk c + 1 can only start once its own MFMA phase of chunk c is
// over (the phases of a group are sequential), so a second image per group would never be written
// while the first is read.  Pixels are unpadded.  Swizzle: the 16-byte unit c of pixel (y, x) lives
// at unit c ^ 2 ((x >> 1) & 1).  Derivation: a ds_read_b128 is served in lane groups of 16 =
// {kq, lrow 0-3, 12-15} + {kq + 1, lrow 4-11} (and the converse), i.e. patch rows 0 and 3 at unit k
// and patch rows 1 and 2 at unit k ^ 1.  The 16-byte bank slot of unit c of pixel (y, x) is
// 4 ((30 y + x) mod 4) + c = 4 ((2 y + x) mod 4) + c.  The 4 pixels of a patch row hit the 4
// residues once each; the pixel of the same residue in patch row r + 1 or r + 3 sits 2 columns to
// the left or right (2 (y + 1) + x +- 2 = 2 y + x mod 4).  Rows {0, 3} and {1, 2} already differ in
// bit 0 of the unit; within each pair, flipping bit 1 by (x >> 1) & 1 separates the two pixels of a
// residue, for any patch origin -- so all nine tap offsets are conflict-free.  Patch columns are 4
// apart and rows do not enter, so a fragment address is a per-lane base (one per dx) + a
// compile-time offset.
//
// Weights never pass through LDS: the host packs the conv once in MFMA-A-fragment order
// [chunk][tap][ct 0..7][lane][8 bf16] (ops/conv.py, pack_frag) and a wave fetches a fragment with
// one 16-byte-per-lane global load, WD K-steps ahead of its use (288 KB per conv, L2-resident).  The
// first WD steps of an MFMA phase are issued at the end of the commit before it, behind the next
// chunk's halo and affine, which are in flight across the barrier wait and the MFMA phase.
//
// Rounding points and the per-output accumulation order are conv2d_nhwc_kernel's (activation
// rounded to bf16 before LDS, zero padding after the activation, chunks in order, taps 0..8 within
// a chunk, 32-deep K-steps with lane group kq holding channels 8 kq..8 kq + 7, (acc + bias) +
// residual, one rounding), so the output is bit-identical to it.
//
// A second build (POOL) is the level-2 entry conv, 64 -> 128 channels from a 2 x 2 max-pooled source
// (conv2d_nhwc_kernel<3, 32, 64, 2, ...> bit for bit): two chunks per tile, and the four raw values
// of a halo unit fetched in two halves so that no more than 40 VGPRs of halo cross an MFMA phase
// (Halo<true>).  Five phases per tile: commit(0), MFMA(0), commit(1), MFMA(1), epilogue.  Its PROJ build
// also computes the level's residual projection (1x1, 64 -> 128, its own affine, no ReLU;
// conv2d_nhwc_kernel<1, 64, 64, 2, ...> bit for bit) of the same pooled pixels as a second output: the
// commits write the projection's input of the tile's centre pixels to a second LDS image per group, and
// after the epilogue the freed accumulators take two 32-deep K-steps per fragment from zero.
#include "common.h"

namespace {
namespace pp128 {
constexpr int TH = 8, TW = 28;              // output tile
constexpr int GW = 4, GT = GW * 64, NTP = 2 * GT;
constexpr int IH = TH + 2, IW = TW + 2, IPIX = IH * IW;  // input image 10 x 30
constexpr int IN_B = IPIX * 64;             // 19200
constexpr int LDS = 2 * IN_B;
constexpr int NF = 14, FC = 7;              // 4 x 4 pixel patches: 2 rows x 7 columns
constexpr int NCH = 4;                      // 32-channel input chunks
constexpr int C = 128;
constexpr int HU = IPIX * 4, HUPT = (HU + GT - 1) / GT;  // 16-byte halo units per chunk, per thread
constexpr int WD = 3;                       // weight fragments are fetched WD K-steps ahead
constexpr int WSTEP = 8 * 64 * 8;           // elements per K-step of the fragment layout (8 ct)
constexpr int BD = 6, BR = 7;               // pixel fragments are read BD MFMA pairs ahead, ring of BR
static_assert(IW % 4 == 2, "the swizzle derivation needs 30 y = 2 y (mod 4)");
// PROJ: a second image per group, the 1x1 projection's input of the tile's 8 x 28 centre pixels, all 64
// channels (128-byte pixels).  Swizzle: unit u of pixel (y, x) lives at unit u ^ 2 ((x >> 1) & 1) ^
// 4 (y & 1).  Derivation: the 16-byte bank slot of a unit is 8 (x mod 2) + u (28 y is even); a
// ds_read_b128 lane group holds patch rows 0 and 3 at unit k and rows 1 and 2 at unit k ^ 1, four pixels
// per row parity of x: bit 0 separates {0, 3} from {1, 2}, (x >> 1) & 1 in bit 1 the two pixels of one
// row, y & 1 in bit 2 row 0 from 3 and row 1 from 2 (patch origins are multiples of 4).
constexpr int PJ_B = TH * TW * 128;         // 28672
constexpr int LDS_PROJ = LDS + 2 * PJ_B;    // 95744
static_assert(LDS_PROJ <= 128 * 1024, "LDS budget of the ping-pong kernels");
static_assert(BD < BR, "ring");

struct Args {
  const bf16_t* x = nullptr;     // [N, H, W, 128]; POOL: [N, 2 H, 2 W, 64]
  const float* sa = nullptr;     // scale [128] (sa_ns 0) or [N, sa_ns], or null (1)
  const float* ta = nullptr;     // shift likewise, or null (0)
  const bf16_t* wf = nullptr;    // fragment-order weights
  const float* bias = nullptr;   // [128] or null
  const bf16_t* res = nullptr;   // [N, H, W, 128] (may be `out`), [N, H/2, W/2, 128] (res_up2), or null
  bf16_t* out = nullptr;         // [N, H, W, 128]
  int N = 0, H = 0, W = 0;
  int sa_ns = 0, ta_ns = 0;
  int relu = 0;
  int res_up2 = 0;     // the residual is at half resolution, read through nearest 2x up-sampling (even H, W)
  int tiles_x = 0, tiles_y = 0;
  // PROJ build: out2 = conv1x1( pool(x) * sp + tp ) + bias_p, [N, H, W, 128]
  const float* sp = nullptr;     // scale [64]
  const float* tp = nullptr;     // shift [64]
  const bf16_t* wpf = nullptr;   // fragment-order projection weights [2 K-steps][8 ct][64 lanes][8]
  const float* bias_p = nullptr; // [128] or null
  bf16_t* out2 = nullptr;
  // diagnostics (STAMP instantiation only, tools/pp128_phase_profile.py): [grid][2 groups][16] cycle
  // counts of wave 0 of each group
  unsigned long long* stamps = nullptr;
  // C256 build: `out` is [N, H, W, 256]; wf, bias and the post-activation vectors hold both halves
  const float* qs = nullptr;  // post-activation scale [256]
  const float* qt = nullptr;  // post-activation shift [256]
  int qrelu = 0;              // ReLU after the post-activation
};

struct TileXY {
  int n, ty0, tx0;
};

__device__ __forceinline__ TileXY tile_of(const Args& a, int t) {
  const int tpi = a.tiles_x * a.tiles_y;
  TileXY r;
  r.n = t / tpi;
  const int q = t - r.n * tpi;
  r.ty0 = (q / a.tiles_x) * TH;
  r.tx0 = (q % a.tiles_x) * TW;
  return r;
}

template <bool POOL>
struct Halo {
  u32x4 h[HUPT];
  float4 aff[4];  // scale / shift of this thread's 8 channels ride along with the halo
};

// POOL: the four raw values of a unit arrive in two halves.  Source row 2 y (h, hb: columns 2 x and
// 2 x + 1) is issued where the plain build issues its halo and is in flight across the MFMA phase, 40
// VGPRs in place of 20 + the 16 of the affine; source row 2 y + 1 (q, qb) and the affine follow in a
// VALU phase, where the weight and pixel-fragment rings of the MFMA phase (60 VGPRs) are dead: before
// the epilogue for the next tile's chunk 0 (PROJ: behind the projection, which needs the accumulators'
// registers once more), at the top of the commit for chunk 1, whose 64-byte halves of the 128-byte
// source pixels chunk 0 has already brought into the cache.
template <>
struct Halo<true> {
  u32x4 h[HUPT], hb[HUPT];
  u32x4 q[HUPT], qb[HUPT];
  float4 aff[4];
  float4 affp[4];  // PROJ: the projection's scale / shift of the same 8 channels
};

// chunk ch of the tile's 10 x 30 input halo -> registers; clamped, unconditional loads (commit
// zeroes what lies outside the image and skips units past HU)
template <bool POOL>
__device__ __forceinline__ void issue_aff(const Args& a, TileXY t, int c, Halo<POOL>& hr) {
  hr.aff[0] = hr.aff[1] = make_float4(1.f, 1.f, 1.f, 1.f);
  hr.aff[2] = hr.aff[3] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.sa) {
    const float* sr = a.sa + (size_t)t.n * a.sa_ns + c;
    hr.aff[0] = *reinterpret_cast<const float4*>(sr);
    hr.aff[1] = *reinterpret_cast<const float4*>(sr + 4);
  }
  if (a.ta) {
    const float* tr = a.ta + (size_t)t.n * a.ta_ns + c;
    hr.aff[2] = *reinterpret_cast<const float4*>(tr);
    hr.aff[3] = *reinterpret_cast<const float4*>(tr + 4);
  }
}

// POOL: x is [N, 2 H, 2 W, 64]; element offset of channel c of source pixel (2 gy + row, 2 gx)
__device__ __forceinline__ size_t pool_src(const Args& a, int n, int gy, int gx, int row, int c) {
  return (((size_t)n * 2 * a.H + 2 * gy + row) * 2 * a.W + 2 * gx) * 64 + c;
}

template <bool POOL>
__device__ __forceinline__ void issue_halo(const Args& a, TileXY t, int ch, int gt, Halo<POOL>& hr) {
  const int c = ch * 32 + (gt & 3) * 8;  // a thread's channel group is the same for every unit (GT % 4 == 0)
  if constexpr (!POOL) issue_aff(a, t, c, hr);
#pragma unroll
  for (int i = 0; i < HUPT; ++i) {
    const int pi = min(gt + i * GT, HU - 1) >> 2;
    const int y = pi / IW, x = pi - y * IW;
    const int gy = min(max(t.ty0 - 1 + y, 0), a.H - 1);
    const int gx = min(max(t.tx0 - 1 + x, 0), a.W - 1);
    if constexpr (POOL) {
      const bf16_t* p = a.x + pool_src(a, t.n, gy, gx, 0, c);
      hr.h[i] = *reinterpret_cast<const u32x4*>(p);
      hr.hb[i] = *reinterpret_cast<const u32x4*>(p + 64);
    } else {
      hr.h[i] = *reinterpret_cast<const u32x4*>(a.x + (((size_t)t.n * a.H + gy) * a.W + gx) * C + c);
    }
  }
}

// POOL: the second half of chunk ch's halo (source row 2 y + 1) and the affine
__device__ __forceinline__ void issue_halo_b(const Args& a, TileXY t, int ch, int gt, Halo<true>& hr) {
  const int c = ch * 32 + (gt & 3) * 8;
  issue_aff(a, t, c, hr);
#pragma unroll
  for (int i = 0; i < HUPT; ++i) {
    const int pi = min(gt + i * GT, HU - 1) >> 2;
    const int y = pi / IW, x = pi - y * IW;
    const int gy = min(max(t.ty0 - 1 + y, 0), a.H - 1);
    const int gx = min(max(t.tx0 - 1 + x, 0), a.W - 1);
    const bf16_t* p = a.x + pool_src(a, t.n, gy, gx, 1, c);
    hr.q[i] = *reinterpret_cast<const u32x4*>(p);
    hr.qb[i] = *reinterpret_cast<const u32x4*>(p + 64);
  }
}

// PROJ: the projection's scale / shift of chunk ch's channels of this thread
__device__ __forceinline__ void issue_affp(const Args& a, int ch, int gt, Halo<true>& hr) {
  const int c = ch * 32 + (gt & 3) * 8;
  hr.affp[0] = *reinterpret_cast<const float4*>(a.sp + c);
  hr.affp[1] = *reinterpret_cast<const float4*>(a.sp + c + 4);
  hr.affp[2] = *reinterpret_cast<const float4*>(a.tp + c);
  hr.affp[3] = *reinterpret_cast<const float4*>(a.tp + c + 4);
}

// POOL: the maximum of the four raw values in conv2d_nhwc_kernel's order, max(max(r0, r1), max(q0, q1)),
// packed again (the max of bf16 values is exact in bf16), in two steps so that a commit never holds all
// four: reduce_a, h <- max(h, hb), as soon as the first half is in and before the second is issued
// behind it; reduce_b, h <- max(h, max(q, qb)).  commit() then sees h as the plain build's halo.
__device__ __forceinline__ uint32_t max_bf16x2(uint32_t p, uint32_t q) {
  const float lo = fmaxf(lo_bf(p), lo_bf(q)), hi = fmaxf(hi_bf(p), hi_bf(q));
  return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}

__device__ __forceinline__ void reduce_a(Halo<true>& hr) {
#pragma unroll
  for (int i = 0; i < HUPT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) hr.h[i][j] = max_bf16x2(hr.h[i][j], hr.hb[i][j]);
}

__device__ __forceinline__ void reduce_b(Halo<true>& hr) {
#pragma unroll
  for (int i = 0; i < HUPT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) hr.h[i][j] = max_bf16x2(hr.h[i][j], max_bf16x2(hr.q[i][j], hr.qb[i][j]));
}

// P1: activation -> bf16 -> the swizzled input image (zero outside the image: conv padding applies
// after the activation)
template <bool POOL>
__device__ __forceinline__ void commit(const Args& a, TileXY t, int gt, const Halo<POOL>& hr, unsigned char* rin) {
  const int c = gt & 3;
  const float sc[8] = {hr.aff[0].x, hr.aff[0].y, hr.aff[0].z, hr.aff[0].w, hr.aff[1].x, hr.aff[1].y, hr.aff[1].z, hr.aff[1].w};
  const float sh[8] = {hr.aff[2].x, hr.aff[2].y, hr.aff[2].z, hr.aff[2].w, hr.aff[3].x, hr.aff[3].y, hr.aff[3].z, hr.aff[3].w};
  const bool relu = a.relu != 0;
#pragma unroll
  for (int i = 0; i < HUPT; ++i) {
    const int u = gt + i * GT;
    if (u >= HU) continue;
    const int pi = u >> 2;
    const int y = pi / IW, x = pi - y * IW;
    const int gy = t.ty0 - 1 + y, gx = t.tx0 - 1 + x;
    u32x4 pk = (u32x4){0u, 0u, 0u, 0u};
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float lo = lo_bf(hr.h[i][j]), hi = hi_bf(hr.h[i][j]);
        pk[j] = pack2bf(fmaf(lo, sc[2 * j], sh[2 * j]), fmaf(hi, sc[2 * j + 1], sh[2 * j + 1]));
        if (relu) pk[j] = relu_bf16x2(pk[j]);
      }
    }
    *reinterpret_cast<u32x4*>(rin + pi * 64 + ((c ^ (((x >> 1) & 1) << 1)) << 4)) = pk;
  }
}

// PROJ: the pooled values (h after reduce_b) of the tile's centre pixels under the projection's affine,
// no ReLU, rounded to bf16 -> the group's second image, channel units 4 ch + c.  A 1x1 conv has no
// padding and pixels outside the image are never stored, so every centre pixel is written as it is.
__device__ __forceinline__ void commit_proj(int ch, int gt, const Halo<true>& hr, unsigned char* rpj) {
  const int c = gt & 3;
  const float sc[8] = {hr.affp[0].x, hr.affp[0].y, hr.affp[0].z, hr.affp[0].w, hr.affp[1].x, hr.affp[1].y, hr.affp[1].z, hr.affp[1].w};
  const float sh[8] = {hr.affp[2].x, hr.affp[2].y, hr.affp[2].z, hr.affp[2].w, hr.affp[3].x, hr.affp[3].y, hr.affp[3].z, hr.affp[3].w};
#pragma unroll
  for (int i = 0; i < HUPT; ++i) {
    const int u = gt + i * GT;
    if (u >= HU) continue;
    const int pi = u >> 2;
    const int y = pi / IW, x = pi - y * IW;
    if (y < 1 || y > TH || x < 1 || x > TW) continue;
    const int py = y - 1, px = x - 1;
    u32x4 pj;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      pj[j] = pack2bf(fmaf(lo_bf(hr.h[i][j]), sc[2 * j], sh[2 * j]), fmaf(hi_bf(hr.h[i][j]), sc[2 * j + 1], sh[2 * j + 1]));
    *reinterpret_cast<u32x4*>(rpj + (py * TW + px) * 128 + (((ch * 4 + c) ^ (((px >> 1) & 1) << 1) ^ ((py & 1) << 2)) << 4)) = pj;
  }
}

// The first WD K-steps' weight fragments of an MFMA phase, issued in the commit before it.
struct WPre {
  bf16x8 w[WD][2];
};

// wf: the conv's fragment-order weights; lane: 0..63, cp: channel-tile pair 0..3
__device__ __forceinline__ const bf16_t* w_lane(const bf16_t* wf, int cp, int lane) {
  return wf + cp * 2 * 512 + lane * 8;
}

__device__ __forceinline__ void issue_w(const bf16_t* wl, WPre& p) {
#pragma unroll
  for (int d = 0; d < WD; ++d)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) p.w[d][ct] = *reinterpret_cast<const bf16x8*>(wl + d * WSTEP + ct * 512);
}

// P2: the 9 taps of one input chunk over 14 pixel fragments x 2 channel tiles.  Pixel fragments go
// through a ring of BR registers, read BD fragments (2 BD MFMAs) ahead; weight fragments come from
// global memory WD steps ahead.  A0[dx]: this lane's byte address of patch pixel (ly, lx + dx).
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[2][NF], const unsigned char* rin, const bf16_t* wl, const WPre& pre,
                                          const int (&A0)[3]) {
  bf16x8 w[9][2];  // fully unrolled: WD + 1 steps are live at a time
#pragma unroll
  for (int d = 0; d < WD; ++d) {
    w[d][0] = pre.w[d][0];
    w[d][1] = pre.w[d][1];
  }
  auto rd = [&](int f) {
    const int s = f / NF, j = f % NF, dy = s / 3, dx = s % 3;
    return *reinterpret_cast<const bf16x8*>(rin + A0[dx] + ((4 * (j / FC) + dy) * IW + 4 * (j % FC)) * 64);
  };
  bf16x8 bf[BR];
#pragma unroll
  for (int f = 0; f < BD; ++f) bf[f] = rd(f);
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    if (s + WD < 9) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        w[s + WD][ct] = *reinterpret_cast<const bf16x8*>(wl + (s + WD) * WSTEP + ct * 512);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int f = s * NF + j;
      if (f + BD < 9 * NF) bf[(f + BD) % BR] = rd(f + BD);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[s][ct], bf[f % BR], acc[ct][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// PROJ: the 1x1 projection of the tile's centre pixels from zero accumulators, conv2d_nhwc_kernel<1, 64,
// 64, 2, ...>'s two 32-deep K-steps (channels 0-31, then 32-63; lane group kq holds channels 8 kq..8 kq + 7
// of the step).  wl: w_lane of the projection's fragment-order weights.
__device__ __forceinline__ void proj_mma(f32x4 (&acc)[2][NF], const unsigned char* rpj, const bf16_t* wl, int lrow, int kq) {
  bf16x8 w[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) w[s][ct] = *reinterpret_cast<const bf16x8*>(wl + s * WSTEP + ct * 512);
  const int ly = lrow >> 2, lx = lrow & 3;
  const int P0 = (ly * TW + lx) * 128 + ((kq ^ (((lx >> 1) & 1) << 1) ^ ((ly & 1) << 2)) << 4);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto rd = [&](int f) {
    const int s = f / NF, j = f % NF;
    return *reinterpret_cast<const bf16x8*>(rpj + (P0 ^ (s << 6)) + (4 * (j / FC) * TW + 4 * (j % FC)) * 128);
  };
  constexpr int PD = 3, PR = 4;  // read PD fragments ahead, ring of PR
  bf16x8 bf[PR];
#pragma unroll
  for (int f = 0; f < PD; ++f) bf[f] = rd(f);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int f = 0; f < 2 * NF; ++f) {
    if (f + PD < 2 * NF) bf[(f + PD) % PR] = rd(f + PD);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
      acc[ct][f % NF] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[f / NF][ct], bf[f % PR], acc[ct][f % NF], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// P3: (acc + bias) + residual -> bf16 -> 8-byte stores (4 channels of one pixel per lane; the four kq
// lanes of a pixel write 32 contiguous bytes per channel tile).  Straight-line buffer accesses: a
// branch per store makes the compiler's wait-count pass wait for ALL outstanding memory operations at
// every join.  RES: with a residual.  Without one the per-layer kernel still adds a +0.0f residual,
// which only matters when acc + bias is -0.0, i.e. when both are; adding +0.0f to the BIAS once gives
// the same bits for 8 VALU operations per tile.  FULL: the tile lies inside the image (every tile at
// 56^2), so one per-lane offset serves all 28 accesses and the fragment's offset is scalar; otherwise
// pixels outside the image get an out-of-range offset, which the descriptor's range check drops, as do
// tiles that are not this group's.  Every residual is loaded before the first store: `out` may be the
// residual.  RES 2: the residual is [N, H/2, W/2, 128] and pixel (py, px) reads (py >> 1, px >> 1)
// through a descriptor of that image's size (a 1x1 projection of an up-sampled map, computed before
// the up-sampling: a quarter of the bytes).  Tile and patch origins are even (8, 28, 4), so
// (origin + y) >> 1 = origin / 2 + (y >> 1) and the FULL form keeps its scalar fragment offsets.
template <int RES, bool FULL>
__device__ __forceinline__ void epilogue(const Args& a, TileXY t, const f32x4 (&acc)[2][NF], int cp, int lrow, int kq,
                                         bool act) {
  const int ly = lrow >> 2, lx = lrow & 3;
  const int co = cp * 32 + kq * 4;
  const int img_b = a.H * a.W * C * 2;  // host-checked: < 2^31
  const size_t img = (size_t)t.n * a.H * a.W * C;
  const int Wr = a.W >> 1;
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(RES == 2 ? a.res + (size_t)t.n * (a.H >> 1) * Wr * C : (RES ? a.res + img : a.x)), (short)0,
      RES == 2 ? (a.H >> 1) * Wr * C * 2 : (RES ? img_b : 0), 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.out + img, (short)0, img_b, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.bias ? a.bias : a.sa), (short)0, a.bias ? C * 4 : 0, 0x00020000);  // null: loads give 0
  // byte offset of this lane's 4 channels of fragment j's pixel: per-lane part, scalar part
  auto voff = [&](int j, int y, int x) {
    if constexpr (FULL) return (((t.ty0 + y) * a.W + t.tx0 + x) * C + co) * 2;
    const int py = t.ty0 + 4 * (j / FC) + y, px = t.tx0 + 4 * (j % FC) + x;
    return (py < a.H && px < a.W) ? ((py * a.W + px) * C + co) * 2 : 0x7ffffff0;
  };
  auto soff = [&](int j) { return FULL ? ((j / FC) * 4 * a.W + (j % FC) * 4) * C * 2 : 0; };
  // the same pair for the half-resolution residual
  auto voff_r = [&](int j, int y, int x) {
    if constexpr (FULL) return ((((t.ty0 + y) >> 1) * Wr + ((t.tx0 + x) >> 1)) * C + co) * 2;
    const int py = t.ty0 + 4 * (j / FC) + y, px = t.tx0 + 4 * (j % FC) + x;
    return (py < a.H && px < a.W) ? (((py >> 1) * Wr + (px >> 1)) * C + co) * 2 : 0x7ffffff0;
  };
  auto soff_r = [&](int j) { return FULL ? ((j / FC) * 2 * Wr + (j % FC) * 2) * C * 2 : 0; };
  u32x2 rv[RES ? NF : 1][2];
  f32x4 bias[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
    bias[ct] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (co + ct * 16) * 4, 0, 0));
  if constexpr (RES != 0) {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int o = RES == 2 ? voff_r(j, ly, lx) : voff(j, ly, lx);
      const int so = RES == 2 ? soff_r(j) : soff(j);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) rv[j][ct] = __builtin_amdgcn_raw_buffer_load_b64(rr, o + ct * 32, so, 0);
    }
  } else {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) bias[ct] = bias[ct] + (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __builtin_amdgcn_sched_barrier(0);
  int sy = ly, sx = lx;
  asm volatile("" : "+v"(sy), "+v"(sx));  // the store offsets are formed again, not kept across the loads
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int o = act ? voff(j, sy, sx) : 0x7ffffff0;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      u32x2 st;
      if constexpr (RES != 0) {
        const u32x2 r = rv[j][ct];
        st[0] = pack2bf(acc[ct][j][0] + bias[ct][0] + lo_bf(r[0]), acc[ct][j][1] + bias[ct][1] + hi_bf(r[0]));
        st[1] = pack2bf(acc[ct][j][2] + bias[ct][2] + lo_bf(r[1]), acc[ct][j][3] + bias[ct][3] + hi_bf(r[1]));
      } else {
        st[0] = pack2bf(acc[ct][j][0] + bias[ct][0], acc[ct][j][1] + bias[ct][1]);
        st[1] = pack2bf(acc[ct][j][2] + bias[ct][2], acc[ct][j][3] + bias[ct][3]);
      }
      __builtin_amdgcn_raw_buffer_store_b64(st, ro, o + ct * 32, soff(j), 0);
    }
  }
}

// C256: P3 of one 128-channel half (`half` 0 / 1) of a 256-channel output with the per-layer kernel's
// post-activation (post_affine in conv2d_nhwc.hip): (acc + bias) rounded to bf16, fmaf(v, qs[co],
// qt[co]), one more rounding, ReLU (a.qrelu).  No residual, so the +0.0f goes to the bias as in
// epilogue<0>.  The output pixel stride is 256 channels and this half's channels start at 128 half;
// bias, qs and qt are [256].  FULL and the dropped out-of-range offsets as in epilogue().
template <bool FULL>
__device__ __forceinline__ void epilogue_c256(const Args& a, TileXY t, int half, const f32x4 (&acc)[2][NF], int cp, int lrow,
                                              int kq, bool act) {
  constexpr int CO = 2 * C;
  const int ly = lrow >> 2, lx = lrow & 3;
  const int co = half * C + cp * 32 + kq * 4;
  const int img_b = a.H * a.W * CO * 2;  // host-checked: < 2^31
  const __amdgpu_buffer_rsrc_t ro =
      __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)t.n * a.H * a.W * CO, (short)0, img_b, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.bias ? a.bias : a.qs), (short)0, a.bias ? CO * 4 : 0, 0x00020000);  // null: loads give 0
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.qs), (short)0, CO * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.qt), (short)0, CO * 4, 0x00020000);
  auto voff = [&](int j, int y, int x) {
    if constexpr (FULL) return (((t.ty0 + y) * a.W + t.tx0 + x) * CO + co) * 2;
    const int py = t.ty0 + 4 * (j / FC) + y, px = t.tx0 + 4 * (j % FC) + x;
    return (py < a.H && px < a.W) ? ((py * a.W + px) * CO + co) * 2 : 0x7ffffff0;
  };
  auto soff = [&](int j) { return FULL ? ((j / FC) * 4 * a.W + (j % FC) * 4) * CO * 2 : 0; };
  f32x4 bias[2], qs[2], qt[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    bias[ct] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (co + ct * 16) * 4, 0, 0));
    qs[ct] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (co + ct * 16) * 4, 0, 0));
    qt[ct] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rt, (co + ct * 16) * 4, 0, 0));
    bias[ct] = bias[ct] + (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const bool qrelu = a.qrelu != 0;
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int o = act ? voff(j, ly, lx) : 0x7ffffff0;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const uint32_t p0 = pack2bf(acc[ct][j][0] + bias[ct][0], acc[ct][j][1] + bias[ct][1]);
      const uint32_t p1 = pack2bf(acc[ct][j][2] + bias[ct][2], acc[ct][j][3] + bias[ct][3]);
      u32x2 st;
      st[0] = pack2bf(fmaf(lo_bf(p0), qs[ct][0], qt[ct][0]), fmaf(hi_bf(p0), qs[ct][1], qt[ct][1]));
      st[1] = pack2bf(fmaf(lo_bf(p1), qs[ct][2], qt[ct][2]), fmaf(hi_bf(p1), qs[ct][3], qt[ct][3]));
      if (qrelu) {
        st[0] = relu_bf16x2(st[0]);
        st[1] = relu_bf16x2(st[1]);
      }
      __builtin_amdgcn_raw_buffer_store_b64(st, ro, o + ct * 32, soff(j), 0);
    }
  }
}

// POOL: the level-2 entry conv, 64 -> 128 channels: x is [N, 2 H, 2 W, 64] and is read through a 2 x 2
// max-pool (conv2d_nhwc_kernel's INMODE 2), two 32-channel chunks (six phases per tile), weights
// [2 chunks][9 taps][8 ct] in the same fragment order, no residual.  PROJ (with POOL): the level's 1x1
// projection of the same pooled pixels as a second output (Args::out2), computed after the epilogue on
// the freed accumulators.
//
// C256 (without POOL): 128 -> 256 channels as two 128-channel halves (CPnet's level-3 entry conv on the
// pooled tensor, conv2d_nhwc_kernel<3, 32, 64, 0, ...> with its post-activation bit for bit).  A work
// item is (tile, half): item i is half i & 1 of tile i >> 1, so the two halves of a tile are consecutive
// items, one per group, and the second finds the input in the cache.  Weights are [2 halves][4 chunks]
// [9 taps][8 ct] (each half in the 128 -> 128 fragment order); the epilogue is epilogue_c256.
template <bool STAMP = false, bool POOL = false, bool PROJ = false, bool C256 = false>
__global__ __launch_bounds__(NTP, 2) void conv_pp128_kernel(Args a) {
  static_assert(POOL || !PROJ, "the projection reads the pooled input");
  static_assert(!(POOL && C256), "the 256-channel build reads a plain 128-channel input");
  constexpr int NC = POOL ? 2 : NCH;
  // STAMP: as conv_pair_pp64_kernel; slots: commit / MFMA of chunk 0, of chunks 1..3 together, epilogue;
  // work cycles of slot i at i, the wait at its closing barrier at 8 + i, iterations at 15
  unsigned long long ph_work[5] = {0, 0, 0, 0, 0}, ph_wait[5] = {0, 0, 0, 0, 0};
  unsigned long long tstamp = STAMP ? __builtin_amdgcn_s_memtime() : 0;
  auto pre = [&](int i) {
    if constexpr (STAMP) {
      const unsigned long long tn = __builtin_amdgcn_s_memtime();
      ph_work[i] += tn - tstamp;
      tstamp = tn;
    }
  };
  auto post = [&](int i) {
    if constexpr (STAMP) {
      const unsigned long long tn = __builtin_amdgcn_s_memtime();
      ph_wait[i] += tn - tstamp;
      tstamp = tn;
    }
  };
  auto slot = [](int c) { return c > 0 ? 2 : 0; };
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid0 = threadIdx.x;
  const int total = a.N * a.tiles_x * a.tiles_y * (C256 ? 2 : 1);  // work items
  auto tile_at = [&](int item) { return tile_of(a, C256 ? item >> 1 : item); };
  const int t0 = (int)(((long long)blockIdx.x * total) / gridDim.x);
  const int t1 = (int)(((long long)(blockIdx.x + 1) * total) / gridDim.x);
  if (t0 >= t1) return;  // workgroup-uniform
  const int grp = __builtin_amdgcn_readfirstlane(tid0 / GT);  // waves w and w + 4 share a SIMD
  const int gt0 = tid0 & (GT - 1);
  unsigned char* reg = smem + grp * IN_B;
  unsigned char* rpj = PROJ ? smem + LDS + grp * PJ_B : nullptr;
  Halo<POOL> halo;
  issue_halo(a, tile_at(min(t0 + grp, t1 - 1)), 0, gt0, halo);
  if constexpr (POOL) issue_halo_b(a, tile_at(min(t0 + grp, t1 - 1)), 0, gt0, halo);
  if constexpr (PROJ) issue_affp(a, 0, gt0, halo);
  if (grp == 1) __builtin_amdgcn_s_barrier();  // the stagger: group 1 runs one phase behind
  const int iters = (t1 - t0 + 1) >> 1;
  for (int k = 0; k < iters; ++k) {
    int gt = gt0;
    asm volatile("" : "+v"(gt));  // per-iteration opaque copy: no addresses hoisted out of the tile loop
    const int cp = __builtin_amdgcn_readfirstlane(gt >> 6), lane = gt & 63, lrow = lane & 15, kq = lane >> 4;
    const int t = t0 + 2 * k + grp;
    // a group without a tile in the last iteration (odd range) recomputes the range's last tile and
    // stores nothing
    const bool act = t < t1;
    const TileXY cur = tile_at(act ? t : t1 - 1);
    const bf16_t* wl = w_lane(C256 ? a.wf + ((act ? t : t1 - 1) & 1) * (NCH * 9 * WSTEP) : a.wf, cp, lane);
    int A0[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int x = (lrow & 3) + dx;
      A0[dx] = ((lrow >> 2) * IW + x) * 64 + ((kq ^ (((x >> 1) & 1) << 1)) << 4);
    }
    f32x4 acc[2][NF];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    WPre wpre;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      // P1: input chunk c -> activated image.  Behind it the next chunk's halo (or the group's next
      // tile's first) and then the first weight fragments of this chunk's MFMA phase.  Loads return in
      // issue order: a halo issued inside the MFMA phase held every later weight fragment back until
      // the halo had arrived from HBM (MFMA phases of 5.8-8k cycles for 4k of MFMAs).  Issued here, it
      // travels while the group waits at the barrier for the other group's MFMA phase to end.
      int gc = gt0;
      asm volatile("" : "+v"(gc));
      if constexpr (POOL) {
        reduce_a(halo);
        if (c > 0) {
          __builtin_amdgcn_sched_barrier(0);
          issue_halo_b(a, cur, c, gc, halo);
        }
        reduce_b(halo);
        if constexpr (PROJ) {
          if (c > 0) {
            __builtin_amdgcn_sched_barrier(0);
            issue_affp(a, c, gc, halo);
          }
        }
      }
      commit(a, cur, gc, halo, reg);
      if constexpr (PROJ) {
        __builtin_amdgcn_sched_barrier(0);
        commit_proj(c, gc, halo, rpj);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (c + 1 < NC)
        issue_halo(a, cur, c + 1, gc, halo);
      else
        issue_halo(a, tile_at(min(t + 2, t1 - 1)), 0, gc, halo);
      issue_w(wl + c * 9 * WSTEP, wpre);
      pre(slot(c));
      __syncthreads();
      post(slot(c));
      // P2: the chunk's MFMAs
      __builtin_amdgcn_s_setprio(1);
      mma_chunk(acc, reg, wl + c * 9 * WSTEP, wpre, A0);
      __builtin_amdgcn_s_setprio(0);
      pre(slot(c) + 1);
      __syncthreads();
      post(slot(c) + 1);
    }
    // P3: output epilogue
    int g3 = gt0;
    asm volatile("" : "+v"(g3));
    const bool full = cur.ty0 + TH <= a.H && cur.tx0 + TW <= a.W;  // workgroup-uniform, as a.res is
    if constexpr (POOL) {
      // the second half of the next tile's first halo travels during the epilogue and the barrier wait
      // (PROJ: during the barrier wait only; the projection needs the accumulators' registers once more)
      if constexpr (!PROJ) {
        issue_halo_b(a, tile_at(min(t + 2, t1 - 1)), 0, g3, halo);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (full)
        epilogue<0, true>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
      else
        epilogue<0, false>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
      if constexpr (PROJ) {
        __builtin_amdgcn_sched_barrier(0);
        int g4 = gt0;
        asm volatile("" : "+v"(g4));
        proj_mma(acc, rpj, w_lane(a.wpf, cp, g4 & 63), g4 & 15, (g4 & 63) >> 4);
        Args b = a;
        b.out = a.out2;
        b.bias = a.bias_p;
        if (full)
          epilogue<0, true>(b, cur, acc, cp, g4 & 15, (g4 & 63) >> 4, act);
        else
          epilogue<0, false>(b, cur, acc, cp, g4 & 15, (g4 & 63) >> 4, act);
        __builtin_amdgcn_sched_barrier(0);
        issue_halo_b(a, tile_at(min(t + 2, t1 - 1)), 0, g4, halo);
        issue_affp(a, 0, g4, halo);
      }
    } else if constexpr (C256) {
      const int half = (act ? t : t1 - 1) & 1;
      if (full)
        epilogue_c256<true>(a, cur, half, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
      else
        epilogue_c256<false>(a, cur, half, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
    } else if (a.res != nullptr && a.res_up2) {
      if (full)
        epilogue<2, true>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
      else
        epilogue<2, false>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
    } else if (a.res != nullptr) {
      if (full)
        epilogue<1, true>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
      else
        epilogue<1, false>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
    } else {
      if (full)
        epilogue<0, true>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
      else
        epilogue<0, false>(a, cur, acc, cp, g3 & 15, (g3 & 63) >> 4, act);
    }
    pre(4);
    __syncthreads();
    post(4);
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();  // balance the stagger
  if constexpr (STAMP) {
    if ((tid0 & (GT - 1)) < 16) {  // wave 0 of each group: lane k stores slot k
      const int k = tid0 & 15;
      unsigned long long v = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        if (k == i) v = ph_work[i];
        if (k == 8 + i) v = ph_wait[i];
      }
      if (k == 15) v = (unsigned long long)iters;
      a.stamps[((size_t)blockIdx.x * 2 + grp) * 16 + k] = v;
    }
  }
}
}  // namespace pp128

// BE_CONV_PP128 (default 1, A/B): 0 keeps every call on conv2d_nhwc_kernel
int g_pp128 = be_env_int("BE_CONV_PP128", 1);

// BE_CONV_PP128_RES_UP2 (default 1, A/B): 0 makes be_conv_pp128_takes_res_up2 answer 0, so callers
// keep a full-resolution residual
int g_pp128_res_up2 = be_env_int("BE_CONV_PP128_RES_UP2", 1);

// BE_CONV_PP128_POOL (default 1, A/B): 0 keeps the pooled 64 -> 128 entry conv on conv2d_nhwc_kernel
int g_pp128_pool = be_env_int("BE_CONV_PP128_POOL", 1);

// BE_CONV_PP128_POOL_PROJ (default 1, A/B): 0 makes be_conv_pp128_takes_pool_proj answer 0, so the
// level's 1x1 projection stays a launch of its own beside the pooled build
int g_pp128_pool_proj = be_env_int("BE_CONV_PP128_POOL_PROJ", 1);

// BE_CPNET_L3_PREPOOL (default 1, A/B): 0 makes be_conv_pp128_takes_prepool answer 0, so CPnet's level-3
// entry keeps its two pooled-input launches of the per-layer kernel
int g_l3_prepool = be_env_int("BE_CPNET_L3_PREPOOL", 1);

// BE_CONV_PP128_C256 (default 1, A/B): 0 makes be_conv_pp128_takes_c256 answer 0, so the 128 -> 256
// entry conv of a pre-pooled level stays on conv2d_nhwc_kernel
int g_pp128_c256 = be_env_int("BE_CONV_PP128_C256", 1);

int g_pp128_c256_launches = 0;  // be_conv_pp128_c256_launches
int g_pp128_grid = 0;      // be_conv_pp128_set_grid (0 = one workgroup per CU)
int g_pp128_launches = 0;  // be_conv_pp128_launches
int g_pp128_pool_launches = 0;  // be_conv_pp128_pool_launches
unsigned long long* g_pp128_stamps = nullptr;  // diagnostics: be_conv_pp128_set_stamps
int g_pp128_stamps_cap = 0;                    // workgroups the stamp buffer holds

// The size rule, in one place: the grid on which a 3x3 128 -> 128 call of N images of H x W runs on
// conv_pp128_kernel, or 0 when it stays on the per-layer kernel (switched off, too few tiles for the
// grid that is not forced, or too large for 32-bit offsets).
// halves = 2: the 256-channel build, whose work items are (tile, 128-channel half) and whose output
// image is twice as large; the rule then counts items where it counts tiles.
int pp128_grid_for(int N, int H, int W, int* tiles_x, int* tiles_y, int halves = 1) {
  if (!g_pp128 || N <= 0 || H <= 0 || W <= 0 || (long long)H * W * 256 * halves >= (1LL << 31) - 64) return 0;
  const int tx = (W + pp128::TW - 1) / pp128::TW, ty = (H + pp128::TH - 1) / pp128::TH;
  const long long tiles = (long long)N * tx * ty * halves;
  const bool forced = g_pp128_grid > 0;
  const int g = forced ? (int)(tiles < g_pp128_grid ? tiles : g_pp128_grid) : 256;
  if (!(forced || tiles >= 2LL * g) || tiles >= (1LL << 30)) return 0;
  if (tiles_x) *tiles_x = tx;
  if (tiles_y) *tiles_y = ty;
  return g;
}

// The fields every build shares; an entry point sets on top only what is its own (tiles_x / tiles_y come
// from pp128_grid_for, everything else stays at Args' defaults).
pp128::Args pp128_args(const void* x, const float* pscale, const float* pshift, int pshift_ns, int pscale_ns, int prelu,
                       const void* wfrag, const float* bias, void* out, int N, int H, int W) {
  pp128::Args a;
  a.x = (const bf16_t*)x; a.sa = pscale; a.ta = pshift; a.sa_ns = pscale_ns; a.ta_ns = pshift_ns;
  a.wf = (const bf16_t*)wfrag; a.bias = bias; a.out = (bf16_t*)out;
  a.N = N; a.H = H; a.W = W; a.relu = prelu & 1;
  a.stamps = g_pp128_stamps;
  return a;
}

// One launch of the <POOL, PROJ, C256> build on `grid` workgroups: the phase-stamped instantiation when a
// stamp buffer is set (diagnostics: be_conv_pp128_set_stamps; -30 if it is too small for the grid), the
// PROJ build's larger LDS with its once-per-device attribute (-33).
template <bool POOL, bool PROJ, bool C256>
int pp128_launch(const pp128::Args& a, int grid, hipStream_t stream) {
  constexpr int lds = PROJ ? pp128::LDS_PROJ : pp128::LDS;
  if constexpr (PROJ) {
    static bool attr_set[BE_MAX_DEV] = {};
    if (!attr_set[be_cur_dev()]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&pp128::conv_pp128_kernel<false, POOL, PROJ, C256>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
          hipFuncSetAttribute(reinterpret_cast<const void*>(&pp128::conv_pp128_kernel<true, POOL, PROJ, C256>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return -33;
      attr_set[be_cur_dev()] = true;
    }
  }
  if (a.stamps != nullptr) {
    if (grid > g_pp128_stamps_cap) return -30;
    hipLaunchKernelGGL((pp128::conv_pp128_kernel<true, POOL, PROJ, C256>), dim3(grid), dim3(pp128::NTP), lds, stream, a);
  } else {
    hipLaunchKernelGGL((pp128::conv_pp128_kernel<false, POOL, PROJ, C256>), dim3(grid), dim3(pp128::NTP), lds, stream, a);
  }
  return BE_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int be_conv2d_nhwc(const void* x, const void* x2, const float* pscale, const float* pshift, int pshift_ns, int pscale_ns,
                   int prelu, const void* w, const float* bias, const void* res, void* out, int N, int H, int W,
                   int Hs, int Ws, int Cin, int Cout, int cout_valid, int ks, int ck, int tco, int inmode,
                   int out_f32_nchw, int nw, const float* qscale, const float* qshift, int qshift_ns,
                   hipStream_t stream);

// Tests / tuning: the ping-pong kernel's grid (0 = 256, one workgroup per CU, and the tile-count
// rule of be_conv2d_nhwc_frag).  A positive value forces every eligible call onto the kernel with
// at most that many workgroups, however few tiles it has: uneven ranges, idle groups' dummy tiles.
int be_conv_pp128_set_grid(int blocks) {
  g_pp128_grid = blocks;
  return 0;
}

// Diagnostics: eligible calls run the phase-stamped build, which writes [workgroup][group][16] u64
// cycle counts into `buf` (device, >= cap_workgroups * 256 bytes); nullptr switches back.  Not for
// production launches.
int be_conv_pp128_set_stamps(void* buf, int cap_workgroups) {
  g_pp128_stamps = static_cast<unsigned long long*>(buf);
  g_pp128_stamps_cap = buf ? cap_workgroups : 0;
  return 0;
}

// Launches of conv_pp128_kernel by this process so far (tests: which kernel did a call take).
int be_conv_pp128_launches() { return g_pp128_launches; }

// be_conv2d_nhwc with the weights once more in MFMA-fragment order (ops/conv.py pack_frag; wfrag may be
// null).  A 3x3, Cin = Cout = 128, INMODE 0, no-x2, bf16-NHWC-output call without an output
// activation runs on conv_pp128_kernel when every group of every workgroup gets at least two 8 x 28
// tiles (as pp64_ok: batch-1 latency calls would only recompute dummy tiles) or the grid is forced
// (be_conv_pp128_set_grid); every other call goes to be_conv2d_nhwc unchanged.  Under the same size
// rule a 3x3, Cin = 64, Cout = 128, INMODE 2 call from an even source, without a residual, runs on the
// kernel's pooled build (be_conv_pp128_takes_pool).
//
// res_up2 != 0: `res` is [N, H/2, W/2, 128] and is read through nearest 2x up-sampling.  Only the
// ping-pong kernel has that epilogue: the caller asks be_conv_pp128_takes_res_up2 first, and a call
// that the kernel does not take is an error (-31), not a fallback.
int be_conv2d_nhwc_frag_res(const void* x, const void* x2, const float* pscale, const float* pshift, int pshift_ns,
                            int pscale_ns, int prelu, const void* w, const float* bias, const void* res, void* out,
                            int N, int H, int W, int Hs, int Ws, int Cin, int Cout, int cout_valid, int ks, int ck,
                            int tco, int inmode, int out_f32_nchw, int nw, const float* qscale, const float* qshift,
                            int qshift_ns, const void* wfrag, int res_up2, hipStream_t stream) {
  // what the plain and the pooled call have in common
  const bool frag_ok = wfrag && ks == 3 && ck == 32 && !x2 && !out_f32_nchw && Cout == 128 && !(prelu & 2) && !qscale &&
                       !qshift && x && out;
  const bool shape_ok = frag_ok && inmode == 0 && Cin == 128 && Hs == H && Ws == W;
  if (res_up2 && !(shape_ok && res && H % 2 == 0 && W % 2 == 0)) return -31;
  // the pooled entry conv: 3x3, 64 -> 128, INMODE 2 from an even source, no residual
  const bool pool_ok = frag_ok && g_pp128_pool && inmode == 2 && Cin == 64 && Hs == 2 * H && Ws == 2 * W && !res;
  if (shape_ok || pool_ok) {
    pp128::Args a = pp128_args(x, pscale, pshift, pshift_ns, pscale_ns, prelu, wfrag, bias, out, N, H, W);
    const int g = pp128_grid_for(N, H, W, &a.tiles_x, &a.tiles_y);
    if (g > 0 && pool_ok) {
      ++g_pp128_pool_launches;
      return pp128_launch<true, false, false>(a, g, stream);
    }
    if (g > 0) {
      a.res = (const bf16_t*)res;
      a.res_up2 = res_up2 ? 1 : 0;
      ++g_pp128_launches;
      return pp128_launch<false, false, false>(a, g, stream);
    }
  }
  if (res_up2) return -31;
  return be_conv2d_nhwc(x, x2, pscale, pshift, pshift_ns, pscale_ns, prelu, w, bias, res, out, N, H, W, Hs, Ws, Cin, Cout,
                        cout_valid, ks, ck, tco, inmode, out_f32_nchw, nw, qscale, qshift, qshift_ns, stream);
}

int be_conv2d_nhwc_frag(const void* x, const void* x2, const float* pscale, const float* pshift, int pshift_ns,
                        int pscale_ns, int prelu, const void* w, const float* bias, const void* res, void* out, int N,
                        int H, int W, int Hs, int Ws, int Cin, int Cout, int cout_valid, int ks, int ck, int tco,
                        int inmode, int out_f32_nchw, int nw, const float* qscale, const float* qshift, int qshift_ns,
                        const void* wfrag, hipStream_t stream) {
  return be_conv2d_nhwc_frag_res(x, x2, pscale, pshift, pshift_ns, pscale_ns, prelu, w, bias, res, out, N, H, W, Hs, Ws,
                                 Cin, Cout, cout_valid, ks, ck, tco, inmode, out_f32_nchw, nw, qscale, qshift,
                                 qshift_ns, wfrag, 0, stream);
}

// 1 if a be_conv2d_nhwc_frag call of the kernel's shape (3x3, 128 -> 128, fragment-order weights, no
// input transform, bf16 NHWC output) with N images of H x W runs on conv_pp128_kernel now: the size
// rule above under the present BE_CONV_PP128 and be_conv_pp128_set_grid.
int be_conv_pp128_takes(int N, int H, int W) { return pp128_grid_for(N, H, W, nullptr, nullptr) > 0 ? 1 : 0; }

// 1 if a be_conv2d_nhwc_frag call of the pooled entry shape (3x3, 64 -> 128, INMODE 2, fragment-order
// weights, no residual, bf16 NHWC output) with N source images of Hs x Ws runs on the kernel's pooled
// build now: an even source size, the size rule of the Hs/2 x Ws/2 output, BE_CONV_PP128_POOL.
int be_conv_pp128_takes_pool(int N, int Hs, int Ws) {
  return g_pp128_pool && Hs % 2 == 0 && Ws % 2 == 0 && pp128_grid_for(N, Hs / 2, Ws / 2, nullptr, nullptr) > 0 ? 1 : 0;
}

// Tests / A/B runs in one process: the two switches that BE_CONV_PP128_POOL and BE_CONV_PP128_POOL_PROJ
// set when the library is loaded.
int be_conv_pp128_set_pool(int pool, int pool_proj) {
  g_pp128_pool = pool;
  g_pp128_pool_proj = pool_proj;
  return 0;
}

// Launches of the pooled builds (with or without the projection) by this process so far.  They have a
// counter of their own: be_conv_pp128_launches keeps counting the 128 -> 128 calls alone.
int be_conv_pp128_pool_launches() { return g_pp128_pool_launches; }

// 1 if be_conv_pp128_pool_proj takes N source images of Hs x Ws now: the rule above and
// BE_CONV_PP128_POOL_PROJ.
int be_conv_pp128_takes_pool_proj(int N, int Hs, int Ws) {
  return g_pp128_pool_proj && be_conv_pp128_takes_pool(N, Hs, Ws);
}

// The level-2 entry of CPnet's encoder in one launch, from x [N, Hs, Ws, 64] bf16 through a 2x2 max-pool:
//   out  = conv3x3( relu?( pool(x) * pscale + pshift[n] ) ) + bias      [N, Hs/2, Ws/2, 128]
//   out2 = conv1x1(        pool(x) * sp     + tp          ) + bias_p    likewise
// each bit for bit what be_conv2d_nhwc gives for it alone (INMODE 2; ck 32 and ck 64).  wfrag: the 3x3
// conv in pack_frag order [2][9][8][64][8]; wpfrag: the 1x1 in pack_frag_1x1 order [2][8][64][8].  The
// caller asks be_conv_pp128_takes_pool_proj first: a call the kernel does not take is an error (-32).
int be_conv_pp128_pool_proj(const void* x, const float* pscale, const float* pshift, int pshift_ns, int pscale_ns, int prelu,
                            const void* wfrag, const float* bias, void* out, const float* sp, const float* tp,
                            const void* wpfrag, const float* bias_p, void* out2, int N, int Hs, int Ws,
                            hipStream_t stream) {
  if (!x || !wfrag || !out || !sp || !tp || !wpfrag || !out2 || out == out2 || (prelu & ~1)) return -32;
  if (!be_conv_pp128_takes_pool_proj(N, Hs, Ws)) return -32;
  pp128::Args a = pp128_args(x, pscale, pshift, pshift_ns, pscale_ns, prelu, wfrag, bias, out, N, Hs / 2, Ws / 2);
  const int g = pp128_grid_for(N, Hs / 2, Ws / 2, &a.tiles_x, &a.tiles_y);
  a.sp = sp; a.tp = tp; a.wpf = (const bf16_t*)wpfrag; a.bias_p = bias_p; a.out2 = (bf16_t*)out2;
  ++g_pp128_pool_launches;
  return pp128_launch<true, true, false>(a, g, stream);
}

// The size rule of the 256-channel build, in one place: pp128_grid_for with the item count (tiles x 2
// halves) in place of the tile count.
static int pp128_c256_grid_for(int N, int H, int W, int* tiles_x, int* tiles_y) {
  return pp128_grid_for(N, H, W, tiles_x, tiles_y, 2);
}

// 1 if a level whose entry convs read a 2x2 max-pool of N source images (pooled size H x W, 128
// channels) should pool once into a tensor of its own (be_pool2_nhwc) and run both entry convs on it:
// the size rule of the 256-channel build and BE_CPNET_L3_PREPOOL.  Small calls (batch-1 requests) keep
// the pooled-input launches of the per-layer kernel.
int be_conv_pp128_takes_prepool(int N, int H, int W) {
  return g_l3_prepool && pp128_c256_grid_for(N, H, W, nullptr, nullptr) > 0 ? 1 : 0;
}

// 1 if be_conv_pp128_c256 takes N images of H x W now: be_conv_pp128_takes_prepool and BE_CONV_PP128_C256.
int be_conv_pp128_takes_c256(int N, int H, int W) { return g_pp128_c256 && be_conv_pp128_takes_prepool(N, H, W); }

// Tests / A/B runs in one process: the two switches that BE_CPNET_L3_PREPOOL and BE_CONV_PP128_C256 set
// when the library is loaded.
int be_conv_pp128_set_c256(int prepool, int c256) {
  g_l3_prepool = prepool;
  g_pp128_c256 = c256;
  return 0;
}

// Launches of the 256-channel build by this process so far; neither be_conv_pp128_launches nor
// be_conv_pp128_pool_launches counts them.
int be_conv_pp128_c256_launches() { return g_pp128_c256_launches; }

// 3x3 conv, 128 -> 256 channels, of x [N, H, W, 128] bf16 NHWC with the consumer's pre-activation applied
// to the stored value (CPnet's level-3 entry conv on the pooled tensor):
//   out = relu?( bf16( conv3x3( relu?( x * pscale + pshift[n] ) ) + bias ) * qscale + qshift )   [N, H, W, 256]
// bit for bit what be_conv2d_nhwc gives (INMODE 0, ck 32) with the same qscale / qshift [256] and prelu
// (bit 0: input ReLU, bit 1: output ReLU).  wfrag: the two 128-channel halves of the conv, each in
// pack_frag order, [2][4][9][8][64][8] (ops/conv.py, pack_frag_c256).  The caller asks
// be_conv_pp128_takes_c256 first: a call the kernel does not take is an error (-34), not a fallback.
int be_conv_pp128_c256(const void* x, const float* pscale, const float* pshift, int pshift_ns, int pscale_ns, int prelu,
                       const void* wfrag, const float* bias, void* out, const float* qscale, const float* qshift, int N,
                       int H, int W, hipStream_t stream) {
  if (!x || !wfrag || !out || x == out || !qscale || !qshift || (prelu & ~3)) return -34;
  if (!be_conv_pp128_takes_c256(N, H, W)) return -34;
  pp128::Args a = pp128_args(x, pscale, pshift, pshift_ns, pscale_ns, prelu, wfrag, bias, out, N, H, W);
  const int g = pp128_c256_grid_for(N, H, W, &a.tiles_x, &a.tiles_y);
  a.qs = qscale; a.qt = qshift; a.qrelu = (prelu >> 1) & 1;
  ++g_pp128_c256_launches;
  return pp128_launch<false, false, true>(a, g, stream);
}

// 1 if such a call may also hand its residual over at half resolution (be_conv2d_nhwc_frag_res).
int be_conv_pp128_takes_res_up2(int N, int H, int W) {
  return g_pp128_res_up2 && H % 2 == 0 && W % 2 == 0 && be_conv_pp128_takes(N, H, W);
}

}  // extern "C"
