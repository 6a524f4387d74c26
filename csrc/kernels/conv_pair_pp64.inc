// Two-group ping-pong fused half-block for CM = 64 (the level-1 pairs at 112^2), included once by
// conv_pair.hip inside its anonymous namespace.  NOT a standalone header: no include guard on purpose.
//
// Same phase scheme as conv_pair_pp_kernel: the 8 waves are two groups of 4 that own alternate
// tiles of the workgroup's range and run ONE PHASE APART on the same workgroup barriers, so one
// group's VALU / LDS-store phase runs beside the other group's MFMA phase on every SIMD:
//     P1 commit (per 32-channel input chunk)   P2 stage A (per chunk, MFMA, s_setprio 1)
//     P3 epi A -> h                            P4 stage B (both h chunks, MFMA, s_setprio 1)
//     P5 next halo issue + output epilogue
//
// Geometry: a 16 x 16 output tile per group.  Per group ONE LDS region of 41.5 KB that holds, in
// turn, the 20 x 20 input image of one 32-channel chunk (64-byte pixels), the 18 x 18 h region
// (128-byte pixels) and the output staging (4 waves x 8 KB); 81 KB per workgroup.  Pixels are
// unpadded; the 16-byte chunk c of a pixel is XOR-swizzled so that every ds_read_b128 lane group
// ({kq, lrow 0-3 / 12-15} + {kq + 1, lrow 4-11}) of a 16-pixel row fragment hits 16 distinct slots:
//     input image  c ^ 2 * (((x >> 2) ^ y) & 1)     (the level-0 ping-pong's rule; IW = 20 = 0 mod 4)
//     h            c ^ 2 * ((x >> 1) & 3)           (c = 0..7: bit 0 separates kq from kq + 1)
// Both flip address bits above the pixel-internal offset only, so a fragment address is a per-lane
// base + a compile-time offset, XORed with a compile-time constant.
//
// Weights never pass through LDS: the host packs each conv once in MFMA-A-fragment order
// [chunk][ks][ct][lane][8 bf16] (ops/conv_pair.py, pack_frag) and a wave fetches a fragment with one
// coalesced 16-byte-per-lane global load straight into the operand registers, WD K-steps ahead of
// its use (the 74 KB per conv stay in L2).  The first WD steps of an MFMA phase are issued at the
// end of the VALU phase before it.  The small per-phase operands are issued a phase early as well
// (chunk 0's actA affine with its halo, actB's scale / shift ahead of the last stage A, the bias with
// the residual in P3): their L2 round trip at the top of a VALU phase cost 2-3 % per call.
//
// A wave owns 2 channel tiles (ct = 2 cp, 2 cp + 1; cp = gw & 1) x half of the pixel tiles
// (ph = gw >> 1), so every pixel fragment read feeds two MFMAs: stage A 11 pixel-tile slots
// (9 row tiles + the edge columns 16, 17 in 8-row tiles; slot 10 of ph = 1 is padding) = 88
// accumulator VGPRs, stage B 8 output rows = 64.  Stage A computes 324 h pixels per 256 outputs
// (the one-group 16 x 32 tile: 612 per 512): +5.9 % MFMA work for stage A, +2.9 % for the pair.
//
// Rounding points and the per-output accumulation order (A chunks in order, taps 0..8 within a
// chunk, then the B chunks likewise, 32-deep K-steps with lane kq holding channels 8 kq..8 kq + 7)
// are the one-group kernel's, so the output is bit-identical to it.
namespace pp64 {
constexpr int TS = 16;                    // output tile edge
constexpr int GW = 4, GT = GW * 64, NTP = 2 * GT;
constexpr int RW = TS + 2, RPIX = RW * RW;  // h region 18 x 18
constexpr int IW = TS + 4, IPIX = IW * IW;  // input image 20 x 20
constexpr int IN_B = IPIX * 64;             // 25600
constexpr int H_B = RPIX * 128;             // 41472
constexpr int OUTW_B = 8 * TS * 64;         // one wave's 8 rows x 16 px x 32 channels
constexpr int RB = H_B;                     // one group's region
constexpr int LDS = 2 * RB;
constexpr int APT = 11, BPT = 8;            // pixel-tile slots per wave
constexpr int HU = IPIX * 4, HUPT = (HU + GT - 1) / GT;  // 16-byte halo units per chunk, per thread
constexpr int WD = 3;                       // weight fragments are fetched WD K-steps ahead
constexpr int WSTEP = 4 * 64 * 8;           // elements per K-step of the fragment layout (4 ct)
// PROJ build (pool2 + c0 + c1 with the block's 1x1 projection inside): per group a second image,
// actP(pool(x)) at the 16 x 16 output pixels, 64-byte pixels, outside the region that h overlays.
// Written by the commit, read in P3 as stage-B style 16-pixel row fragments; the input image's
// swizzle c ^ 2 * (((x >> 2) ^ y) & 1) is conflict-free for it too (16 = 0 mod 4, as IW).
constexpr int P_B = TS * TS * 64;           // 16384
constexpr int LDS_PROJ = 2 * (RB + P_B);    // 115712; 82944 already means one workgroup per CU
static_assert(IN_B <= RB && GW * OUTW_B <= RB, "region overlays");
static_assert(LDS_PROJ <= 128 * 1024, "LDS budget of the ping-pong kernels");

__device__ __forceinline__ TileXY tile16(const PairArgs& a, int t) {
  const int tpi = a.tiles_x * a.tiles_y;
  TileXY r;
  r.n = t / tpi;
  const int q = t - r.n * tpi;
  r.ty0 = (q / a.tiles_x) * TS;
  r.tx0 = (q % a.tiles_x) * TS;
  return r;
}

__device__ __forceinline__ bool interior(const PairArgs& a, TileXY t) {
  return t.ty0 >= 2 && t.ty0 + TS + 2 <= a.H && t.tx0 >= 2 && t.tx0 + TS + 2 <= a.W;
}

// INMODE 2 (2x2 max pool on the way in) keeps the four raw source pixels: the max is taken in the
// commit, so the loads stay in flight across the barrier between P5 and P1
template <int INMODE>
struct Halo {
  u32x4 h[HUPT][INMODE == 2 ? 4 : 1];
  float4 aff[4];  // chunk 0: actA scale / shift of this thread's 8 channels ride along with the halo
};

// chunk ch of the tile's 20 x 20 input halo -> registers; clamped, unconditional loads (commit
// zeroes what lies outside the image and skips units past HU).  INMODE 0: full resolution,
// 1: nearest 2x upsampling of a half-resolution input, 2: 2x2 max pool of a double-resolution one.
template <int CIN, int INMODE>
__device__ __forceinline__ void issue_halo(const PairArgs& a, TileXY t, int ch, int gt, Halo<INMODE>& hr) {
  const int c = ch * 32 + (gt & 3) * 8;  // a thread's chunk is the same for every unit (GT % 4 == 0)
  if (ch == 0) {  // later chunks: read in the commit (no registers to spare across stage A)
    hr.aff[0] = *reinterpret_cast<const float4*>(a.sa + c);
    hr.aff[1] = *reinterpret_cast<const float4*>(a.sa + c + 4);
    const float* tr = a.ta + (size_t)t.n * a.ta_ns + c;
    hr.aff[2] = *reinterpret_cast<const float4*>(tr);
    hr.aff[3] = *reinterpret_cast<const float4*>(tr + 4);
  }
#pragma unroll
  for (int i = 0; i < HUPT; ++i) {
    const int pi = min(gt + i * GT, HU - 1) >> 2;
    const int y = pi / IW, x = pi - y * IW;
    const int gy = min(max(t.ty0 - 2 + y, 0), a.H - 1);
    const int gx = min(max(t.tx0 - 2 + x, 0), a.W - 1);
    if constexpr (INMODE == 0) {
      hr.h[i][0] = *reinterpret_cast<const u32x4*>(a.x + (((size_t)t.n * a.Hs + gy) * a.Ws + gx) * CIN + c);
    } else if constexpr (INMODE == 1) {
      hr.h[i][0] = *reinterpret_cast<const u32x4*>(a.x + (((size_t)t.n * a.Hs + (gy >> 1)) * a.Ws + (gx >> 1)) * CIN + c);
    } else {
      const bf16_t* base = a.x + (((size_t)t.n * a.Hs + 2 * gy) * a.Ws + 2 * gx) * CIN + c;
      hr.h[i][0] = *reinterpret_cast<const u32x4*>(base);
      hr.h[i][1] = *reinterpret_cast<const u32x4*>(base + CIN);
      hr.h[i][2] = *reinterpret_cast<const u32x4*>(base + (size_t)a.Ws * CIN);
      hr.h[i][3] = *reinterpret_cast<const u32x4*>(base + (size_t)a.Ws * CIN + CIN);
    }
  }
}

// P1: actA -> bf16 -> the swizzled input image (zero outside the image: conv padding applies after
// the activation).  Chunks 1.. read their affine here (L2-hot), not carried across the MFMA phase.
//
// PROJ: the same (pooled) values through actP (no ReLU) -> bf16 -> the projection's image `preg`, for
// the 16 x 16 pixels of the output tile; paff is actP's scale / shift of this thread's 8 channels.
struct PAff {
  float4 f[4];
};

__device__ __forceinline__ void issue_paff(const PairArgs& a, int gt, PAff& p) {
  const int c = (gt & 3) * 8;
  p.f[0] = *reinterpret_cast<const float4*>(a.sp + c);
  p.f[1] = *reinterpret_cast<const float4*>(a.sp + c + 4);
  p.f[2] = *reinterpret_cast<const float4*>(a.tp + c);
  p.f[3] = *reinterpret_cast<const float4*>(a.tp + c + 4);
}

// byte offset of 16-byte unit c of pixel (oy, ox) of the projection's 16 x 16 image
__device__ __forceinline__ int p_off(int oy, int ox, int c) {
  return (oy * TS + ox) * 64 + ((c ^ ((((ox >> 2) ^ oy) & 1) << 1)) << 4);
}

template <int INMODE, bool PROJ = false>
__device__ __forceinline__ void commit(const PairArgs& a, TileXY t, int ch, int gt, bool inner, const Halo<INMODE>& hr,
                                       unsigned char* rin, const PAff* paff = nullptr, unsigned char* preg = nullptr) {
  const int c = gt & 3, cc = ch * 32 + c * 8;
  float sc[8], sh[8];
  float ps[8], pt[8];
  if constexpr (PROJ) unpack_aff(paff->f, ps, pt);
  if (ch == 0) {
    unpack_aff(hr.aff, sc, sh);
  } else {
    float4 f[4];
    f[0] = *reinterpret_cast<const float4*>(a.sa + cc);
    f[1] = *reinterpret_cast<const float4*>(a.sa + cc + 4);
    const float* tr = a.ta + (size_t)t.n * a.ta_ns + cc;
    f[2] = *reinterpret_cast<const float4*>(tr);
    f[3] = *reinterpret_cast<const float4*>(tr + 4);
    unpack_aff(f, sc, sh);
  }
#pragma unroll
  for (int i = 0; i < HUPT; ++i) {
    const int u = gt + i * GT;
    if (u >= HU) continue;
    const int pi = u >> 2;
    const int y = pi / IW, x = pi - y * IW;
    const int gy = t.ty0 - 2 + y, gx = t.tx0 - 2 + x;
    u32x4 pk = (u32x4){0u, 0u, 0u, 0u}, pp = (u32x4){0u, 0u, 0u, 0u};
    if (inner || (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float lo = lo_bf(hr.h[i][0][j]), hi = hi_bf(hr.h[i][0][j]);
        if constexpr (INMODE == 2) {  // max of bf16 values is exact in bf16
          lo = fmaxf(fmaxf(lo, lo_bf(hr.h[i][1][j])), fmaxf(lo_bf(hr.h[i][2][j]), lo_bf(hr.h[i][3][j])));
          hi = fmaxf(fmaxf(hi, hi_bf(hr.h[i][1][j])), fmaxf(hi_bf(hr.h[i][2][j]), hi_bf(hr.h[i][3][j])));
        }
        pk[j] = relu_bf16x2(pack2bf(fmaf(lo, sc[2 * j], sh[2 * j]), fmaf(hi, sc[2 * j + 1], sh[2 * j + 1])));
        if constexpr (PROJ) pp[j] = pack2bf(fmaf(lo, ps[2 * j], pt[2 * j]), fmaf(hi, ps[2 * j + 1], pt[2 * j + 1]));
      }
    }
    *reinterpret_cast<u32x4*>(rin + pi * 64 + ((c ^ ((((x >> 2) ^ y) & 1) << 1)) << 4)) = pk;
    if constexpr (PROJ) {
      if (y >= 2 && y < TS + 2 && x >= 2 && x < TS + 2) *reinterpret_cast<u32x4*>(preg + p_off(y - 2, x - 2, c)) = pp;
    }
  }
}

// Stage-A slot j of pixel half ph -> this lane's h-region pixel (ry, rx).  Slots 0..8: region rows
// 9 ph + j, columns 0..15; slot 9: columns 16, 17 of rows 8 ph .. 8 ph + 7; slot 10: columns 16, 17 of
// rows 16, 17 (ph = 0, lanes 0..3).  false: padding (reads pixel (0, 0), never stored).
__device__ __forceinline__ bool a_pix(int ph, int j, int lrow, int& ry, int& rx) {
  if (j < 9) {
    ry = 9 * ph + j;
    rx = lrow;
    return true;
  }
  if (j == 9) {
    ry = 8 * ph + (lrow >> 1);
    rx = 16 + (lrow & 1);
    return true;
  }
  ry = 16 + (lrow >> 1);
  rx = 16 + (lrow & 1);
  const bool ok = ph == 0 && ry < RW;
  if (!ok) { ry = 0; rx = 0; }
  return ok;
}

// The first WD K-steps' weight fragments of an MFMA phase, issued in the phase before it.
struct WPre {
  bf16x8 w[WD][2];
};

// wf: the conv's fragment-order weights at this phase's K-step 0; lane: 0..63, cp: channel-tile pair
__device__ __forceinline__ const bf16_t* w_lane(const bf16_t* wf, int cp, int lane) {
  return wf + cp * 2 * 512 + lane * 8;
}

__device__ __forceinline__ void issue_w(const bf16_t* wl, WPre& p) {
#pragma unroll
  for (int d = 0; d < WD; ++d)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) p.w[d][ct] = *reinterpret_cast<const bf16x8*>(wl + d * WSTEP + ct * 512);
}

// NS K-steps over NPT pixel tiles x 2 channel tiles.  One pixel-fragment set with rolling reload
// (each fragment of step s + 1 is read right after its last MFMA of step s); weight fragments come
// from global memory WD steps ahead.  rd(s, j): LDS byte offset of pixel tile j's fragment at step s.
template <int NS, int NPT, typename RD>
__device__ __forceinline__ void mma_run(f32x4 (&acc)[2][NPT], const unsigned char* reg, const bf16_t* wl, const WPre& pre,
                                        RD rd) {
  bf16x8 w[NS][2];  // fully unrolled: WD + 1 steps are live at a time
#pragma unroll
  for (int d = 0; d < WD; ++d) {
    w[d][0] = pre.w[d][0];
    w[d][1] = pre.w[d][1];
  }
  bf16x8 bf[NPT];
#pragma unroll
  for (int j = 0; j < NPT; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(reg + rd(0, j));
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s + WD < NS) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        w[s + WD][ct] = *reinterpret_cast<const bf16x8*>(wl + (s + WD) * WSTEP + ct * 512);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
        acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[s][ct], bf[j], acc[ct][j], 0, 0, 0);
      if (s + 1 < NS) bf[j] = *reinterpret_cast<const bf16x8*>(reg + rd(s + 1, j));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// P2: stage A over one input chunk
__device__ __forceinline__ void mma_a(f32x4 (&acc)[2][APT], const unsigned char* rin, const bf16_t* wl, const WPre& pre,
                                      int ph, int lrow, int kq) {
  int A0[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx)
    A0[dx] = ((9 * ph * IW + lrow + dx) * 64 + kq * 16) ^ (((((lrow + dx) >> 2) ^ ph) & 1) << 5);
  int L[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    int ry, rx;
    a_pix(ph, 9 + e, lrow, ry, rx);
    L[e] = ((ry * IW + rx) * 64 + kq * 16) ^ ((ry & 1) << 5);
  }
  mma_run<9, APT>(acc, rin, wl, pre, [&](int ks, int j) {
    const int dy = ks / 3, dx = ks % 3;
    if (j < 9) return (A0[dx] + (j + dy) * IW * 64) ^ (((j + dy) & 1) << 5);
    return (L[j - 9] + (dy * IW + dx) * 64) ^ ((dy & 1) << 5);
  });
}

// P3: actB (+ skip operand x2 of stage A's output) -> h (bf16) over the input image, zero outside
// the image
template <bool X2>
__device__ __forceinline__ void epi_a(const PairArgs& a, TileXY t, bool inner, const f32x4 (&acc)[2][APT],
                                      unsigned char* rh, const float4 (&sbp)[2], const float4 (&tbp)[2], int cp, int ph,
                                      int lrow, int kq) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int cc = (2 * cp + ct) * 16 + kq * 4;
    const float4 s = sbp[ct], sh = tbp[ct];
    const int c8 = (2 * cp + ct) * 2 + (kq >> 1);
    u32x2 xv[X2 ? APT : 1];
    if constexpr (X2) {  // clamped, unconditional loads, all in flight before the first use
#pragma unroll
      for (int j = 0; j < APT; ++j) {
        int ry, rx;
        a_pix(ph, j, lrow, ry, rx);
        const int gy = min(max(t.ty0 - 1 + ry, 0), a.H - 1), gx = min(max(t.tx0 - 1 + rx, 0), a.W - 1);
        xv[j] = *reinterpret_cast<const u32x2*>(a.x2 + (((size_t)t.n * a.H + gy) * a.W + gx) * 64 + cc);
      }
    }
#pragma unroll
    for (int j = 0; j < APT; ++j) {
      int ry, rx;
      if (!a_pix(ph, j, lrow, ry, rx)) continue;
      const int off = (ry * RW + rx) * 128 + ((c8 ^ (((rx >> 1) & 3) << 1)) << 4) + (kq & 1) * 8;
      const int gy = t.ty0 - 1 + ry, gx = t.tx0 - 1 + rx;
      u32x2 st = (u32x2){0u, 0u};
      if (inner || (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)) {
        float v0 = acc[ct][j][0], v1 = acc[ct][j][1], v2 = acc[ct][j][2], v3 = acc[ct][j][3];
        if constexpr (X2) {
          v0 += lo_bf(xv[j][0]); v1 += hi_bf(xv[j][0]); v2 += lo_bf(xv[j][1]); v3 += hi_bf(xv[j][1]);
        }
        st[0] = relu_bf16x2(pack2bf(fmaf(v0, s.x, sh.x), fmaf(v1, s.y, sh.y)));
        st[1] = relu_bf16x2(pack2bf(fmaf(v2, s.z, sh.z), fmaf(v3, s.w, sh.w)));
      }
      *reinterpret_cast<u32x2*>(rh + off) = st;
    }
  }
}

// P4: stage B over both 32-channel chunks of h; wave (cp, ph) owns output rows 8 ph .. 8 ph + 7
__device__ __forceinline__ void mma_b(f32x4 (&acc)[2][BPT], const unsigned char* rh, const bf16_t* wl, const WPre& pre,
                                      int ph, int lrow, int kq) {
  int B0[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx)
    B0[dx] = (8 * ph * RW + lrow + dx) * 128 + ((kq ^ ((((lrow + dx) >> 1) & 3) << 1)) << 4);
  mma_run<18, BPT>(acc, rh, wl, pre, [&](int s, int pt) {
    const int cb = s / 9, ks = s % 9, dy = ks / 3, dx = ks % 3;
    return (B0[dx] + (pt + dy) * RW * 128) ^ (cb << 6);
  });
}

struct Res {
  u32x2 rv[BPT][2];
  float4 bias[2];
};

// RES 1: residual at output resolution, 2: nearest 2x upsampling of a half-resolution one
template <int RES>
__device__ __forceinline__ void issue_res(const PairArgs& a, TileXY t, int cp, int ph, int lrow, int kq, Res& r) {
#pragma unroll
  for (int pt = 0; pt < BPT; ++pt) {
    const int py = min(t.ty0 + 8 * ph + pt, a.H - 1), px = min(t.tx0 + lrow, a.W - 1);
    const bf16_t* rp = RES == 1 ? a.res + (((size_t)t.n * a.H + py) * a.W + px) * 64 + cp * 32 + kq * 4
                                : a.res + (((size_t)t.n * (a.H >> 1) + (py >> 1)) * (a.W >> 1) + (px >> 1)) * 64 + cp * 32 + kq * 4;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) r.rv[pt][ct] = *reinterpret_cast<const u32x2*>(rp + ct * 16);
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) r.bias[ct] = *reinterpret_cast<const float4*>(a.bias + (2 * cp + ct) * 16 + kq * 4);
}

// PROJ: the residual is the block's 1x1 projection of the commit's actP image, computed where the
// other builds fetch theirs: per (ct, output row) ONE 32-deep MFMA from a zero accumulator (lane kq:
// channels 8 kq .. 8 kq + 7), then (acc + biasP) + 0.0f rounded to bf16 -- conv2d_nhwc_kernel's 1x1
// at CK = 32 with no residual, operation for operation (the + 0.0f turns a -0.0 sum into +0.0 as its
// zero residual does), so the packed result is the tensor that kernel would have written and epi_b
// adds it as any residual.  wp / bp: the wave's two weight fragments and biases, fetched a phase early.
struct ProjW {
  bf16x8 w[2];
  float4 b[2];
};

__device__ __forceinline__ void issue_projw(const PairArgs& a, int cp, int lane, ProjW& p) {
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    p.w[ct] = *reinterpret_cast<const bf16x8*>(a.wpf + (2 * cp + ct) * 512 + lane * 8);
    p.b[ct] = *reinterpret_cast<const float4*>(a.biasp + (2 * cp + ct) * 16 + (lane >> 4) * 4);
  }
}

__device__ __forceinline__ void proj_res(const PairArgs& a, const unsigned char* preg, const ProjW& p, int cp, int ph,
                                         int lrow, int kq, Res& r) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // p_off(8 ph + pt, lrow, kq): 8 ph is even, so the row's parity is pt's
  const int P0 = ((8 * ph * TS + lrow) * 64 + kq * 16) ^ (((lrow >> 2) & 1) << 5);
#pragma unroll
  for (int pt = 0; pt < BPT; ++pt) {
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(preg + ((P0 + pt * TS * 64) ^ ((pt & 1) << 5)));
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const f32x4 v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p.w[ct], b, zero, 0, 0, 0);
      r.rv[pt][ct][0] = pack2bf(v[0] + p.b[ct].x + 0.0f, v[1] + p.b[ct].y + 0.0f);
      r.rv[pt][ct][1] = pack2bf(v[2] + p.b[ct].z + 0.0f, v[3] + p.b[ct].w + 0.0f);
    }
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) r.bias[ct] = *reinterpret_cast<const float4*>(a.bias + (2 * cp + ct) * 16 + kq * 4);
}

// P5: bias + residual -> wave-private staging (64-byte half pixels, swizzled like the level-0 h)
// -> 16-byte buffer stores; pixels outside the image and tiles that are not this group's get an
// out-of-range offset, which the descriptor's range check drops
__device__ __forceinline__ void epi_b(const PairArgs& a, TileXY t, const f32x4 (&acc)[2][BPT], const Res& r,
                                      unsigned char* ws, int cp, int ph, int lrow, int kq, bool act) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      a.out + (size_t)t.n * a.H * a.W * 64, (short)0, a.H * a.W * 128, 0x00020000);
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const float4 bias = r.bias[ct];
    const int ow = lrow * 64 + ((((2 * ct) | (kq >> 1)) ^ ((lrow >> 1) & 3)) << 4) + (kq & 1) * 8;
#pragma unroll
    for (int pt = 0; pt < BPT; ++pt) {
      u32x2 rv = r.rv[pt][ct];
      asm volatile("" : "+v"(rv));  // unpacked here, not next to its load in P3
      u32x2 st;
      st[0] = pack2bf(acc[ct][pt][0] + bias.x + lo_bf(rv[0]), acc[ct][pt][1] + bias.y + hi_bf(rv[0]));
      st[1] = pack2bf(acc[ct][pt][2] + bias.z + lo_bf(rv[1]), acc[ct][pt][3] + bias.w + hi_bf(rv[1]));
      *reinterpret_cast<u32x2*>(ws + ow + pt * 1024) = st;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int lane = lrow + 16 * kq;
  const int rd = (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 3) & 3)) << 4);
  const int px = t.tx0 + (lane >> 2);
#pragma unroll
  for (int it = 0; it < BPT; ++it) {
    const int py = t.ty0 + 8 * ph + it;
    const u32x4 v = *reinterpret_cast<const u32x4*>(ws + rd + it * 1024);
    const int off = (act && py < a.H && px < a.W) ? ((py * a.W + px) * 64 + cp * 32 + (lane & 3) * 8) * 2 : 0x7ffffff0;
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 0);
  }
}

// NCA input chunks of 32 channels (Cin = 32 NCA), INMODE / X2 / RES as above.  The level-1
// half-blocks: (2, 0, false, 1) c2 + c3 + x1, (1, 2, false, 1) pool2 + c0 + c1 + proj,
// (4, 1, true, 2) up2 + c0 + c1 + skip + up2(proj).  PROJ: (1, 2, false, 0) with the projection computed
// inside (commit / proj_res) instead of read as a residual.
template <int NCA, int INMODE, bool X2, int RES, bool STAMP = false, bool PROJ = false>
__global__ __launch_bounds__(NTP, 2) void conv_pair_pp64_kernel(PairArgs a) {
  static_assert(PROJ ? (NCA == 1 && RES == 0 && !X2) : RES != 0, "the residual is read or projected");
  constexpr int CIN = 32 * NCA;
  // STAMP (diagnostics, tools/pp_phase_profile.py): as conv_pair_pp_kernel, [grid][2 groups][16];
  // slots: commit / stage A of chunk 0, of the later chunks together, epi A, stage B, epi B
  unsigned long long ph_work[7] = {0, 0, 0, 0, 0, 0, 0}, ph_wait[7] = {0, 0, 0, 0, 0, 0, 0};
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
  const int total = a.N * a.tiles_x * a.tiles_y;
  const int t0 = (int)(((long long)blockIdx.x * total) / gridDim.x);
  const int t1 = (int)(((long long)(blockIdx.x + 1) * total) / gridDim.x);
  if (t0 >= t1) return;  // workgroup-uniform
  const int grp = __builtin_amdgcn_readfirstlane(tid0 / GT);  // waves w and w + 4 share a SIMD
  const int gt0 = tid0 & (GT - 1);
  unsigned char* reg = smem + grp * RB;
  unsigned char* preg = smem + 2 * RB + grp * P_B;  // PROJ builds only
  Halo<INMODE> halo;
  PAff paff;  // PROJ: rides with chunk 0's halo like its actA affine
  issue_halo<CIN, INMODE>(a, tile16(a, min(t0 + grp, t1 - 1)), 0, gt0, halo);
  if constexpr (PROJ) issue_paff(a, gt0, paff);
  if (grp == 1) __builtin_amdgcn_s_barrier();  // the stagger: group 1 runs one phase behind
  const int iters = (t1 - t0 + 1) >> 1;
  for (int k = 0; k < iters; ++k) {
    int gt = gt0;
    asm volatile("" : "+v"(gt));  // per-iteration opaque copy: no addresses hoisted out of the tile loop
    const int gw = __builtin_amdgcn_readfirstlane(gt >> 6), lane = gt & 63, lrow = lane & 15, kq = lane >> 4;
    const int cp = gw & 1, ph = gw >> 1;
    const int t = t0 + 2 * k + grp;
    // a group without a tile in the last iteration (odd range) recomputes the range's last tile and
    // stores nothing
    const bool act = t < t1;
    const TileXY cur = tile16(a, act ? t : t1 - 1);
    const bool inner = interior(a, cur);
    const bf16_t* wla = w_lane(a.waf, cp, lane);
    const bf16_t* wlb = w_lane(a.wbf, cp, lane);
    f32x4 acc_a[2][APT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < APT; ++j) acc_a[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    WPre wpre;
    float4 sbp[2], tbp[2];  // actB scale / shift, issued ahead of the last stage A
#pragma unroll
    for (int c = 0; c < NCA; ++c) {
      // P1: input chunk c -> activated image; then the first weight fragments of its stage A
      int gc = gt0;
      asm volatile("" : "+v"(gc));
      if constexpr (PROJ)
        commit<INMODE, true>(a, cur, c, gc, inner, halo, reg, &paff, preg);
      else
        commit<INMODE>(a, cur, c, gc, inner, halo, reg);
      issue_w(wla + c * 9 * WSTEP, wpre);
      pre(slot(c));
      __syncthreads();
      post(slot(c));
      // P2: stage A over chunk c, the next chunk's halo in flight.  (Issued at the end of the commit
      // instead, as conv_pp128.hip does, it gained nothing here: 64 -> 64 unchanged, 128 -> 64 up2
      // 1-4 % slower per call; profiles/proj/README.md.)
      if (c + 1 < NCA) issue_halo<CIN, INMODE>(a, cur, c + 1, gt, halo);
      if (c == NCA - 1) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          sbp[ct] = *reinterpret_cast<const float4*>(a.sb + (2 * cp + ct) * 16 + kq * 4);
          tbp[ct] = *reinterpret_cast<const float4*>(a.tb + (size_t)cur.n * a.tb_ns + (2 * cp + ct) * 16 + kq * 4);
        }
      }
      __builtin_amdgcn_s_setprio(1);
      mma_a(acc_a, reg, wla + c * 9 * WSTEP, wpre, ph, lrow, kq);
      __builtin_amdgcn_s_setprio(0);
      pre(slot(c) + 1);
      __syncthreads();
      post(slot(c) + 1);
    }
    // P3: epilogue A -> h; this tile's residual and stage B's first weight fragments issued behind it
    int g3 = gt0;
    asm volatile("" : "+v"(g3));
    ProjW pw;
    if constexpr (PROJ) issue_projw(a, cp, g3 & 63, pw);  // back from L2 by the end of epi_a
    epi_a<X2>(a, cur, inner, acc_a, reg, sbp, tbp, cp, ph, g3 & 15, (g3 & 63) >> 4);
    Res res;
    if constexpr (PROJ) {
      issue_w(wlb, wpre);
      proj_res(a, preg, pw, cp, ph, g3 & 15, (g3 & 63) >> 4, res);
    } else {
      issue_res<RES>(a, cur, cp, ph, g3 & 15, (g3 & 63) >> 4, res);
      issue_w(wlb, wpre);
    }
    pre(4);
    __syncthreads();
    post(4);
    // P4: stage B
    int g4 = gt0;
    asm volatile("" : "+v"(g4));
    f32x4 acc_b[2][BPT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < BPT; ++j) acc_b[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
    mma_b(acc_b, reg, wlb, wpre, ph, g4 & 15, (g4 & 63) >> 4);
    __builtin_amdgcn_s_setprio(0);
    pre(5);
    __syncthreads();
    post(5);
    // P5: the group's next halo, then the output epilogue (its staging overlays h: every wave of the
    // group is past stage B)
    int g5 = gt0;
    asm volatile("" : "+v"(g5));
    // (the pooled input's four raw loads per unit are issued after it: its registers are free then)
    if constexpr (INMODE != 2) issue_halo<CIN, INMODE>(a, tile16(a, min(t + 2, t1 - 1)), 0, g5, halo);
    __builtin_amdgcn_sched_barrier(0);
    epi_b(a, cur, acc_b, res, reg + gw * OUTW_B, cp, ph, g5 & 15, (g5 & 63) >> 4, act);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (INMODE == 2) issue_halo<CIN, INMODE>(a, tile16(a, min(t + 2, t1 - 1)), 0, g5, halo);
    if constexpr (PROJ) issue_paff(a, g5, paff);
    pre(6);
    __syncthreads();
    post(6);
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();  // balance the stagger
  if constexpr (STAMP) {
    if ((tid0 & (GT - 1)) < 16) {  // wave 0 of each group: lane k stores slot k
      const int k = tid0 & 15;
      unsigned long long v = 0;
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        if (k == i) v = ph_work[i];
        if (k == 8 + i) v = ph_wait[i];
      }
      if (k == 15) v = (unsigned long long)iters;
      a.stamps[((size_t)blockIdx.x * 2 + grp) * 16 + k] = v;
    }
  }
}
}  // namespace pp64
