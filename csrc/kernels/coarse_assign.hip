// Coarse quantizer of the IVF-PQ tier (search/ivfpq.py): per row of x the best and the second-best
// inner product against all centroids, by split-bf16 MFMA sums, with nothing but (i1, s1, s2) per row
// reaching HBM.  The caller certifies i1 as the exact argmax where s1 - s2 exceeds twice the error bound
// of the sums (coarse_certificate_eps) and recomputes the other rows.
//
//   be_coarse_split   centroids [nlist, D] fp32 -> bf16 image [nlist, 2D] = hi | lo along K, hi = bf16_rn(c),
//                     lo = bf16_rn(c - hi); and the largest centroid norm.  Once per assignment call.
//   be_coarse_top2    x [n, D] bf16 or fp32 against the image -> i1 (column of the largest score under
//                     (score descending, index ascending)), s1 (that score), s2 (the largest score among
//                     the other columns, -inf if there is none).  Score: one fp32 MFMA accumulator over
//                     x.c_hi + x.c_lo (bf16 rows, exact in bf16) or x_hi.c_hi + x_hi.c_lo + x_lo.c_hi
//                     (fp32 rows, split by the loader).
//
// be_coarse_top2, MI355X design:
//  * The centroids are the fragment-row operand of v_mfma_f32_16x16x32_bf16 and the x rows the
//    lane-column operand: the kernel computes cent . x^T tiles.  In the 16x16 accumulator layout lane l
//    then holds x row (l & 15) of a column fragment and centroids 4 (l >> 4) + e of a row fragment, so a
//    lane's whole selection state for that x row is (s1, i1, s2) in registers: 12 registers for the four
//    column fragments of a wave, updated with four VALU operations per accumulator element when a
//    centroid tile is complete.  No LDS lists, no LDS atomics, no re-selection.  (The other orientation
//    needs a state per accumulator row: 96 registers beside 128 accumulators.)
//  * 512 threads = 8 waves as 4 (x rows) x 2 (centroids), two waves per SIMD.  The workgroup owns 256 x
//    rows for the whole kernel and sweeps all 256-centroid tiles in ascending order; a wave owns
//    64 x rows x 128 centroids = 4 x 8 fragments (128 fp32 accumulators): 12 fragment reads of 1 KiB
//    feed 32 MFMAs.  A lane meets the columns of its row in ascending order, so within a lane a strict
//    "greater" keeps the smaller index among ties.
//  * K in 64-deep steps over the parts: the same x step meets c_hi and then c_lo (and, fp32 rows, x_lo
//    meets c_hi).  Two LDS buffers of (x 256 rows + centroids 256 rows) x 128 B = 64 KiB.  Step g + 1 --
//    which may be the first of the next centroid tile: the sweep is one flat loop -- is fetched from
//    global memory into registers before step g's MFMAs and stored to the other buffer after them: one
//    barrier per step (knn_topk.hip's loop at twice the block).  128-byte rows, 16-byte chunk c of row r
//    at c ^ ((r >> 1) & 7).  D % 32 == 0: the missing half of a last step is stored as zeros.
//  * After the sweep the four lanes that share an x row are merged by two xor shuffles and the two waves
//    that share it through 3 KiB of the (then idle) tile memory.  Every merge compares (score, index)
//    pairs exactly; s2 of a merge is the best of the loser's s1 and both sides' s2.
//  * LDS: 128 KiB, operand tiles only.  No global atomic, no host read, no grid barrier, no scratch.
//    Rows past n and columns past nlist are clamped when loaded; such a column enters the update as -inf
//    and such a row is not written.
#include "common.h"

#include <limits.h>

namespace {

constexpr int BX = 256, BC = 256, BK = 64, NT = 512;
constexpr int IMG = 256 * 128;       // one operand image of one step (bytes)
constexpr int LDS_COARSE = 4 * IMG;  // two buffers of (x, centroids)
static_assert(LDS_COARSE <= 160 * 1024, "LDS of one CU");
static_assert(3 * BX * 4 <= LDS_COARSE, "the wave merge reuses the tile memory");

#define CA_NEG_INF (-__builtin_huge_valf())

// (score a, index ia) strictly precedes (b, ib): larger score first, then the smaller index
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// (s1, i1, s2) <- the top two of its columns and the other side's (o1, oi, o2); the sides share no column
__device__ __forceinline__ void merge(float& s1, int& i1, float& s2, float o1, int oi, float o2) {
  const bool win = before(o1, oi, s1, i1);
  s2 = fmaxf(fmaxf(s2, o2), win ? s1 : o1);
  s1 = win ? o1 : s1;
  i1 = win ? oi : i1;
}

// eight fp32 values -> their bf16 hi parts, or (lo) the bf16 of what hi left over
__device__ __forceinline__ u32x4 split8(const float4& a, const float4& b, bool lo) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float p0 = v[2 * q], p1 = v[2 * q + 1];
    if (lo) {
      p0 -= bf2f(f2bf(p0));
      p1 -= bf2f(f2bf(p1));
    }
    w[q] = pack2bf(p0, p1);
  }
  return (u32x4){w[0], w[1], w[2], w[3]};
}

template <bool XF32>
__global__ __launch_bounds__(NT, 1) void coarse_top2_kernel(const void* __restrict__ Xv, const bf16_t* __restrict__ C2,
                                                            int n, int nlist, int D, int* __restrict__ out_i,
                                                            float* __restrict__ out_s1, float* __restrict__ out_s2) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const bf16_t* Xb = reinterpret_cast<const bf16_t*>(Xv);
  const float* Xf = reinterpret_cast<const float*>(Xv);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wx = wave >> 1, wc = wave & 1;
  const int x0 = blockIdx.x * BX;
  const int T = (nlist + BC - 1) / BC;
  const int nk = (D + BK - 1) / BK;
  const int ns = (XF32 ? 3 : 2) * nk;  // K steps of one centroid tile

  // staging: thread -> 16-byte chunk sc of rows srow + 64 u of both operand images
  const int srow = tid >> 3, sc = tid & 7;
  long long xoff[4];
  int dst[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int R = srow + 64 * u;
    int row = x0 + R;
    row = row < n ? row : n - 1;
    xoff[u] = (long long)row * D + sc * 8;
    dst[u] = R * 128 + ((sc ^ ((R >> 1) & 7)) << 4);
  }
  const int frow = lane & 15, fch = lane >> 4, fsw = (frow >> 1) & 7;

  // the fetch cursor runs one step ahead of the MFMAs: centroid tile ft, part fp, K step fk of the part
  int ft = 0, fp = 0, fk = 0;
  bool flo = false;  // the fetched x values are stored as their lo parts (fp32 rows, part 2)
  u32x4 rc[4], rx[4];
  float4 ra[4], rb[4];
  auto fetch = [&]() {
    const int k0 = fk * BK;
    const bool in = k0 + sc * 8 < D;  // D % 32 == 0: a chunk is whole or absent
    const int cpart = fp == 1 ? D : 0;
    flo = fp == 2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int col = ft * BC + srow + 64 * u;
      col = col < nlist ? col : nlist - 1;
      rc[u] = in ? *reinterpret_cast<const u32x4*>(C2 + (long long)col * (2 * D) + cpart + k0 + sc * 8)
                 : (u32x4){0u, 0u, 0u, 0u};
      if (XF32) {
        ra[u] = in ? *reinterpret_cast<const float4*>(Xf + xoff[u] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        rb[u] = in ? *reinterpret_cast<const float4*>(Xf + xoff[u] + k0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        rx[u] = in ? *reinterpret_cast<const u32x4*>(Xb + xoff[u] + k0) : (u32x4){0u, 0u, 0u, 0u};
      }
    }
    if (++fk == nk) {
      fk = 0;
      if (++fp == (XF32 ? 3 : 2)) {
        fp = 0;
        ++ft;
      }
    }
  };
  auto stash = [&](int buf) {
    unsigned char* a = smem + buf * 2 * IMG;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<u32x4*>(a + dst[u]) = XF32 ? split8(ra[u], rb[u], flo) : rx[u];
      *reinterpret_cast<u32x4*>(a + IMG + dst[u]) = rc[u];
    }
  };

  float s1[4], s2[4];
  int i1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s1[j] = CA_NEG_INF;
    s2[j] = CA_NEG_INF;
    i1[j] = INT_MAX;
  }
  f32x4 acc[8][4];  // [centroid fragment i][x fragment j]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  fetch();
  stash(0);
  __syncthreads();
  int buf = 0;
  for (int t = 0; t < T; ++t) {
    for (int s = 0; s < ns; ++s) {
      const bool more = t + 1 < T || s + 1 < ns;
      if (more) fetch();
      const unsigned char* sx = smem + buf * 2 * IMG + (wx * 64 + frow) * 128;
      const unsigned char* scn = smem + buf * 2 * IMG + IMG + (wc * 128 + frow) * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int ch = ((ks * 4 + fch) ^ fsw) << 4;
        bf16x8 fx[4], fc[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) fx[j] = *reinterpret_cast<const bf16x8*>(sx + j * 16 * 128 + ch);
#pragma unroll
        for (int i = 0; i < 8; ++i) fc[i] = *reinterpret_cast<const bf16x8*>(scn + i * 16 * 128 + ch);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[i], fx[j], acc[i][j], 0, 0, 0);
      }
      if (more) stash(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }

    // ---- selection: acc[i][j][e] is centroid c0 + i*16 + 4*fch + e against x row wx*64 + j*16 + frow; the
    // columns come in ascending order (tiles, then i, then e), so "greater" alone keeps the smaller index
    const int c0 = t * BC + wc * 128;
    const bool edge = c0 + 128 > nlist;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = c0 + i * 16 + 4 * fch + e;
        const bool valid = !edge || col < nlist;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = valid ? acc[i][j][e] : CA_NEG_INF;
          const bool up = v > s1[j];
          s2[j] = up ? s1[j] : fmaxf(s2[j], v);
          i1[j] = up ? col : i1[j];
          s1[j] = up ? v : s1[j];
        }
      }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // ---- the four lanes of an x row (fch = 0..3), then the two waves of it (wc = 0, 1)
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float o1 = __shfl_xor(s1[j], off, 64), o2 = __shfl_xor(s2[j], off, 64);
      const int oi = __shfl_xor(i1[j], off, 64);
      merge(s1[j], i1[j], s2[j], o1, oi, o2);
    }
  // the last step's barrier has passed: no wave reads the tiles any more
  float* m1 = reinterpret_cast<float*>(smem);
  float* m2 = m1 + BX;
  int* mi = reinterpret_cast<int*>(m2 + BX);
  if (wc == 1 && fch == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wx * 64 + j * 16 + frow;
      m1[r] = s1[j];
      m2[r] = s2[j];
      mi[r] = i1[j];
    }
  }
  __syncthreads();
  if (wc == 0 && fch == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wx * 64 + j * 16 + frow;
      merge(s1[j], i1[j], s2[j], m1[r], mi[r], m2[r]);
      const int row = x0 + r;
      if (row < n) {
        out_i[row] = i1[j];
        out_s1[row] = s1[j];
        out_s2[row] = s2[j];
      }
    }
  }
}

// One wave per centroid: hi | lo along K, and the wave's norm into the running maximum (norms are not
// negative, so their bit patterns order as unsigned integers).
__global__ __launch_bounds__(256) void coarse_split_kernel(const float* __restrict__ cent, int nlist, int D,
                                                           bf16_t* __restrict__ image, float* __restrict__ max_norm) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nlist) return;
  const float* c = cent + (long long)row * D;
  bf16_t* o = image + (long long)row * (2 * D);
  float ss = 0.f;
  for (int k = lane; k < D; k += 64) {
    const float v = c[k];
    const bf16_t h = f2bf(v);
    o[k] = h;
    o[D + k] = f2bf(v - bf2f(h));
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) atomicMax(reinterpret_cast<unsigned int*>(max_norm), __float_as_uint(sqrtf(ss)));
}

}  // namespace

extern "C" {

// cent [nlist, D] fp32 -> image [nlist, 2D] bf16 (hi | lo); *max_norm (zero on entry) <- the largest |c|.
int be_coarse_split(const float* cent, int nlist, int D, void* image, float* max_norm, hipStream_t s) {
  if (nlist < 1 || D < 1) return -1;
  hipLaunchKernelGGL(coarse_split_kernel, dim3((unsigned)((nlist + 3) / 4)), dim3(256), 0, s, cent, nlist, D,
                     (bf16_t*)image, max_norm);
  return BE_CHECK_LAUNCH();
}

// x [n, D] bf16 (x_bf16 != 0) or fp32, image [nlist, 2D] from be_coarse_split -> out_i / out_s1 / out_s2 [n].
int be_coarse_top2(const void* x, int x_bf16, const void* image, int n, int nlist, int D, int* out_i, float* out_s1,
                   float* out_s2, hipStream_t s) {
  if (D < 32 || D % 32 || D > 8192) return -2;
  if (n < 1 || nlist < 1) return -4;
  static bool attr[BE_MAX_DEV] = {};
  if (!attr[be_cur_dev()]) {
    if (hipFuncSetAttribute((const void*)coarse_top2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_COARSE) != hipSuccess ||
        hipFuncSetAttribute((const void*)coarse_top2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_COARSE) != hipSuccess)
      return -30;
    attr[be_cur_dev()] = true;
  }
  const dim3 grid((unsigned)((n + BX - 1) / BX));
  if (x_bf16)
    hipLaunchKernelGGL(coarse_top2_kernel<false>, grid, dim3(NT), LDS_COARSE, s, x, (const bf16_t*)image, n, nlist, D,
                       out_i, out_s1, out_s2);
  else
    hipLaunchKernelGGL(coarse_top2_kernel<true>, grid, dim3(NT), LDS_COARSE, s, x, (const bf16_t*)image, n, nlist, D,
                       out_i, out_s1, out_s2);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
