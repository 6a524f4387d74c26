// Build side of the IVF-PQ tier (search/ivfpq.py): residual product-quantiser encoding and one Lloyd
// iteration of the PQ codebooks, with the nearest codeword chosen inside an fp32 MFMA kernel, so that no
// distance is ever stored to HBM.
//
//   be_pq_encode       x [n, D] (fp32 or bf16), coarse centroids [nlist, D], assign [n], codebooks [m, 256, ds]
//                      -> codes [n, m] uint8:  r = fp32(x) - c[assign] (one fp32 rounding),
//                      code = argmin_k (|cb_k|^2 - 2 r.cb_k), a tie to the smaller k
//   be_pq_kmeans_step  residuals [S, D] fp32, codebooks -> new codebooks: the same assignment, then per
//                      (sub-space, codeword) the sum and count of its rows, sum / count; a codeword without
//                      rows keeps its value.  Two kernels: per-slab partials, then a reduce in slab order.
//
// Both are one kernel template (pq_assign_kernel), MI355X design:
//  * A workgroup is 1024 threads = 16 waves and owns a group of 16 consecutive sub-spaces (16 ds columns of
//    x: one 256-byte slice of a bf16 row at ds = 8) and a contiguous range of 128-row tiles, which it walks in
//    ascending order.  Wave w owns sub-space w of the group for the whole kernel, so its codebook is loaded ONCE
//    into registers as the MFMA's first operand, scaled by -2 (exact): 16 VGPRs at ds = 4, 32 at ds = 8.  A
//    4-wave workgroup would reload a codebook per (tile, sub-space); 16 waves make that unnecessary and still
//    fit the register file (4 waves per SIMD, 128 registers each).
//  * v_mfma_f32_16x16x4_f32: first operand = 16 codewords x 4 dims, second = 4 dims x 16 data rows, and the
//    accumulator starts as the codewords' squared norms, so D = |cb_k|^2 - 2 r.cb_k after one (ds = 4) or two
//    (ds = 8) instructions.  The output's codeword index is spread over registers and lane quarters: lane l
//    holds data row l % 16 against codewords 16 t + 4 (l / 16) + e, e = 0..3.  Over the 16 codeword tiles t a
//    lane runs a strict-less minimum over its 64 codewords in ascending k, and two cross-lane steps (xor 16,
//    xor 32) comparing (score, k) finish the argmin with the tie rule intact.  At ds = 8 lane quarter g feeds
//    dims 2 g and 2 g + 1 to the two K steps (the order of K is free as both operands agree), so a row
//    fragment is one 8-byte LDS read.
//  * LDS: the tile's residuals, formed once by all threads, as fp32 rows of 16 ds + 4 floats (the + 4 spreads
//    a fragment read over all 64 banks); the group's 16 x 256 norms (accumulated in double, rounded once);
//    the tile's codes [128][16].  67.6 + 16 + 2 KiB at ds = 8.  The next tile's x, assign and centroid slices
//    are fetched into registers before the current tile's MFMAs and stored after them.
//  * The codes leave as one 16-byte store per row (the group's 16 bytes of the [n, m] row).
//  * k-means: after a tile's codes are in LDS, wave w walks the tile's rows in order; code and residual slice
//    are wave-uniform LDS reads, lane k % 64 adds the slice into accumulator set k / 64 of its registers
//    (4 x (ds + 1)).  No atomics anywhere, so the sums have one fixed order: rows ascending inside a slab,
//    slabs ascending in pq_kmeans_reduce_kernel.  Partials [slabs, m, 256, ds + 1] (the count as an int).
//  * The fp32 MFMA, not the input stream, sets the pace: 512 n D flop is 23 TFLOP at 58 M x 768, 0.15 s at
//    the fp32 matrix peak, against 15 ms to read 89 GB of bf16 rows.  The per-lane selection (3 VALU operations
//    per score) runs beside other waves' MFMAs.
//  * Rows past n are clamped when loaded and never written; assign is clamped to the centroid table.
#include "common.h"

namespace {

constexpr int PQ_ROWS = 128, PQ_NT = 1024, PQ_GROUP = 16;

template <int DS>
struct PQ {
  static constexpr int W = PQ_GROUP * DS;           // floats of a row that the group owns
  static constexpr int STRIDE = W + 4;              // LDS row stride (floats): STRIDE % 64 == 4
  static constexpr int CPR = W / 4;                 // 4-float chunks per row
  static constexpr int NCH = PQ_ROWS * CPR / PQ_NT; // chunks per thread
  static constexpr int OFF_NORM = PQ_ROWS * STRIDE * 4;
  static constexpr int OFF_CODE = OFF_NORM + PQ_GROUP * 256 * 4;
  static constexpr int LDS = OFF_CODE + PQ_ROWS * PQ_GROUP;
};

enum { PQ_F32 = 0, PQ_BF16 = 1, PQ_KMEANS = 2 };

template <int DS, int MODE>
__global__ __launch_bounds__(PQ_NT, 1) void pq_assign_kernel(const void* __restrict__ xv, const float* __restrict__ cent,
                                                             const int* __restrict__ assign,
                                                             const float* __restrict__ cb, int n, int D, int m,
                                                             int nlist, int slabs, unsigned char* __restrict__ codes,
                                                             float* __restrict__ part) {
  using P = PQ<DS>;
  static_assert(P::LDS <= 160 * 1024, "LDS of one CU");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* res = reinterpret_cast<float*>(smem);
  float* norms = reinterpret_cast<float*>(smem + P::OFF_NORM);
  unsigned char* tcode = smem + P::OFF_CODE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = blockIdx.x, slab = blockIdx.y;
  const int T = (n + PQ_ROWS - 1) / PQ_ROWS;
  const int t_lo = (int)((long long)slab * T / slabs), t_hi = (int)((long long)(slab + 1) * T / slabs);
  const int col0 = grp * P::W;          // first column of the group
  const int j = grp * PQ_GROUP + wave;  // this wave's sub-space
  const int fr = lane & 15, fq = lane >> 4;

  // ---- this wave's codebook as the MFMA's first operand (x -2), and its norms
  const float* cbj = cb + (long long)j * 256 * DS;
  float a0[16], a1[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const float* p = cbj + (16 * t + fr) * DS;
    if (DS == 4) {
      a0[t] = -2.f * p[fq];
      a1[t] = 0.f;
    } else {
      const float2 v = *reinterpret_cast<const float2*>(p + 2 * fq);
      a0[t] = -2.f * v.x;
      a1[t] = -2.f * v.y;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float* p = cbj + (lane + 64 * q) * DS;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < DS; ++i) s += (double)p[i] * (double)p[i];
    norms[wave * 256 + lane + 64 * q] = (float)s;
  }

  // k-means: lane owns codewords lane + 64 q of sub-space j
  float sum[4][DS];
  int cnt[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cnt[q] = 0;
#pragma unroll
    for (int i = 0; i < DS; ++i) sum[q][i] = 0.f;
  }

  // ---- staging: thread -> chunk (row, c4) of the tile, NCH of them
  f32x4 rx[P::NCH], rc[P::NCH];
  auto fetch = [&](int tile) {
#pragma unroll
    for (int u = 0; u < P::NCH; ++u) {
      const int q = tid + PQ_NT * u;
      int row = tile * PQ_ROWS + q / P::CPR;
      row = row < n ? row : n - 1;
      const long long off = (long long)row * D + col0 + (q % P::CPR) * 4;
      if (MODE == PQ_BF16) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(xv) + off);
        rx[u] = (f32x4){lo_bf(w.x), hi_bf(w.x), lo_bf(w.y), hi_bf(w.y)};
      } else {
        rx[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(xv) + off);
      }
      if (MODE != PQ_KMEANS) {
        int a = assign[row];
        a = a < 0 ? 0 : (a < nlist ? a : nlist - 1);
        rc[u] = *reinterpret_cast<const f32x4*>(cent + (long long)a * D + col0 + (q % P::CPR) * 4);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < P::NCH; ++u) {
      const int q = tid + PQ_NT * u;
      f32x4 r = rx[u];
      if (MODE != PQ_KMEANS) r = rx[u] - rc[u];
      *reinterpret_cast<f32x4*>(res + (q / P::CPR) * P::STRIDE + (q % P::CPR) * 4) = r;
    }
  };

  // k-means keeps its registers for the sums and fetches a tile when it needs it
  if (MODE != PQ_KMEANS && t_lo < t_hi) fetch(t_lo);
  for (int tile = t_lo; tile < t_hi; ++tile) {
    if (MODE == PQ_KMEANS) fetch(tile);
    stash();
    __syncthreads();  // residuals (and, the first time, the norms) are in LDS
    if (MODE != PQ_KMEANS && tile + 1 < t_hi) fetch(tile + 1);

    const float* nw = norms + wave * 256 + 4 * fq;
#pragma unroll 1
    for (int f = 0; f < PQ_ROWS / 16; ++f) {
      const float* rp = res + (16 * f + fr) * P::STRIDE + wave * DS;
      float b0, b1 = 0.f;
      if (DS == 4) {
        b0 = rp[fq];
      } else {
        const float2 v = *reinterpret_cast<const float2*>(rp + 2 * fq);
        b0 = v.x;
        b1 = v.y;
      }
      float best = __builtin_huge_valf();
      int bk = 0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        f32x4 acc = *reinterpret_cast<const f32x4*>(nw + 16 * t);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[t], b0, acc, 0, 0, 0);
        if (DS == 8) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t], b1, acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool lt = acc[e] < best;  // ascending k and strict: the first minimum stays
          best = lt ? acc[e] : best;
          bk = lt ? 16 * t + e : bk;
        }
      }
      bk += 4 * fq;
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int ok = __shfl_xor(bk, off, 64);
        const bool take = ov < best || (ov == best && ok < bk);
        best = take ? ov : best;
        bk = take ? ok : bk;
      }
      if (lane < 16) tcode[(16 * f + lane) * PQ_GROUP + wave] = (unsigned char)bk;
    }
    __syncthreads();  // the tile's codes are in LDS; nobody reads the residuals for the MFMAs any more

    if (MODE == PQ_KMEANS) {
      const int rows = min(PQ_ROWS, n - tile * PQ_ROWS);
      for (int r = 0; r < rows; ++r) {
        const int c = __builtin_amdgcn_readfirstlane((int)tcode[r * PQ_GROUP + wave]);
        const float* rp = res + r * P::STRIDE + wave * DS;
        float v[DS];
#pragma unroll
        for (int i = 0; i < DS; i += 4) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(rp + i);
          v[i] = w[0]; v[i + 1] = w[1]; v[i + 2] = w[2]; v[i + 3] = w[3];
        }
        const bool mine = (c & 63) == lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if ((c >> 6) == q) {  // wave-uniform
            cnt[q] += mine ? 1 : 0;
#pragma unroll
            for (int i = 0; i < DS; ++i) sum[q][i] += mine ? v[i] : 0.f;
          }
        }
      }
      __syncthreads();  // the next stash overwrites the residuals
    } else if (tid < PQ_ROWS) {
      const int row = tile * PQ_ROWS + tid;
      if (row < n)
        *reinterpret_cast<u32x4*>(codes + (long long)row * m + grp * PQ_GROUP) =
            *reinterpret_cast<const u32x4*>(tcode + tid * PQ_GROUP);
    }
  }

  if (MODE == PQ_KMEANS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* p = part + (((long long)slab * m + j) * 256 + lane + 64 * q) * (DS + 1);
#pragma unroll
      for (int i = 0; i < DS; ++i) p[i] = sum[q][i];
      p[DS] = __int_as_float(cnt[q]);
    }
  }
}

// One thread per (sub-space, codeword): the slabs' partial sums in ascending slab order, then sum / count.
template <int DS>
__global__ __launch_bounds__(256) void pq_kmeans_reduce_kernel(const float* __restrict__ part,
                                                               const float* __restrict__ cb_old, int slabs, int m,
                                                               float* __restrict__ cb_new) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m * 256) return;
  float s[DS];
#pragma unroll
  for (int i = 0; i < DS; ++i) s[i] = 0.f;
  int cnt = 0;
  for (int sl = 0; sl < slabs; ++sl) {
    const float* p = part + ((long long)sl * m * 256 + e) * (DS + 1);
#pragma unroll
    for (int i = 0; i < DS; ++i) s[i] += p[i];
    cnt += __float_as_int(p[DS]);
  }
  const float c = (float)cnt;
#pragma unroll
  for (int i = 0; i < DS; ++i) cb_new[(long long)e * DS + i] = cnt > 0 ? s[i] / c : cb_old[(long long)e * DS + i];
}

template <int DS, int MODE>
int pq_launch(const void* x, const float* cent, const int* assign, const float* cb, int n, int D, int m, int nlist,
              int slabs, unsigned char* codes, float* part, hipStream_t s) {
  static bool attr[BE_MAX_DEV] = {};
  if (!attr[be_cur_dev()]) {
    if (hipFuncSetAttribute((const void*)pq_assign_kernel<DS, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            PQ<DS>::LDS) != hipSuccess)
      return -30;
    attr[be_cur_dev()] = true;
  }
  hipLaunchKernelGGL((pq_assign_kernel<DS, MODE>), dim3((unsigned)(m / PQ_GROUP), (unsigned)slabs), dim3(PQ_NT),
                     PQ<DS>::LDS, s, x, cent, assign, cb, n, D, m, nlist, slabs, codes, part);
  return BE_CHECK_LAUNCH();
}

// 0 when the kernels serve the shape: sub-spaces of 4 or 8 dims, whole groups of 16 sub-spaces.
int pq_shape(int n, int D, int m) {
  if (m < 16 || m % 16) return -2;
  if (D != m * 4 && D != m * 8) return -1;
  if (n < 1) return -3;
  return 0;
}

}  // namespace

extern "C" {

// x [n, D] fp32 (x_bf16 = 0) or bf16 (1); cent [nlist, D] fp32; assign [n] int32; cb [m, 256, D/m] fp32 ->
// codes [n, m] uint8 (rows 16-byte aligned).  D/m in {4, 8} and m % 16 == 0, otherwise a negative status.
int be_pq_encode(const void* x, int x_bf16, const float* cent, const int* assign, const float* cb, int n, int D, int m,
                 int nlist, unsigned char* codes, hipStream_t s) {
  const int bad = pq_shape(n, D, m);
  if (bad) return bad;
  if (nlist < 1) return -4;
  const int T = (n + PQ_ROWS - 1) / PQ_ROWS, groups = m / PQ_GROUP;
  int slabs = 256 / groups;  // one workgroup per CU
  slabs = slabs < 1 ? 1 : (slabs > T ? T : slabs);
  if (D / m == 4)
    return x_bf16 ? pq_launch<4, PQ_BF16>(x, cent, assign, cb, n, D, m, nlist, slabs, codes, nullptr, s)
                  : pq_launch<4, PQ_F32>(x, cent, assign, cb, n, D, m, nlist, slabs, codes, nullptr, s);
  return x_bf16 ? pq_launch<8, PQ_BF16>(x, cent, assign, cb, n, D, m, nlist, slabs, codes, nullptr, s)
                : pq_launch<8, PQ_F32>(x, cent, assign, cb, n, D, m, nlist, slabs, codes, nullptr, s);
}

// res [S, D] fp32 residuals, cb [m, 256, D/m] -> cb_new (another buffer); part [slabs, m, 256, D/m + 1] is
// scratch that the first kernel fills completely.  slabs in 1..ceil(S / 128): the result's summation order
// depends on it, so the caller derives it from the shape alone.
int be_pq_kmeans_step(const float* res, const float* cb, int S, int D, int m, int slabs, float* part, float* cb_new,
                      hipStream_t s) {
  const int bad = pq_shape(S, D, m);
  if (bad) return bad;
  if (slabs < 1 || slabs > (S + PQ_ROWS - 1) / PQ_ROWS) return -5;
  const int rc = D / m == 4
                     ? pq_launch<4, PQ_KMEANS>(res, nullptr, nullptr, cb, S, D, m, 1, slabs, nullptr, part, s)
                     : pq_launch<8, PQ_KMEANS>(res, nullptr, nullptr, cb, S, D, m, 1, slabs, nullptr, part, s);
  if (rc) return rc;
  const dim3 grid((unsigned)m);  // m * 256 threads
  if (D / m == 4)
    hipLaunchKernelGGL(pq_kmeans_reduce_kernel<4>, grid, dim3(256), 0, s, part, cb, slabs, m, cb_new);
  else
    hipLaunchKernelGGL(pq_kmeans_reduce_kernel<8>, grid, dim3(256), 0, s, part, cb, slabs, m, cb_new);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
