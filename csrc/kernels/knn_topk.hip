// Brute-force k nearest neighbours for the landscape view's UMAP (search/umap.py): bf16 MFMA score
// tiles with the top-k selected inside the kernel, so no score ever reaches HBM.
//
//   be_knn_topk_bf16    A [m, K] . B [n, K]^T -> per row of A the kk largest inner products and their
//                       column indices, ordered by (score descending, index ascending), per column split
//   be_knn_merge        the splits' partial lists [m, S, kk] -> [m, kk] under the same order
//   be_knn_rescore_f32  fp32 inner products of the listed candidates (the exact scores the table keeps)
//
// be_knn_topk_bf16, MI355X design:
//  * 256 threads = 4 waves as 2 (rows) x 2 (columns); the workgroup owns 128 rows of A and one of S
//    contiguous ranges of 128-column tiles of B, which it sweeps in ascending order.  A wave owns
//    64 x 64 scores = 4 x 4 fragments of v_mfma_f32_16x16x32_bf16 (64 fp32 accumulators): 8 fragment
//    reads of 1 KiB feed 16 MFMAs, which is what the LDS port of a CU sustains with four waves.
//  * K in 64-deep steps, two LDS buffers of (A 128 rows + B 128 rows) x 128 B = 32 KiB.  Step t + 1 is
//    fetched from global memory into registers before step t's MFMAs and stored to the other buffer after
//    them: one barrier per step.  128-byte rows, 16-byte chunk c of row r at c ^ ((r >> 1) & 7)
//    (gemm_8p's conflict-free swizzle).  K % 32 == 0: the missing half of a last step is stored as zeros.
//  * Selection state in LDS: per row a list of CAP = 80 (score, index) slots, a count and a threshold
//    (the row's current kk-th entry, (-inf, INT_MAX) while the list is short).  When a tile's
//    accumulators are complete, an entry is appended (LDS atomic on the count) only if it precedes the
//    threshold in the total order.  A row whose slots ran out is re-selected by one wave (rank by counting
//    over the row's slots; ranks are a permutation because indices are unique), the threshold refreshed,
//    and the lanes that could not append try again.  Appends arrive in any order; what is kept never
//    depends on it, because the filter and every selection compare (score, index) pairs exactly.
//  * LDS: 64 KiB tiles + 80 KiB lists + 1.5 KiB thresholds and counts = 145.5 KiB, one workgroup per CU.
//  * No global atomic, no host read, no grid barrier.  Rows past m and columns past n are clamped when
//    loaded and never appended.
#include "common.h"

#include <limits.h>

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256, CAP = 80;
constexpr int IMG = 128 * 128;  // one operand image (bytes)
constexpr int OFF_LS = 4 * IMG;
constexpr int OFF_LI = OFF_LS + BM * CAP * 4;
constexpr int OFF_TS = OFF_LI + BM * CAP * 4;
constexpr int OFF_TI = OFF_TS + BM * 4;
constexpr int OFF_CNT = OFF_TI + BM * 4;
constexpr int LDS_KNN = OFF_CNT + BM * 4;
static_assert(LDS_KNN <= 160 * 1024, "LDS of one CU");

#define KNN_NEG_INF (-__builtin_huge_valf())

// (score a, index ia) strictly precedes (b, ib): larger score first, then the smaller index
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

struct Sel {
  float* ls;  // [BM][CAP]
  int* li;    // [BM][CAP]
  float* ts;  // [BM] threshold score
  int* ti;    // [BM] threshold index
  int* cnt;   // [BM] slots used (may count failed appends past CAP)
};

// One wave sorts row r's min(cnt, CAP) slots in place and keeps the first kk.
__device__ __forceinline__ void select_row(const Sel& s, int r, int kk, int lane) {
  int c = s.cnt[r];
  c = c < CAP ? c : CAP;
  float* v = s.ls + r * CAP;
  int* ix = s.li + r * CAP;
  const int l1 = lane + 64;
  const bool h0 = lane < c, h1 = l1 < c;
  const float v0 = h0 ? v[lane] : KNN_NEG_INF, v1 = h1 ? v[l1] : KNN_NEG_INF;
  const int i0 = h0 ? ix[lane] : INT_MAX, i1 = h1 ? ix[l1] : INT_MAX;
  int r0 = 0, r1 = 0;
  for (int t = 0; t < c; ++t) {
    const float w = v[t];
    const int iw = ix[t];
    r0 += before(w, iw, v0, i0) ? 1 : 0;
    r1 += before(w, iw, v1, i1) ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();  // every lane has read the row before any lane rewrites it
  if (h0 && r0 < kk) { v[r0] = v0; ix[r0] = i0; }
  if (h1 && r1 < kk) { v[r1] = v1; ix[r1] = i1; }
  if (c >= kk) {
    if (h0 && r0 == kk - 1) { s.ts[r] = v0; s.ti[r] = i0; }
    if (h1 && r1 == kk - 1) { s.ts[r] = v1; s.ti[r] = i1; }
  }
  if (lane == 0) s.cnt[r] = c < kk ? c : kk;
}

// Wave `wave` re-selects its 32 rows: those that ran out of slots, or (all) every row that holds anything.
__device__ __forceinline__ void select_rows(const Sel& s, int wave, int kk, int lane, bool all) {
  for (int rr = 0; rr < BM / 4; ++rr) {
    const int r = wave * (BM / 4) + rr;
    const int c = __builtin_amdgcn_readfirstlane(s.cnt[r]);
    if (all ? c > 0 : c >= CAP) select_row(s, r, kk, lane);
  }
}

__global__ __launch_bounds__(NT, 1) void knn_topk_bf16_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ B,
                                                              int m, int n, int K, int kk, int self_base, int S,
                                                              float* __restrict__ out_s, int* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  Sel sel;
  sel.ls = reinterpret_cast<float*>(smem + OFF_LS);
  sel.li = reinterpret_cast<int*>(smem + OFF_LI);
  sel.ts = reinterpret_cast<float*>(smem + OFF_TS);
  sel.ti = reinterpret_cast<int*>(smem + OFF_TI);
  sel.cnt = reinterpret_cast<int*>(smem + OFF_CNT);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.x * BM, split = blockIdx.y;
  const int T = (n + BN - 1) / BN;
  const int t_lo = (int)((long long)split * T / S), t_hi = (int)((long long)(split + 1) * T / S);
  const int nk = (K + BK - 1) / BK;

  for (int r = tid; r < BM; r += NT) {
    sel.ts[r] = KNN_NEG_INF;
    sel.ti[r] = INT_MAX;
    sel.cnt[r] = 0;
  }
  __syncthreads();

  // staging: thread -> 16-byte chunk sc of rows srow + 32 u of both operand images
  const int srow = tid >> 3, sc = tid & 7;
  long long aoff[4];
  int dst[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int R = srow + 32 * u;
    int row = m0 + R;
    row = row < m ? row : m - 1;
    aoff[u] = (long long)row * K + sc * 8;
    dst[u] = R * 128 + ((sc ^ ((R >> 1) & 7)) << 4);
  }
  const int frow = lane & 15, fch = lane >> 4, fsw = (frow >> 1) & 7;

  for (int t = t_lo; t < t_hi; ++t) {
    const int n0 = t * BN;
    long long boff[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int col = n0 + srow + 32 * u;
      col = col < n ? col : n - 1;
      boff[u] = (long long)col * K + sc * 8;
    }
    u32x4 ra[4], rb[4];
    auto fetch = [&](int step) {
      const int k0 = step * BK;
      const bool in = k0 + sc * 8 < K;  // K % 32 == 0: a chunk is whole or absent
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ra[u] = in ? *reinterpret_cast<const u32x4*>(A + aoff[u] + k0) : (u32x4){0u, 0u, 0u, 0u};
        rb[u] = in ? *reinterpret_cast<const u32x4*>(B + boff[u] + k0) : (u32x4){0u, 0u, 0u, 0u};
      }
    };
    auto stash = [&](int buf) {
      unsigned char* a = smem + buf * 2 * IMG;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        *reinterpret_cast<u32x4*>(a + dst[u]) = ra[u];
        *reinterpret_cast<u32x4*>(a + IMG + dst[u]) = rb[u];
      }
    };

    f32x4 acc[4][4];  // [column fragment j][row fragment i]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    fetch(0);
    stash(0);
    __syncthreads();
    for (int step = 0; step < nk; ++step) {
      const bool more = step + 1 < nk;
      if (more) fetch(step + 1);
      const unsigned char* sa = smem + (step & 1) * 2 * IMG + (wr * 64 + frow) * 128;
      const unsigned char* sb = smem + (step & 1) * 2 * IMG + IMG + (wc * 64 + frow) * 128;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int ch = ((ks * 4 + fch) ^ fsw) << 4;
        bf16x8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(sa + i * 16 * 128 + ch);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(sb + j * 16 * 128 + ch);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[j][i], 0, 0, 0);
      }
      if (more) stash((step + 1) & 1);
      __syncthreads();
    }

    // ---- selection: acc[j][i][e] is row wr*64 + i*16 + frow, column wc*64 + j*16 + 4*fch + e of the tile
    unsigned todo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + wr * 64 + i * 16 + frow;
      const int skip = self_base >= 0 ? self_base + row : -1;
      todo[i] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = n0 + wc * 64 + j * 16 + 4 * fch + e;
          if (row < m && col < n && col != skip) todo[i] |= 1u << (j * 4 + e);
        }
    }
    for (;;) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!todo[i]) continue;
        const int r = wr * 64 + i * 16 + frow;
        const float th = sel.ts[r];
        const int thi = sel.ti[r];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned bit = 1u << (j * 4 + e);
            if (!(todo[i] & bit)) continue;
            const float v = acc[j][i][e];
            const int col = n0 + wc * 64 + j * 16 + 4 * fch + e;
            if (before(v, col, th, thi)) {
              const int pos = atomicAdd(&sel.cnt[r], 1);
              if (pos < CAP) {
                sel.ls[r * CAP + pos] = v;
                sel.li[r * CAP + pos] = col;
                todo[i] &= ~bit;
              }
            } else {
              todo[i] &= ~bit;
            }
          }
      }
      // a bit is left only where a row had no slot: that row is at CAP and is re-selected to kk < CAP
      if (!__syncthreads_or((int)(todo[0] | todo[1] | todo[2] | todo[3]))) break;
      select_rows(sel, wave, kk, lane, false);
      __syncthreads();
    }
  }

  select_rows(sel, wave, kk, lane, true);
  __syncthreads();
  for (int o = tid; o < BM * kk; o += NT) {
    const int r = o / kk, t = o - r * kk;
    const int row = m0 + r;
    if (row >= m) break;
    const bool has = t < sel.cnt[r];
    const long long g = ((long long)row * S + split) * kk + t;
    out_s[g] = has ? sel.ls[r * CAP + t] : KNN_NEG_INF;
    out_i[g] = has ? sel.li[r * CAP + t] : -1;
  }
}

// One wave per row: lane l walks split l's sorted list; kk rounds of a wave-wide "first in the order".
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ ps, const int* __restrict__ pi, int m,
                                                        int S, int kk, float* __restrict__ out_s,
                                                        int* __restrict__ out_i) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const long long base = ((long long)row * S + lane) * kk;
  int p = 0;
  auto head = [&](float& v, int& ix) {
    v = KNN_NEG_INF;
    ix = INT_MAX;
    if (lane < S && p < kk) {
      const int c = pi[base + p];
      if (c >= 0) { v = ps[base + p]; ix = c; }
    }
  };
  float hv;
  int hi;
  head(hv, hi);
  for (int t = 0; t < kk; ++t) {
    float bv = hv;
    int bi = hi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      out_s[(long long)row * kk + t] = bi == INT_MAX ? KNN_NEG_INF : bv;
      out_i[(long long)row * kk + t] = bi == INT_MAX ? -1 : bi;
    }
    if (bi != INT_MAX && hi == bi) {  // column indices are unique across splits: one lane advances
      ++p;
      head(hv, hi);
    }
  }
}

// 16 lanes per (row, candidate): lane `sub` owns dims sub*4 + 64 c (float4 loads, 16 lanes cover 256
// contiguous bytes), one fmaf chain in ascending c, then a fixed xor butterfly.
__global__ __launch_bounds__(256) void knn_rescore_f32_kernel(const float* __restrict__ q, const float* __restrict__ x,
                                                              const int* __restrict__ cand, long long total, int n,
                                                              int d, int kk, float* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const long long e = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (e >= total) return;  // whole 16-lane groups leave together; the shuffles below stay inside a group
  const long long row = e / kk;
  const int c = cand[e];
  float s = 0.f;
  if (c >= 0 && c < n) {
    const float* a = q + row * d;
    const float* b = x + (long long)c * d;
    if ((d & 3) == 0) {
      for (int k = sub * 4; k < d; k += 64) {
        const float4 av = *reinterpret_cast<const float4*>(a + k);
        const float4 bv = *reinterpret_cast<const float4*>(b + k);
        s = fmaf(av.x, bv.x, s);
        s = fmaf(av.y, bv.y, s);
        s = fmaf(av.z, bv.z, s);
        s = fmaf(av.w, bv.w, s);
      }
    } else {
      for (int k = sub; k < d; k += 16) s = fmaf(a[k], b[k], s);
    }
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
  if (sub == 0) out[e] = (c >= 0 && c < n) ? s : KNN_NEG_INF;
}

}  // namespace

extern "C" {

// A [m, K], B [n, K] bf16 row-major; out_s / out_i [m, S, kk]: per row and column split the kk largest
// A[i].B[j] with their columns, (score descending, index ascending), padded with -inf / -1.  Column
// self_base + row is excluded when self_base >= 0.  S == 1 writes the final [m, kk] lists.
int be_knn_topk_bf16(const void* A, const void* B, int m, int n, int K, int kk, int self_base, int S, float* out_s,
                     int* out_i, hipStream_t s) {
  if (kk < 1 || kk > 64) return -1;
  if (K < 32 || K % 32) return -2;
  if (S < 1 || S > 65535) return -3;
  if (m < 0 || n < 1 || self_base < -1) return -4;
  if (m == 0) return 0;
  static bool attr[BE_MAX_DEV] = {};
  if (!attr[be_cur_dev()]) {
    if (hipFuncSetAttribute((const void*)knn_topk_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_KNN) !=
        hipSuccess)
      return -30;
    attr[be_cur_dev()] = true;
  }
  const dim3 grid((unsigned)((m + BM - 1) / BM), (unsigned)S);
  hipLaunchKernelGGL(knn_topk_bf16_kernel, grid, dim3(NT), LDS_KNN, s, (const bf16_t*)A, (const bf16_t*)B, m, n, K, kk,
                     self_base, S, out_s, out_i);
  return BE_CHECK_LAUNCH();
}

// part_s / part_i [m, S, kk] (each list ordered, padded with -inf / -1) -> out_s / out_i [m, kk].  S <= 64.
int be_knn_merge(const float* part_s, const int* part_i, int m, int S, int kk, float* out_s, int* out_i, hipStream_t s) {
  if (kk < 1 || kk > 64) return -1;
  if (S < 1 || S > 64) return -3;
  if (m < 0) return -4;
  if (m == 0) return 0;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, part_s, part_i, m, S, kk, out_s,
                     out_i);
  return BE_CHECK_LAUNCH();
}

// q [m, d], x [n, d] fp32; cand [m, kk] int32 -> out [m, kk]: q[i].x[cand[i, t]] in fp32, -inf for a
// candidate outside 0..n-1 (the -1 padding).
int be_knn_rescore_f32(const float* q, const float* x, const int* cand, int m, int n, int d, int kk, float* out,
                       hipStream_t s) {
  if (kk < 1 || d < 1 || n < 1 || m < 0) return -1;
  if (m == 0) return 0;
  const long long total = (long long)m * kk;
  const long long blocks = (total + 15) / 16;
  if (blocks >= (1LL << 31)) return -5;
  hipLaunchKernelGGL(knn_rescore_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q, x, cand, total, n, d, kk, out);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
