// IVF-PQ search with the top-k selected inside the list scan: no score row ever reaches HBM.
//
//   be_ivfpq_lut        q [Q, D] x codebooks [m, 256, ds] -> the fp16 lookup table [Q, m, 256]
//   be_ivfpq_scan_topk  per (query, split) the kk best (score, list-sorted row) pairs of one slot range
//   be_ivfpq_merge      the splits' partial lists [Q, P, kk] -> [Q, kk], rows mapped to ids (no PQ in it)
//
// Order everywhere: (score descending, list-sorted row ascending), the 64-bit keys of topk_select.h.
//
// be_ivfpq_scan_topk, MI355X design:
//  * A workgroup of 512 threads (8 waves) owns one query and slots [s tot / P, (s + 1) tot / P) of the query's
//    candidate row, the concatenation of its probed lists.  The range ignores list boundaries, so every
//    workgroup of a query scores the same number of rows whatever the list sizes, and the query's table is
//    staged into LDS once per workgroup for all of them.
//  * The range is swept in chunks of 2048 slots, 4 per thread (slot = chunk + 512 r + tid): four independent
//    chains of LDS lookups per thread hide the lookup latency.  Each thread walks the row with a cursor that
//    carries its list's base score (list_cursor.h).  Codes are read as 16-byte loads; the score is
//    base + sum_j t[j][code_j] in fp32, ascending j, starting from base: the order of be_ivfpq_scan, so the
//    scores are bit-equal.
//  * Selection in LDS behind the table (topk_select.h); one barrier per chunk.
//  * Output: the sorted first kk keys unpacked to (score, row), padded with (-inf, -1).
//  * LDS = table m * 512 B + cap * 8 B + 16 B:   m    16   32   48   64   96   128   192
//                                 kk <= 128 (KiB)     10   18   26   34   50    66    98
//                                 kk = 1024 (KiB)     24   32   40   48   64    80   112
//    so m = 192 runs one workgroup (2 waves per SIMD) on a CU's 160 KiB and m = 96 two.
//  * No global atomic, no host read, no grid barrier.
//
// be_ivfpq_merge: one workgroup per query.  The running list (KP = power of two >= kk keys, ascending, in
// LDS) takes one split at a time: element i becomes min(list[i], split[KP - 1 - i]), which leaves the KP
// smallest keys of both as a bitonic sequence, and log2(KP) compare-exchange steps sort it again.  It takes the same
// arguments as be_topk_merge (topk_merge.hip) and returns the same bits; at P <= 16 and kk = 1000 it measured
// 0.05 ms faster per search than the level sweep, so this path keeps it.
#include <hip/hip_fp16.h>

#include "common.h"
#include "list_cursor.h"
#include "topk_select.h"

namespace {

constexpr int NT = 512, RPT = 4;

// WPE: waves per SIMD the register budget must allow (4 = two workgroups on a CU, 2 = one)
template <int M, int WPE>
__global__ __launch_bounds__(NT, WPE) void ivfpq_scan_topk_kernel(
    const __half* __restrict__ lut, const float* __restrict__ base, const int* __restrict__ probes,
    const long long* __restrict__ list_off, const long long* __restrict__ cand_off,
    const unsigned char* __restrict__ codes, int nprobe, int kk, int cap, int P, float* __restrict__ out_s,
    int* __restrict__ out_r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __half* t = reinterpret_cast<__half*>(smem);
  const int tid = threadIdx.x;
  const int q = blockIdx.x / P, split = blockIdx.x - q * P;
  float* os = out_s + (size_t)blockIdx.x * kk;
  int* orow = out_r + (size_t)blockIdx.x * kk;

  ListCursor<true> cur(cand_off, probes, list_off, base, q, nprobe);
  long long lo, hi;
  cur.range(split, P, lo, hi);
  if (lo >= hi) {  // the whole workgroup: nothing staged, nothing selected
    select_nothing<NT>(kk, tid, os, orow);
    return;
  }
  const __half* lq = lut + (size_t)q * M * 256;
  for (int e = tid * 8; e < M * 256; e += NT * 8)
    *reinterpret_cast<uint4*>(t + e) = *reinterpret_cast<const uint4*>(lq + e);
  const Selector sel(smem + M * 512, cap, kk, tid);
  __syncthreads();
  if (lo + tid < hi) cur.seek(lo + tid);

  for (long long c0 = lo; c0 < hi; c0 += NT * RPT) {
    float acc[RPT];
    int row[RPT];
    unsigned todo = 0;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const long long slot = c0 + r * NT + tid;
      acc[r] = 0.f;
      row[r] = 0;
      if (slot < hi) {
        row[r] = cur.row(slot);
        acc[r] = cur.base;
        todo |= 1u << r;
      }
    }
    // codes of step v + 1 are fetched before the lookups of step v: 8 x 16 bytes in flight per thread
    uint4 w[RPT], wn[RPT];
    auto fetch = [&](uint4* d, int v) {
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        d[r] = (todo >> r & 1u) ? reinterpret_cast<const uint4*>(codes + (size_t)row[r] * M)[v] : make_uint4(0, 0, 0, 0);
    };
    fetch(w, 0);
#pragma unroll 1
    for (int v = 0; v < M / 16; ++v) {
      if (v + 1 < M / 16) fetch(wn, v + 1);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int j = v * 16 + k;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const unsigned ww = (k >> 2) == 0 ? w[r].x : (k >> 2) == 1 ? w[r].y : (k >> 2) == 2 ? w[r].z : w[r].w;
          acc[r] += __half2float(t[j * 256 + ((ww >> ((k & 3) * 8)) & 0xffu)]);
        }
      }
#pragma unroll
      for (int r = 0; r < RPT; ++r) w[r] = wn[r];
    }
    key_t key[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) key[r] = make_key(acc[r], row[r]);
    select_offer<NT, RPT>(sel, todo, [&](int r) { return key[r]; }, tid);
  }
  select_finish<NT>(sel, tid, os, orow, nullptr);
}

__global__ __launch_bounds__(NT) void topk_merge_kernel(const float* __restrict__ ps, const int* __restrict__ pr,
                                                        const long long* __restrict__ ids, int P, int kk, int KP,
                                                        float* __restrict__ out_s, long long* __restrict__ out_i) {
  __shared__ key_t mb[1024];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  auto part = [&](int s, int i) -> key_t {
    if (i >= kk) return KEY_PAD;
    const size_t g = (q * P + s) * kk + i;
    const int r = pr[g];
    return r < 0 ? KEY_PAD : make_key(ps[g], r);
  };
  for (int i = tid; i < KP; i += NT) mb[i] = part(0, i);
  __syncthreads();
  for (int s = 1; s < P; ++s) {
    for (int i = tid; i < KP; i += NT) {
      const key_t a = mb[i], b = part(s, KP - 1 - i);
      mb[i] = a < b ? a : b;
    }
    __syncthreads();
    for (int j = KP >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (KP >> 1); i += NT) {
        const int lo = pair_lo(i, j);
        const key_t a = mb[lo], b = mb[lo + j];
        if (a > b) { mb[lo] = b; mb[lo + j] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < kk; i += NT) {
    const key_t k = mb[i];
    const bool has = k != KEY_PAD;
    const int r = (int)(unsigned)k;
    out_s[q * kk + i] = has ? key_score(k) : TOPK_NEG_INF;
    out_i[q * kk + i] = has ? (ids ? ids[r] : (long long)r) : -1;
  }
}

// One workgroup per (query, sub-space), a thread per codeword: one fmaf chain in ascending i.
__global__ __launch_bounds__(256) void ivfpq_lut_kernel(const float* __restrict__ q, const float* __restrict__ cb, int m,
                                                        int ds, __half* __restrict__ lut) {
  const size_t g = blockIdx.x;
  const int j = (int)(g % m);
  const float* qv = q + (g / m) * ((size_t)m * ds) + (size_t)j * ds;
  const float* c = cb + ((size_t)j * 256 + threadIdx.x) * ds;
  float acc = 0.f;
  for (int i = 0; i < ds; ++i) acc = fmaf(qv[i], c[i], acc);
  lut[g * 256 + threadIdx.x] = __float2half_rn(acc);
}

template <int M, int WPE>
int launch_scan_topk(int slot, const __half* lut, const float* base, const int* probes, const long long* list_off,
                     const long long* cand_off, const unsigned char* codes, int Q, int nprobe, int kk, int cap, int P,
                     float* out_s, int* out_r, hipStream_t s) {
  const int lds = M * 512 + select_lds_bytes(cap);
  constexpr int LDS_MAX = M * 512 + select_lds_bytes(select_cap(1024));
  static_assert(LDS_MAX <= 160 * 1024, "LDS of one CU");
  static bool attr[8][BE_MAX_DEV] = {};
  if (!attr[slot][be_cur_dev()]) {
    if (hipFuncSetAttribute((const void*)ivfpq_scan_topk_kernel<M, WPE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_MAX) != hipSuccess)
      return -30;
    attr[slot][be_cur_dev()] = true;
  }
  hipLaunchKernelGGL((ivfpq_scan_topk_kernel<M, WPE>), dim3((unsigned)(Q * P)), dim3(NT), lds, s, lut, base, probes,
                     list_off, cand_off, codes, nprobe, kk, cap, P, out_s, out_r);
  return BE_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// q [Q, m * ds], cb [m, 256, ds] fp32 -> lut [Q, m, 256] fp16.
int be_ivfpq_lut(const float* q, const float* cb, int Q, int m, int ds, void* lut, hipStream_t s) {
  if (Q < 0 || m < 1 || ds < 1) return -1;
  if ((long long)Q * m >= (1LL << 31)) return -5;
  if (Q == 0) return 0;
  hipLaunchKernelGGL(ivfpq_lut_kernel, dim3((unsigned)(Q * m)), dim3(256), 0, s, q, cb, m, ds,
                     reinterpret_cast<__half*>(lut));
  return BE_CHECK_LAUNCH();
}

// lut [Q, m, 256] fp16; base / probes / cand_off [Q, nprobe] (cand_off the exclusive prefix sum of the probed
// lists' sizes); list_off [nlist + 1]; codes [N, m] uint8, list-sorted; part_s / part_r [Q, P, kk].
int be_ivfpq_scan_topk(const void* lut, const float* base, const int* probes, const long long* list_off,
                       const long long* cand_off, const unsigned char* codes, long long N, int Q, int nprobe, int m,
                       int kk, int P, float* part_s, int* part_r, hipStream_t s) {
  if (kk < 1 || kk > 1024) return -1;
  if (N < 0 || N >= (1LL << 31)) return -2;
  if (P < 1 || P > 65535) return -3;
  if (Q < 0 || nprobe < 1) return -4;
  if ((long long)Q * P >= (1LL << 31)) return -5;
  if (Q == 0) return 0;
  const int cap = select_cap(kk);
  const __half* l = reinterpret_cast<const __half*>(lut);
#define PQS_LAUNCH(slot, M, WPE)                                                                                     \
  case M:                                                                                                            \
    return launch_scan_topk<M, WPE>(slot, l, base, probes, list_off, cand_off, codes, Q, nprobe, kk, cap, P, part_s, \
                                    part_r, s)
  switch (m) {
    PQS_LAUNCH(0, 16, 4);
    PQS_LAUNCH(1, 32, 4);
    PQS_LAUNCH(2, 48, 4);
    PQS_LAUNCH(3, 64, 4);
    PQS_LAUNCH(4, 96, 4);
    PQS_LAUNCH(5, 128, 2);
    PQS_LAUNCH(6, 192, 2);
    default: return -6;
  }
#undef PQS_LAUNCH
}

// part_s / part_r [Q, P, kk] (each list ordered, padded with -inf / -1) -> out_s [Q, kk], out_i [Q, kk]:
// ids[row] of the kk first rows under the order, or the row itself where ids is null; -inf / -1 in empty slots.
int be_ivfpq_merge(const float* part_s, const int* part_r, const long long* ids, int Q, int P, int kk, float* out_s,
                   long long* out_i, hipStream_t s) {
  if (kk < 1 || kk > 1024) return -1;
  if (P < 1) return -3;
  if (Q < 0) return -4;
  if (Q == 0) return 0;
  int KP = 1;
  while (KP < kk) KP <<= 1;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(NT), 0, s, part_s, part_r, ids, P, kk, KP, out_s, out_i);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
