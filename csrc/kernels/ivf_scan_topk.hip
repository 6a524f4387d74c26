// IVF-Flat search with the top-k selected inside the exact list scan: no score row ever reaches HBM.
//
//   be_ivf_scan_topk  per (query, slot range) the kk best (score, list-sorted row) pairs of exact bf16 scores
//   be_ivf_merge      the ranges' partial lists [Q, P, kk] -> [Q, kk], rows mapped to ids
//
// Order everywhere: (score descending, list-sorted row ascending), the 64-bit keys of topk_select.h.
//
// No matrix instructions: every query has its own candidate set and every row is used once, so the scan is a
// bandwidth-bound GEMV per query (1.5 KB of bf16 per row at D = 768 against 2 D flop); there is no operand to
// reuse from an MFMA tile, and the VALU fmaf chain below is far from being the limit.
//
// be_ivf_scan_topk, MI355X design:
//  * A workgroup of 256 threads (4 waves, 16 lane groups of 16) owns one query and slots [s tot / P,
//    (s + 1) tot / P) of the query's candidate row, the concatenation of its probed lists.  The range ignores
//    list boundaries, so every workgroup of a query streams the same number of rows whatever the list sizes,
//    and the grid is Q P.
//  * A row is read by one lane group, each lane owning D / 16 dims as D / 128 16-byte loads (16 lanes cover 256
//    contiguous bytes per load); the query's matching fp32 slice stays in registers.  The range is swept in
//    chunks of 16 R slots (slot = chunk + 16 r + group, so the 16 groups read 16 adjacent rows).  The loads of
//    chunk v + 1 are issued before the arithmetic, the selection and the barrier of chunk v: 2 R rows per lane
//    group in flight, through registers (direct-to-LDS loads would only add an LDS round trip, no row is
//    shared).  R = 8 / 8 / 4 / 4 / 2 / 2 at D / 128 = 1 / 2 / 3 / 4 / 6 / 8, so a lane holds at most 32 loads
//    (at D = 768: 24 loads, 96 KiB in flight per workgroup).
//  * A group's slots only grow, so it keeps its current list (first slot, end slot, first row) in registers,
//    finds the first one by a binary search of the query's cand_off row and steps to the next list when a slot
//    passes the end; empty lists are stepped over.
//  * Score: the per-lane fmaf chain of be_ivf_scan_bf16 in the same element order, then the 16-lane xor-shuffle
//    reduction at offsets 8, 4, 2, 1: bit-equal to what that kernel writes.
//  * Selection in LDS (topk_select.h), only the lane of a group with sub == 0 taking part; one barrier per
//    chunk.  LDS holds nothing else: cap * 8 + 16 bytes, 2 KiB up to kk = 128 and 16 KiB at kk = 1024.
//  * Output: the sorted first kk keys unpacked to (score, row), padded with (-inf, -1).
//  * No global atomic, no host read, no grid barrier.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; launch bound 256 threads, 2 waves per SIMD
// planned, i.e. two workgroups on a CU, which 256 VGPRs allow):
//    D / 128        1     2     3     4     6     8
//    VGPRs        152   224   165   209   178   227
//    SGPRs         74    74    65    64    56    55
//    occupancy      3     2     3     2     2     2   waves per SIMD
//  scratch 0 and no AGPRs in every instantiation, LDS dynamic (above) plus 256 bytes of the barrier vote.  In the
//  sweep loop the arithmetic waits with vmcnt(17) .. vmcnt(12) at D = 768: the 12 loads of the next chunk stay in
//  flight across the selection and the barrier.  ivf_merge_kernel: 23 VGPRs, 57 SGPRs, scratch 0.
//
// be_ivf_merge: one workgroup of 512 threads per query sweeps the P kk partial keys through the same
// threshold / append / reselect selection.  The sweep goes level by level (element i of every range before
// element i + 1 of any), and every partial list is ascending, so once P consecutive elements were all rejected
// every range has a rejected element and whatever follows it is larger: the sweep ends there.  The cost is
// about kk + P keys and a few sorts of `cap` keys, not P sorted merges.
#include "common.h"
#include "topk_select.h"

namespace {

constexpr int SNT = 256;  // scan workgroup
constexpr int MNT = 512;  // merge workgroup

template <int CH>
struct RowsInFlight { static constexpr int R = CH <= 2 ? 8 : CH <= 4 ? 4 : 2; };

template <int CH>  // D = 128 * CH
__global__ __launch_bounds__(SNT, 2) void ivf_scan_topk_kernel(
    const float* __restrict__ q, const int* __restrict__ probes, const long long* __restrict__ list_off,
    const long long* __restrict__ cand_off, const bf16_t* __restrict__ vecs, int nprobe, int kk, int cap, int P,
    float* __restrict__ out_s, int* __restrict__ out_r) {
  constexpr int D = 128 * CH, R = RowsInFlight<CH>::R;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  key_t* buf = reinterpret_cast<key_t*>(smem);
  key_t* s_thr = buf + cap;
  int* s_cnt = reinterpret_cast<int*>(s_thr + 1);
  const int tid = threadIdx.x;
  const int sub = tid & 15, grp = tid >> 4;  // 16 lanes per row, 16 rows per sweep step
  const int qi = blockIdx.x / P, split = blockIdx.x - qi * P;
  const long long* co = cand_off + (size_t)qi * nprobe;
  const int* pr = probes + (size_t)qi * nprobe;
  float* os = out_s + (size_t)blockIdx.x * kk;
  int* orow = out_r + (size_t)blockIdx.x * kk;

  const int last = pr[nprobe - 1];
  const long long tot = co[nprobe - 1] + (list_off[last + 1] - list_off[last]);
  const long long lo = split * tot / P, hi = (split + 1) * tot / P;
  if (lo >= hi) {  // the whole workgroup: nothing selected
    for (int i = tid; i < kk; i += SNT) { os[i] = TOPK_NEG_INF; orow[i] = -1; }
    return;
  }
  if (tid == 0) { *s_cnt = 0; *s_thr = KEY_PAD; }

  float qv[CH][8];
  const float* qq = q + (size_t)qi * D;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float4 a = *reinterpret_cast<const float4*>(qq + c * 128 + sub * 8);
    const float4 b = *reinterpret_cast<const float4*>(qq + c * 128 + sub * 8 + 4);
    qv[c][0] = a.x; qv[c][1] = a.y; qv[c][2] = a.z; qv[c][3] = a.w;
    qv[c][4] = b.x; qv[c][5] = b.y; qv[c][6] = b.z; qv[c][7] = b.w;
  }
  __syncthreads();

  // the list that holds this lane group's current slot
  int p = 0;
  long long seg_start = 0, seg_end = 0, seg_row = 0;
  auto load_seg = [&]() {
    const int l = pr[p];
    const long long a = list_off[l];
    seg_start = co[p];
    seg_end = seg_start + (list_off[l + 1] - a);
    seg_row = a;
  };
  if (lo + grp < hi) {  // last p with co[p] <= slot: of lists that start at one slot, the one that is not empty
    int a = 0, b = nprobe - 1;
    while (a < b) {
      const int mid = (a + b + 1) >> 1;
      if (co[mid] <= lo + grp) a = mid; else b = mid - 1;
    }
    p = a;
    load_seg();
  }

  // rows of the chunk at c0 and their loads; a slot past the range has row -1 and loads row 0 (tot > 0, so it
  // exists), its score is never looked at
  auto fetch = [&](long long c0, int* row, u32x4 (*v)[CH]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long slot = c0 + r * 16 + grp;
      row[r] = -1;
      if (slot < hi) {
        while (slot >= seg_end && p + 1 < nprobe) { ++p; load_seg(); }
        row[r] = (int)(seg_row + (slot - seg_start));
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bf16_t* src = vecs + (size_t)(row[r] < 0 ? 0 : row[r]) * D + sub * 8;
#pragma unroll
      for (int c = 0; c < CH; ++c) v[r][c] = *reinterpret_cast<const u32x4*>(src + c * 128);
    }
  };

  // one chunk: the loads of the chunk after it go out first, into the other register set.  They go out even past
  // the range's end (16 R reads of row 0): behind a branch the compiler's wait counts, merged where the paths
  // join, waited for the new loads before the arithmetic on the old ones
  auto step = [&](long long c0, const int* row, const u32x4 (*v)[CH], int* rown, u32x4 (*vn)[CH]) {
    fetch(c0 + 16 * R, rown, vn);
    float s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s[r] = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s[r] = fmaf(lo_bf(v[r][c][j]), qv[c][2 * j], s[r]);
          s[r] = fmaf(hi_bf(v[r][c][j]), qv[c][2 * j + 1], s[r]);
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] += __shfl_xor(s[r], off, 16);
    unsigned todo = 0;
    if (sub == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) todo |= row[r] >= 0 ? 1u << r : 0u;
    }
    for (;;) {
      const key_t th = *s_thr;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!(todo >> r & 1u)) continue;
        const key_t key = make_key(s[r], row[r]);
        if (key < th) {
          const int pos = atomicAdd(s_cnt, 1);
          if (pos < cap) { buf[pos] = key; todo &= ~(1u << r); }
        } else {
          todo &= ~(1u << r);
        }
      }
      // a bit is left only where the buffer had no slot: it is re-selected to kk <= cap / 2 keys
      if (!__syncthreads_or((int)todo)) break;
      reselect<SNT>(buf, s_cnt, s_thr, cap, kk, tid);
      __syncthreads();
    }
  };

  // two register sets that swap roles (a copy between them would wait for the loads just issued)
  int row0[R], row1[R];
  u32x4 v0[R][CH], v1[R][CH];
  fetch(lo, row0, v0);
#pragma unroll 1
  for (long long c0 = lo; c0 < hi; c0 += 32 * R) {
    step(c0, row0, v0, row1, v1);
    if (c0 + 16 * R >= hi) break;
    step(c0 + 16 * R, row1, v1, row0, v0);
  }

  reselect<SNT>(buf, s_cnt, s_thr, cap, kk, tid);
  __syncthreads();
  const int c = *s_cnt;
  for (int i = tid; i < kk; i += SNT) {
    const key_t k = i < c ? buf[i] : KEY_PAD;
    os[i] = i < c ? key_score(k) : TOPK_NEG_INF;
    orow[i] = i < c ? (int)(unsigned)k : -1;
  }
}

__global__ __launch_bounds__(MNT) void ivf_merge_kernel(const float* __restrict__ ps, const int* __restrict__ pr,
                                                        const long long* __restrict__ ids, int P, int kk, int cap,
                                                        float* __restrict__ out_s, long long* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  key_t* buf = reinterpret_cast<key_t*>(smem);
  key_t* s_thr = buf + cap;
  int* s_cnt = reinterpret_cast<int*>(s_thr + 1);
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const float* qs = ps + q * P * kk;
  const int* qr = pr + q * P * kk;
  if (tid == 0) { *s_cnt = 0; *s_thr = KEY_PAD; }
  __syncthreads();
  const long long total = (long long)P * kk;
  long long quiet = 0;  // consecutive elements, up to the chunk's end, that were all rejected
  for (long long e0 = 0; e0 < total && quiet < P; e0 += MNT) {
    const long long e = e0 + tid;
    key_t key = KEY_PAD;
    if (e < total) {  // level i of range s
      const size_t g = (size_t)(e % P) * kk + (size_t)(e / P);
      const int r = qr[g];
      if (r >= 0) key = make_key(qs[g], r);
    }
    // the votes below are 0 / 1 each: __syncthreads_or reduces !!predicate, not the bits
    int todo = key != KEY_PAD, passed = 0;
    for (;;) {
      if (todo) {
        if (key < *s_thr) {
          passed = 1;
          const int pos = atomicAdd(s_cnt, 1);
          if (pos < cap) { buf[pos] = key; todo = 0; }
        } else {
          todo = 0;
        }
      }
      if (!__syncthreads_or(todo)) break;
      reselect<MNT>(buf, s_cnt, s_thr, cap, kk, tid);
      __syncthreads();
    }
    quiet = __syncthreads_or(passed) ? 0 : quiet + MNT;
  }
  reselect<MNT>(buf, s_cnt, s_thr, cap, kk, tid);
  __syncthreads();
  const int c = *s_cnt;
  for (int i = tid; i < kk; i += MNT) {
    const key_t k = i < c ? buf[i] : KEY_PAD;
    const int r = (int)(unsigned)k;
    out_s[q * kk + i] = i < c ? key_score(k) : TOPK_NEG_INF;
    out_i[q * kk + i] = i < c ? (ids ? ids[r] : (long long)r) : -1;
  }
}

int select_cap(int kk) {
  int cap = 256;
  while (cap < 2 * kk) cap <<= 1;
  return cap;
}

template <int CH>
int launch_scan_topk(const float* q, const int* probes, const long long* list_off, const long long* cand_off,
                     const bf16_t* vecs, int Q, int nprobe, int kk, int P, float* part_s, int* part_r, hipStream_t s) {
  const int cap = select_cap(kk);
  hipLaunchKernelGGL(ivf_scan_topk_kernel<CH>, dim3((unsigned)(Q * P)), dim3(SNT), cap * 8 + 16, s, q, probes, list_off,
                     cand_off, vecs, nprobe, kk, cap, P, part_s, part_r);
  return BE_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// q [Q, D] fp32; probes / cand_off [Q, nprobe] (cand_off the exclusive prefix sum of the probed lists' sizes);
// list_off [nlist + 1]; vecs [N, D] bf16, list-sorted; part_s / part_r [Q, P, kk].
int be_ivf_scan_topk(const float* q, const int* probes, const long long* list_off, const long long* cand_off,
                     const void* vecs, long long N, int Q, int nprobe, int D, int kk, int P, float* part_s, int* part_r,
                     hipStream_t s) {
  if (kk < 1 || kk > 1024) return -1;
  if (N < 0 || N >= (1LL << 31)) return -2;
  if (P < 1 || P > 65535) return -3;
  if (Q < 0 || nprobe < 1) return -4;
  if ((long long)Q * P >= (1LL << 31)) return -5;
  if (D < 128 || D % 128 || D > 1024) return -6;
  if (Q == 0) return 0;
  const bf16_t* v = reinterpret_cast<const bf16_t*>(vecs);
#define IVT_LAUNCH(CH) \
  case CH: return launch_scan_topk<CH>(q, probes, list_off, cand_off, v, Q, nprobe, kk, P, part_s, part_r, s)
  switch (D / 128) {
    IVT_LAUNCH(1);
    IVT_LAUNCH(2);
    IVT_LAUNCH(3);
    IVT_LAUNCH(4);
    IVT_LAUNCH(6);
    IVT_LAUNCH(8);
    default: return -6;
  }
#undef IVT_LAUNCH
}

// part_s / part_r [Q, P, kk] (each list ordered, padded with -inf / -1) -> out_s [Q, kk], out_i [Q, kk]:
// ids[row] of the kk first rows under the order, or the row itself where ids is null; -inf / -1 in empty slots.
int be_ivf_merge(const float* part_s, const int* part_r, const long long* ids, int Q, int P, int kk, float* out_s,
                 long long* out_i, hipStream_t s) {
  if (kk < 1 || kk > 1024) return -1;
  if (P < 1 || P > 65535) return -3;
  if (Q < 0) return -4;
  if (Q == 0) return 0;
  const int cap = select_cap(kk);
  hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)Q), dim3(MNT), cap * 8 + 16, s, part_s, part_r, ids, P, kk, cap,
                     out_s, out_i);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
