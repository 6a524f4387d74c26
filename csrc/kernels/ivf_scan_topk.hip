// IVF-Flat search with the top-k selected inside the exact list scan: no score row ever reaches HBM.
//
//   be_ivf_scan_topk  per (query, slot range) the kk best (score, list-sorted row) pairs of exact bf16 scores
// The ranges' partial lists [Q, P, kk] are joined and mapped to ids by be_topk_merge (topk_merge.hip).
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
//  * Each lane group walks the row with a cursor (list_cursor.h).
//  * Score: the per-lane fmaf chain of be_ivf_scan_bf16 in the same element order, then the 16-lane xor-shuffle
//    reduction at offsets 8, 4, 2, 1: bit-equal to what that kernel writes.
//  * Selection in LDS (topk_select.h), only the lane of a group with sub == 0 taking part; one barrier per
//    chunk.  LDS holds nothing else: 2 KiB up to kk = 128 and 16 KiB at kk = 1024.
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
//  flight across the selection and the barrier.
#include "common.h"
#include "list_cursor.h"
#include "topk_select.h"

namespace {

constexpr int NT = 256;

template <int CH>
struct RowsInFlight { static constexpr int R = CH <= 2 ? 8 : CH <= 4 ? 4 : 2; };

template <int CH>  // D = 128 * CH
__global__ __launch_bounds__(NT, 2) void ivf_scan_topk_kernel(
    const float* __restrict__ q, const int* __restrict__ probes, const long long* __restrict__ list_off,
    const long long* __restrict__ cand_off, const bf16_t* __restrict__ vecs, int nprobe, int kk, int cap, int P,
    float* __restrict__ out_s, int* __restrict__ out_r) {
  constexpr int D = 128 * CH, R = RowsInFlight<CH>::R;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int sub = tid & 15, grp = tid >> 4;  // 16 lanes per row, 16 rows per sweep step
  const int qi = blockIdx.x / P, split = blockIdx.x - qi * P;
  float* os = out_s + (size_t)blockIdx.x * kk;
  int* orow = out_r + (size_t)blockIdx.x * kk;

  ListCursor<false> cur(cand_off, probes, list_off, nullptr, qi, nprobe);
  long long lo, hi;
  cur.range(split, P, lo, hi);
  if (lo >= hi) {  // the whole workgroup: nothing selected
    select_nothing<NT>(kk, tid, os, orow);
    return;
  }
  const Selector sel(smem, cap, kk, tid);

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

  if (lo + grp < hi) cur.seek(lo + grp);  // this lane group's position in the row

  // rows of the chunk at c0 and their loads; a slot past the range has row -1 and loads row 0 (tot > 0, so it
  // exists), its score is never looked at
  auto fetch = [&](long long c0, int* row, u32x4 (*v)[CH]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long slot = c0 + r * 16 + grp;
      row[r] = -1;
      if (slot < hi) row[r] = cur.row(slot);
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
    select_offer<NT, R>(sel, todo, [&](int r) { return make_key(s[r], row[r]); }, tid);
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

  select_finish<NT>(sel, tid, os, orow, nullptr);
}

template <int CH>
int launch_scan_topk(const float* q, const int* probes, const long long* list_off, const long long* cand_off,
                     const bf16_t* vecs, int Q, int nprobe, int kk, int P, float* part_s, int* part_r, hipStream_t s) {
  const int cap = select_cap(kk);
  hipLaunchKernelGGL(ivf_scan_topk_kernel<CH>, dim3((unsigned)(Q * P)), dim3(NT), select_lds_bytes(cap), s, q, probes, list_off,
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

}  // extern "C"
