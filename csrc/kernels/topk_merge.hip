// The merge of the list scans' partial top-k lists (ivfpq_search.hip, ivf_scan_topk.hip): nothing of PQ or of
// the vectors in it.
//
//   be_topk_merge  the ranges' partial lists [Q, P, kk] -> [Q, kk], rows mapped to ids
//
// One workgroup of 512 threads per query sweeps the P kk partial keys through the selection of topk_select.h.
// The sweep goes level by level (element i of every range before element i + 1 of any), and every partial list is
// ascending, so once P consecutive elements were all rejected every range has a rejected element and whatever
// follows it is larger: the sweep ends there.  The cost is about kk + P keys and a few sorts of `cap` keys, not P
// sorted merges.  23 VGPRs, scratch 0 (hipcc -Rpass-analysis=kernel-resource-usage, gfx950).
#include "common.h"
#include "topk_select.h"

namespace {

constexpr int NT = 512;

__global__ __launch_bounds__(NT) void topk_sweep_kernel(const float* __restrict__ ps, const int* __restrict__ pr,
                                                        const long long* __restrict__ ids, int P, int kk, int cap,
                                                        float* __restrict__ out_s, long long* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  const float* qs = ps + q * P * kk;
  const int* qr = pr + q * P * kk;
  const Selector sel(smem, cap, kk, tid);
  __syncthreads();
  const long long total = (long long)P * kk;
  long long quiet = 0;  // consecutive elements, up to the chunk's end, that were all rejected
  for (long long e0 = 0; e0 < total && quiet < P; e0 += NT) {
    const long long e = e0 + tid;
    key_t key = KEY_PAD;
    if (e < total) {  // level i of range s
      const size_t g = (size_t)(e % P) * kk + (size_t)(e / P);
      const int r = qr[g];
      if (r >= 0) key = make_key(qs[g], r);
    }
    const bool passed = select_offer<NT, 1>(sel, key != KEY_PAD, [&](int) { return key; }, tid);
    quiet = __syncthreads_or(passed) ? 0 : quiet + NT;
  }
  select_finish<NT>(sel, tid, out_s + q * kk, out_i + q * kk, ids);
}

}  // namespace

extern "C" {

// part_s / part_r [Q, P, kk] (each list ordered, padded with -inf / -1) -> out_s [Q, kk], out_i [Q, kk]:
// ids[row] of the kk first rows under the order, or the row itself where ids is null; -inf / -1 in empty slots.
int be_topk_merge(const float* part_s, const int* part_r, const long long* ids, int Q, int P, int kk, float* out_s,
                  long long* out_i, hipStream_t s) {
  if (kk < 1 || kk > 1024) return -1;
  if (P < 1 || P > 65535) return -3;
  if (Q < 0) return -4;
  if (Q == 0) return 0;
  const int cap = select_cap(kk);
  hipLaunchKernelGGL(topk_sweep_kernel, dim3((unsigned)Q), dim3(NT), select_lds_bytes(cap), s, part_s, part_r, ids, P, kk,
                     cap, out_s, out_i);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
