// A position in a query's candidate row, the concatenation of its probed lists (ivfpq_search.hip,
// ivf_scan_topk.hip).  cand_off [Q, nprobe] is the exclusive prefix sum of the probed lists' sizes, so slot s of
// query q lies in the last probed list p with cand_off[q, p] <= s: of lists that start at one slot, the one that is
// not empty.  A thread's (or lane group's) slots only grow, so it keeps its current list (first slot, end slot,
// first list-sorted row and, where BASE, the list's base score) in registers, finds the first one by a binary
// search and steps to the next list when a slot passes the end; empty lists are stepped over.
#pragma once
#include "common.h"

namespace {

template <bool BASE>
struct ListCursor {
  const long long* co;        // cand_off of the query
  const int* pr;              // probes of the query
  const long long* list_off;  // [nlist + 1]
  const float* bs;            // base scores of the query (BASE only)
  int nprobe;
  int p = 0;
  long long seg_start = 0, seg_end = 0, seg_row = 0;
  float base = 0.f;  // of the list of the last row() (BASE only)

  __device__ ListCursor(const long long* cand_off, const int* probes, const long long* list_off_, const float* base_,
                        int q, int nprobe_)
      : co(cand_off + (size_t)q * nprobe_), pr(probes + (size_t)q * nprobe_), list_off(list_off_),
        bs(BASE ? base_ + (size_t)q * nprobe_ : nullptr), nprobe(nprobe_) {}

  // slots [lo, hi) of range `split` of P: equal shares of the row whatever the list sizes
  __device__ void range(int split, int P, long long& lo, long long& hi) const {
    const int last = pr[nprobe - 1];
    const long long tot = co[nprobe - 1] + (list_off[last + 1] - list_off[last]);
    lo = split * tot / P;
    hi = (split + 1) * tot / P;
  }

  __device__ void load() {
    const int l = pr[p];
    const long long a = list_off[l];
    seg_start = co[p];
    seg_end = seg_start + (list_off[l + 1] - a);
    seg_row = a;
    if (BASE) base = bs[p];
  }

  // to the list of `slot`, a slot of the row
  __device__ void seek(long long slot) {
    int a = 0, b = nprobe - 1;
    while (a < b) {
      const int mid = (a + b + 1) >> 1;
      if (co[mid] <= slot) a = mid; else b = mid - 1;
    }
    p = a;
    load();
  }

  // list-sorted row of `slot`, a slot of the row not below the last one asked for (or sought)
  __device__ int row(long long slot) {
    while (slot >= seg_end && p + 1 < nprobe) { ++p; load(); }
    return (int)(seg_row + (slot - seg_start));
  }
};

}  // namespace
