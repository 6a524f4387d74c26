// Top-k selection in LDS, shared by the list scans that keep their best kk inside the kernel
// (ivfpq_search.hip, ivf_scan_topk.hip).
//
// Order: (score descending, row ascending).  A pair is packed into one 64-bit key, the high word a bit pattern
// that falls as the score rises (-0 counts as +0), the low word the row, so "precedes" is one unsigned compare
// and rows, unique within a query, make every key unique: what is kept never depends on the order in which
// candidates arrive.
//
// A workgroup keeps `cap` keys (a power of two >= 2 kk, at least 256), a count and a threshold, the current
// kk-th key (all ones while fewer than kk were selected).  A candidate is appended (LDS atomic on the count)
// only if its key is below the threshold; when a thread finds no slot the workgroup calls reselect().
#pragma once
#include "common.h"

namespace {

typedef unsigned long long key_t;
constexpr key_t KEY_PAD = ~0ull;

#define TOPK_NEG_INF (-__builtin_huge_valf())

__device__ __forceinline__ key_t make_key(float s, int row) {
  const unsigned u = s == 0.f ? 0u : __float_as_uint(s);
  const unsigned hi = (u & 0x80000000u) ? u : (~u & 0x7fffffffu);
  return ((key_t)hi << 32) | (unsigned)row;
}
__device__ __forceinline__ float key_score(key_t k) {
  const unsigned hi = (unsigned)(k >> 32);
  return __uint_as_float((hi & 0x80000000u) ? hi : (~hi & 0x7fffffffu));
}

// compare-exchange i of a bitonic step of distance j: the pair (lo, lo + j)
__device__ __forceinline__ int pair_lo(int i, int j) { return ((i & ~(j - 1)) << 1) | (i & (j - 1)); }

// The workgroup of NT threads sorts the min(*cnt, cap) keys of buf, keeps the first kk and refreshes the
// threshold.  Called by all threads after a barrier; the caller places a barrier after it.
template <int NT>
__device__ __forceinline__ void reselect(key_t* buf, int* cnt, key_t* thr, int cap, int kk, int tid) {
  int c = *cnt;
  c = c < cap ? c : cap;
  int n = 64;
  while (n < c) n <<= 1;
  for (int i = c + tid; i < n; i += NT) buf[i] = KEY_PAD;
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (n >> 1); i += NT) {
        const int lo = pair_lo(i, j);
        const key_t a = buf[lo], b = buf[lo + j];
        if ((a > b) == ((lo & k) == 0)) { buf[lo] = b; buf[lo + j] = a; }
      }
      __syncthreads();
    }
  if (tid == 0) {
    *cnt = c < kk ? c : kk;
    if (c >= kk) *thr = buf[kk - 1];
  }
}

}  // namespace
