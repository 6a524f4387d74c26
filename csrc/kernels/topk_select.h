// Top-k selection in LDS, shared by the list scans that keep their best kk inside the kernel
// (ivfpq_search.hip, ivf_scan_topk.hip) and by the merge of their partial lists (topk_merge.hip).
//
// Order: (score descending, row ascending).  A pair is packed into one 64-bit key, the high word a bit pattern
// that falls as the score rises (-0 counts as +0), the low word the row, so "precedes" is one unsigned compare
// and rows, unique within a query, make every key unique: what is kept never depends on the order in which
// candidates arrive.
//
// A workgroup keeps `cap` keys (a power of two >= 2 kk, at least 256), a count and a threshold, the current
// kk-th key (all ones while fewer than kk were selected).  A candidate is appended (LDS atomic on the count)
// only if its key is below the threshold; when a thread finds no slot the workgroup sorts the buffer (bitonic,
// ascending keys), keeps the first kk, refreshes the threshold, and the threads that could not append test
// their candidates again.
//
// The protocol is made of barriers and workgroup votes, so every helper below is called by ALL threads of the
// workgroup, from workgroup-uniform control flow (an early return must be taken by the whole workgroup).  A vote
// given to __syncthreads_or is a 0 / 1 value and so is its result: the call reduces !!predicate, not the bits.
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

// host: keys a workgroup keeps for kk results, and the dynamic LDS they take with the threshold and the count
constexpr int select_cap(int kk) {
  int cap = 256;
  while (cap < 2 * kk) cap <<= 1;
  return cap;
}
constexpr int select_lds_bytes(int cap) { return cap * 8 + 16; }

// buf[cap] | thr | cnt at `lds` (8-byte aligned, select_lds_bytes(cap) bytes), emptied.  Called by all threads;
// the caller places a barrier between this and the first select_offer.
struct Selector {
  key_t* buf;
  key_t* thr;
  int* cnt;
  int cap, kk;
  __device__ __forceinline__ Selector(unsigned char* lds, int cap_, int kk_, int tid)
      : buf(reinterpret_cast<key_t*>(lds)), thr(buf + cap_), cnt(reinterpret_cast<int*>(thr + 1)), cap(cap_), kk(kk_) {
    if (tid == 0) { *cnt = 0; *thr = KEY_PAD; }
  }
};

// The workgroup of NT threads sorts the min(*cnt, cap) keys of buf, keeps the first kk and refreshes the
// threshold.  Called by all threads after a barrier; contains barriers; the caller places a barrier after it.
template <int NT>
__device__ __forceinline__ void reselect(const Selector& s, int tid) {
  key_t* buf = s.buf;
  int c = *s.cnt;
  c = c < s.cap ? c : s.cap;
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
    *s.cnt = c < s.kk ? c : s.kk;
    if (c >= s.kk) *s.thr = buf[s.kk - 1];
  }
}

// A thread offers the candidates r < R whose bit is set in `todo` (0 for a thread that has none), key_of(r) their
// keys.  Returns whether one of them was below the threshold.  Called by all threads of the workgroup of NT, after
// a barrier that follows the last write of the selector; contains barriers, and ends in one.
template <int NT, int R, class KeyOf>
__device__ __forceinline__ bool select_offer(const Selector& s, unsigned todo, KeyOf key_of, int tid) {
  bool passed = false;
  for (;;) {
    const key_t th = *s.thr;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!(todo >> r & 1u)) continue;
      const key_t key = key_of(r);
      if (key < th) {
        passed = true;
        const int pos = atomicAdd(s.cnt, 1);
        if (pos < s.cap) { s.buf[pos] = key; todo &= ~(1u << r); }
      } else {
        todo &= ~(1u << r);
      }
    }
    // a bit is left only where the buffer had no slot: it is re-selected to kk <= cap / 2 keys
    if (!__syncthreads_or(todo != 0)) break;
    reselect<NT>(s, tid);
    __syncthreads();
  }
  return passed;
}

// The first min(c, kk) keys of buf unpacked to (score, row), or to (score, ids[row]) where ids is given, the rest
// of the kk pairs (-inf, -1).  No barrier in it.
template <int NT, class IdT>
__device__ __forceinline__ void write_topk(const key_t* buf, int c, int kk, int tid, float* out_s, IdT* out_i,
                                           const long long* ids) {
  for (int i = tid; i < kk; i += NT) {
    const key_t k = i < c ? buf[i] : KEY_PAD;
    const int r = (int)(unsigned)k;
    out_s[i] = i < c ? key_score(k) : TOPK_NEG_INF;
    out_i[i] = i < c ? (ids ? (IdT)ids[r] : (IdT)r) : (IdT)-1;
  }
}

// The result of a workgroup that selected nothing (an empty range: no Selector was made).
template <int NT, class IdT>
__device__ __forceinline__ void select_nothing(int kk, int tid, float* out_s, IdT* out_i) {
  write_topk<NT, IdT>(nullptr, 0, kk, tid, out_s, out_i, nullptr);
}

// The final selection, written as write_topk writes.  Called by all threads after the barrier that ends the last
// select_offer (or follows the Selector's construction); contains barriers.
template <int NT, class IdT>
__device__ __forceinline__ void select_finish(const Selector& s, int tid, float* out_s, IdT* out_i,
                                              const long long* ids) {
  reselect<NT>(s, tid);
  __syncthreads();
  write_topk<NT, IdT>(s.buf, *s.cnt, s.kk, tid, out_s, out_i, ids);
}

}  // namespace
