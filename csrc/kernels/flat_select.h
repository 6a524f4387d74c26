// The per-query selection of the flat scans (flat_scan_topk.hip, flat_sq8_scan_topk.hip): a workgroup of 256 threads
// scores 256-row tiles against up to 64 queries and keeps, per query in LDS, `cap` 64-bit keys of topk_select.h, a
// count and a threshold, the current kk-th key (all ones while fewer than kk were selected).
//
// When a tile's scores are complete a key is appended (LDS atomic on the query's count) only if it is below the
// threshold.  A query whose list is full is re-selected by one wave by rank counting (select_row of knn_topk.hip on
// 64-bit keys; keys are unique, so ranks are a permutation and the list comes out sorted); the lanes that found no
// slot retry.  The workgroup vote is a 0 / 1 value.  What is kept never depends on the arrival order.  The bitonic
// reselect of topk_select.h is not used: it sorts one list with the whole workgroup and wants a power-of-two
// cap >= 256, 128 KiB for 64 queries.
//
// Score layout (the 16x16 MFMA accumulators of both kernels): score_of(i, t, e) of lane (r, g) = (lane & 15,
// lane >> 4) is row 64 wave + 16 i + 4 g + e of the tile against query 16 t + r, so a lane reads one threshold per
// query fragment.  Every function below is called by all threads of the workgroup from uniform control flow.
#pragma once
#include "topk_select.h"

namespace {

constexpr int NT = 256, TILE = 256, FLAT_MAX_K = 256, CAP_MAX = 320;
constexpr int LDS_BUDGET = 160 * 1024 - 256;  // less the static bytes of the barrier vote

constexpr int flat_lists_bytes(int qr, int cap) { return qr * (cap * 8 + 12); }

// host: keys per query next to `fixed` bytes of the workgroup's other LDS (the query image): what the budget allows,
// at most max(kk + 16, min(2 kk + 16, CAP_MAX)), a multiple of 8 (rank_select reads the list four keys at a time)
// and at least kk + 16; 0 where that does not fit.  The result of a scan does not depend on cap.
inline int flat_cap(int qr, long long fixed, int kk) {
  int want = 2 * kk + 16 < CAP_MAX ? 2 * kk + 16 : CAP_MAX;
  want = want > kk + 16 ? want : kk + 16;
  const long long room = ((long long)LDS_BUDGET - fixed) / qr;  // bytes per query for its list
  long long cap = (room - 12) / 8;
  if (room < 12 || (cap & ~7LL) < kk + 16) return 0;
  return (int)((cap < want ? cap : want) & ~7LL);
}

// keys[qr][cap] | thr[qr] | cnt[qr] at `lds` (8-byte aligned, flat_lists_bytes(qr, cap) bytes)
struct FlatLists {
  key_t* keys;
  key_t* thr;
  int* cnt;
  int cap, kk;
  __device__ __forceinline__ FlatLists(unsigned char* lds, int qr, int cap_, int kk_)
      : keys(reinterpret_cast<key_t*>(lds)), thr(keys + qr * cap_), cnt(reinterpret_cast<int*>(thr + qr)), cap(cap_),
        kk(kk_) {}
  // every list empty; the caller places a barrier between this and the first flat_offer
  __device__ __forceinline__ void clear(int qr, int tid) const {
    for (int r = tid; r < qr; r += NT) {
      thr[r] = KEY_PAD;
      cnt[r] = 0;
    }
  }
};

// One wave sorts the min(cnt, cap) keys of one query's list in place by rank counting, keeps the first kk and
// refreshes the threshold.  NS: list slots per lane.
template <int NS>
__device__ __forceinline__ void rank_select(key_t* buf, key_t* thr, int* cnt, int cap, int kk, int lane) {
  int c = *cnt;
  c = c < cap ? c : cap;
  key_t k[NS];
  int rank[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    k[j] = lane + 64 * j < c ? buf[lane + 64 * j] : KEY_PAD;
    rank[j] = 0;
  }
  // four keys per step, so that their LDS reads are in flight together (cap is a multiple of 8: a step may read
  // past c, never past the list; what it reads there is not counted)
  for (int t0 = 0; t0 < c; t0 += 4) {
    key_t w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = buf[t0 + u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < NS; ++j) rank[j] += (t0 + u < c && w[u] < k[j]) ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();  // every lane has read the list before any lane rewrites it
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const bool has = lane + 64 * j < c;
    if (has && rank[j] < kk) buf[rank[j]] = k[j];
    if (has && c >= kk && rank[j] == kk - 1) *thr = k[j];
  }
  if (lane == 0) *cnt = c < kk ? c : kk;
}

__device__ __forceinline__ void rank_select_list(const FlatLists& L, int qq, int lane) {
  if (L.cap <= 128) rank_select<2>(L.keys + qq * L.cap, L.thr + qq, L.cnt + qq, L.cap, L.kk, lane);
  else rank_select<CAP_MAX / 64>(L.keys + qq * L.cap, L.thr + qq, L.cnt + qq, L.cap, L.kk, lane);
}

// The complete scores of the tile at row0 are offered to the lists of the group's nq queries (QT query fragments);
// rows from N on are not.  Contains barriers and ends in one.
template <int QT, class ScoreOf>
__device__ __forceinline__ void flat_offer(const FlatLists& L, int nq, int N, int row0, int wave, int lane,
                                           ScoreOf score_of) {
  const int fr = lane & 15, fg = lane >> 4;
  const int rbase = row0 + wave * 64 + 4 * fg;
  unsigned todo[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    todo[t] = 0;
    if (16 * t + fr < nq) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (rbase + 16 * i + e < N) todo[t] |= 1u << (i * 4 + e);
    }
  }
  for (;;) {
    unsigned open = 0;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (!todo[t]) continue;
      const int qq = 16 * t + fr;
      const key_t th = L.thr[qq];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned bit = 1u << (i * 4 + e);
          if (!(todo[t] & bit)) continue;
          const key_t key = make_key(score_of(i, t, e), rbase + 16 * i + e);
          if (key < th) {
            const int pos = atomicAdd(&L.cnt[qq], 1);
            if (pos < L.cap) {
              L.keys[qq * L.cap + pos] = key;
              todo[t] &= ~bit;
            }
          } else {
            todo[t] &= ~bit;
          }
        }
      open |= todo[t];
    }
    // a bit is left only where a query had no slot: that list is at cap and is re-selected to kk < cap
    if (!__syncthreads_or(open != 0)) break;
    for (int qq = wave; qq < nq; qq += 4) {
      if (__builtin_amdgcn_readfirstlane(L.cnt[qq]) < L.cap) continue;
      rank_select_list(L, qq, lane);
    }
    __syncthreads();
  }
}

// Every list sorted and written as write_topk writes: out_of(qq) is the offset of query qq's kk pairs in out_s /
// out_r.  Called after the vote that ended the last flat_offer, which is the barrier before this.
template <class OutOf>
__device__ __forceinline__ void flat_finish(const FlatLists& L, int nq, int wave, int lane, OutOf out_of,
                                            float* out_s, int* out_r) {
  for (int qq = wave; qq < nq; qq += 4) {
    rank_select_list(L, qq, lane);
    __builtin_amdgcn_wave_barrier();
    write_topk<64, int>(L.keys + qq * L.cap, L.cnt[qq], L.kk, lane, out_s + out_of(qq), out_r + out_of(qq), nullptr);
  }
}

}  // namespace
