// Cellpose evaluation: average precision of predicted labels against ground truth (gfx950).
//
// Semantics: bioengine_worker_amd/cellpose/metrics.py::average_precision (the CPU oracle; the GPU
// tests compare exactly).  Two host entry points, queued back to back on one stream:
//
//   be_cp_ap_overlap   all B image pairs in ONE launch: sparse (t, p) -> common-pixel counts in a
//                      per-image open-addressing hash table in global memory (the scheme of
//                      cellpose_stitch.hip: runs of equal pairs collapsed inside a wave, an LDS table
//                      per workgroup, one global atomic per distinct pair and workgroup)
//   be_cp_ap_match     two passes over the occupied slots: label areas (and from them the label
//                      maxima, one workgroup per image and side), then the fp64 IoU of every pair
//                      against up to 8 ascending thresholds -> edge counts (one atomic per wave and
//                      threshold), per-label degrees and the conflict words
//
// The table also holds the pairs with one background side, (t, 0) and (0, p): a label's area is the
// sum of its row (column) of the table, as the oracle's `ov.sum(1)` / `ov.sum(0)`, so T and P are
// read exactly once and no label is ever used as an index before it passed the range check (a label
// outside [0, bound) sets the error word and its pixel is skipped).
//
// Every loop is bounded: hash probing gives up after `capacity` probes (sets the overflow word and
// drops the increment; the caller re-runs with a larger table), and no kernel waits on another
// workgroup.  Integer atomics only: the result does not depend on arrival order.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int OV_THREADS = 256;
constexpr int OV_ITERS = 8;                        // 256 lanes x 4 px x 8 = 8192 pixels per workgroup
constexpr int OV_SPAN = OV_THREADS * 4 * OV_ITERS;
constexpr int LDS_SLOTS = 1024;                    // 12 KiB: keys (8 B) + counts (4 B)
constexpr int LDS_PROBES = 16;
constexpr u64 NONUNI = ~0ULL;                      // lane whose 4 pixels do not share one key
constexpr int MAX_THR = 8;

__device__ __forceinline__ unsigned hash_key(u64 key) {
  unsigned h = (unsigned)(key >> 32) * 0x9E3779B1u ^ (unsigned)key * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0xC2B2AE3Du;
  h ^= h >> 13;
  return h;
}

// Bounded insert-or-add into table `gk/gv` (capacity `cap`, a power of two; key 0 = empty slot).
__device__ __forceinline__ void global_add(u64 key, int c, u64* __restrict__ gk, int* __restrict__ gv, int cap,
                                           int* __restrict__ overflow) {
  unsigned h = hash_key(key) & (unsigned)(cap - 1);
  for (int i = 0; i < cap; ++i) {
    u64 old = gk[h];  // most adds find their key already claimed: skip the CAS then
    if (old == 0) old = atomicCAS(gk + h, 0ULL, key);
    if (old == 0 || old == key) {
      atomicAdd(gv + h, c);
      return;
    }
    h = (h + 1) & (unsigned)(cap - 1);
  }
  atomicOr(overflow, 1);  // table full: the increment is dropped, the host re-runs with 2 x cap
}

__device__ __forceinline__ void lds_add(u64 key, int c, u64* lk, int* lc, u64* __restrict__ gk, int* __restrict__ gv,
                                        int cap, int* __restrict__ overflow) {
  unsigned h = hash_key(key) & (LDS_SLOTS - 1);
#pragma unroll 1
  for (int i = 0; i < LDS_PROBES; ++i) {
    u64 old = lk[h];
    if (old == 0) old = atomicCAS(lk + h, 0ULL, key);
    if (old == 0 || old == key) {
      atomicAdd(lc + h, c);
      return;
    }
    h = (h + 1) & (LDS_SLOTS - 1);
  }
  global_add(key, c, gk, gv, cap, overflow);  // crowded LDS table: straight to the image's table
}

// (t << 32 | p); 0 for background on both sides and for a label outside its bound (error word set).
__device__ __forceinline__ u64 pair_key(int t, int p, int nt, int np, int* __restrict__ error) {
  if ((unsigned)t >= (unsigned)nt || (unsigned)p >= (unsigned)np) {
    atomicOr(error, 1);
    return 0ULL;
  }
  return ((u64)(unsigned)t << 32) | (unsigned)p;
}

// grid (chunks, B): workgroup (x, y) counts pixels [x * OV_SPAN, +OV_SPAN) of image pair y.
__global__ __launch_bounds__(OV_THREADS) void ap_overlap_kernel(const int* __restrict__ T, const int* __restrict__ P,
                                                                int N, int nt, int np, u64* __restrict__ keys,
                                                                int* __restrict__ vals, int cap,
                                                                int* __restrict__ flags) {
  __shared__ u64 lk[LDS_SLOTS];
  __shared__ int lc[LDS_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < LDS_SLOTS; i += OV_THREADS) {
    lk[i] = 0;
    lc[i] = 0;
  }
  __syncthreads();
  const int img = blockIdx.y;
  const int* __restrict__ Tb = T + (size_t)img * N;
  const int* __restrict__ Pb = P + (size_t)img * N;
  u64* gk = keys + (size_t)img * cap;
  int* gv = vals + (size_t)img * cap;
  int* overflow = flags;
  int* error = flags + 1;
  // 16-byte loads need both images aligned (N % 4 == 0 and an aligned base); otherwise scalar
  const bool aligned = ((((uintptr_t)Tb) | ((uintptr_t)Pb)) & 15) == 0;
  const long long base = (long long)blockIdx.x * OV_SPAN;
#pragma unroll 1
  for (int it = 0; it < OV_ITERS; ++it) {  // trip count is uniform: every lane reaches the shuffles
    const long long px = base + ((long long)it * OV_THREADS + tid) * 4;
    int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (px + 4 <= N && aligned) {
      const int4 va = *reinterpret_cast<const int4*>(Tb + px);
      const int4 vb = *reinterpret_cast<const int4*>(Pb + px);
      a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
      b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < N) {
          a[i] = Tb[px + i];
          b[i] = Pb[px + i];
        }
    }
    u64 k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = pair_key(a[i], b[i], nt, np, error);
    const bool uni = k[0] == k[1] && k[1] == k[2] && k[2] == k[3];
    const u64 ukey = uni ? k[0] : NONUNI;
    // runs of lanes with one key collapse to a single LDS add by the run's first lane
    const u64 prev = __shfl_up(ukey, 1, 64);
    const bool head = lane == 0 || prev != ukey || ukey == NONUNI;
    const u64 heads = __ballot(head);
    if (ukey == NONUNI) {
      u64 cur = k[0];
      int run = 1;
#pragma unroll
      for (int i = 1; i < 4; ++i) {
        if (k[i] != cur) {
          if (cur) lds_add(cur, run, lk, lc, gk, gv, cap, overflow);
          cur = k[i];
          run = 0;
        }
        ++run;
      }
      if (cur) lds_add(cur, run, lk, lc, gk, gv, cap, overflow);
    } else if (head && ukey != 0) {
      const u64 rest = (heads >> lane) >> 1;  // heads above this lane
      const int lanes = rest ? __ffsll((long long)rest) : 64 - lane;
      lds_add(ukey, 4 * lanes, lk, lc, gk, gv, cap, overflow);
    }
  }
  __syncthreads();
  for (int i = tid; i < LDS_SLOTS; i += OV_THREADS)  // one global atomic per distinct pair and workgroup
    if (lk[i]) global_add(lk[i], lc[i], gk, gv, cap, overflow);
}

// Pass 1 over the slots: area[b][label] = sum of the label's row (column) of the table, background
// side included.
__global__ __launch_bounds__(256) void ap_area_kernel(const u64* __restrict__ keys, const int* __restrict__ vals,
                                                      long long nslots, int cap, int nt, int np,
                                                      int* __restrict__ areaT, int* __restrict__ areaP) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
    const u64 key = keys[s];
    if (key == 0) continue;
    const int b = (int)(s / cap);
    const int t = (int)(key >> 32), p = (int)(key & 0xffffffffULL);
    const int v = vals[s];
    if (v <= 0) continue;
    if (t > 0 && t < nt) atomicAdd(areaT + (size_t)b * nt + t, v);
    if (p > 0 && p < np) atomicAdd(areaP + (size_t)b * np + p, v);
  }
}

// grid (B, 2): nmax[b] = the highest label of image b with pixels, side y = 0 true, 1 predicted.  One
// workgroup scans the image's areas (a per-slot atomicMax would put every slot of an image on one word).
__global__ __launch_bounds__(256) void ap_nmax_kernel(const int* __restrict__ areaT, const int* __restrict__ areaP,
                                                      int nt, int np, int* __restrict__ ntrue,
                                                      int* __restrict__ npred) {
  __shared__ int top;
  if (threadIdx.x == 0) top = 0;
  __syncthreads();
  const int b = blockIdx.x;
  const int n = blockIdx.y ? np : nt;
  const int* __restrict__ area = blockIdx.y ? areaP + (size_t)b * np : areaT + (size_t)b * nt;
  int mine = 0;
  for (int l = threadIdx.x; l < n; l += blockDim.x)
    if (l > 0 && area[l] > 0) mine = l;  // ascending: the last hit is this thread's highest
  if (mine > 0) atomicMax(&top, mine);
  __syncthreads();
  if (threadIdx.x == 0) (blockIdx.y ? npred : ntrue)[b] = top;
}

// Pass 2: IoU of every foreground pair in fp64 (one IEEE division, as numpy's) against the
// ascending thresholds; level[s] = how many it passes.  deg* are [B, K, bound].
__global__ __launch_bounds__(256) void ap_match_kernel(const u64* __restrict__ keys, const int* __restrict__ vals,
                                                       long long nslots, int cap, int nt, int np,
                                                       const double* __restrict__ thr, int K,
                                                       const int* __restrict__ areaT, const int* __restrict__ areaP,
                                                       int* __restrict__ edges, int* __restrict__ conflict,
                                                       int* __restrict__ degT, int* __restrict__ degP,
                                                       int* __restrict__ level) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  // cap >= 64 (a power of two): the 64 consecutive slots of a wave lie in one image, so the wave adds
  // its edges to edges[b][k] with one atomic instead of one per lane on the same word
  const bool agg = (cap & 63) == 0;
  for (long long s0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); s0 < nslots; s0 += stride) {
    const long long s = s0 + lane;  // s0 is uniform over the wave: every lane reaches the ballots
    const int b = (int)(s / cap);
    int lvl = 0;
    const u64 key = s < nslots ? keys[s] : 0ULL;
    const int t = (int)(key >> 32), p = (int)(key & 0xffffffffULL);
    if (t > 0 && p > 0 && t < nt && p < np) {
      const long long ov = vals[s];
      const long long uni = (long long)areaT[(size_t)b * nt + t] + (long long)areaP[(size_t)b * np + p] - ov;
      if (ov > 0 && uni > 0) {
        const double iou = (double)ov / (double)uni;
        for (int k = 0; k < K && k < MAX_THR; ++k) {
          if (!(iou >= thr[k])) break;  // ascending: nothing above passes either
          ++lvl;
          if (!agg) atomicAdd(edges + b * MAX_THR + k, 1);
          const int dt = atomicAdd(degT + ((size_t)b * K + k) * nt + t, 1);
          const int dp = atomicAdd(degP + ((size_t)b * K + k) * np + p, 1);
          if (dt > 0 || dp > 0) atomicOr(conflict + b * MAX_THR + k, 1);
        }
        if (lvl) level[s] = lvl;
      }
    }
    if (agg) {
      const int bw = (int)(s0 / cap);
      for (int k = 0; k < K && k < MAX_THR; ++k) {
        const u64 m = __ballot(lvl > k);
        if (m == 0) break;  // uniform
        if (lane == __ffsll((long long)m) - 1) atomicAdd(edges + bw * MAX_THR + k, __popcll(m));
      }
    }
  }
}

}  // namespace

// T / P: [B, N] labels with bounds nt / np (largest label + 1).  keys / vals: [B, cap] zero-filled,
// cap a power of two; flags[0] is the overflow word, flags[1] the error word.
extern "C" int be_cp_ap_overlap(const int* T, const int* P, int B, int N, int nt, int np, unsigned long long* keys,
                                int* vals, int cap, int* flags, hipStream_t s) {
  if (B < 1 || N < 1) return 0;
  if (nt < 1 || np < 1) return (int)hipErrorInvalidValue;
  if (cap < 1 || (cap & (cap - 1))) return (int)hipErrorInvalidValue;
  if (B > 65535) return (int)hipErrorInvalidValue;
  const int chunks = (N + OV_SPAN - 1) / OV_SPAN;
  hipLaunchKernelGGL(ap_overlap_kernel, dim3(chunks, B), dim3(OV_THREADS), 0, s, T, P, N, nt, np, keys, vals, cap,
                     flags);
  return BE_CHECK_LAUNCH();
}

// thr: K <= 8 ascending doubles on the device.  Zero-filled outputs: areaT [B, nt], areaP [B, np],
// edges / conflict [B, 8], degT [B, K, nt], degP [B, K, np], ntrue / npred [B], level [B, cap].
extern "C" int be_cp_ap_match(const unsigned long long* keys, const int* vals, int B, int cap, int nt, int np,
                              const double* thr, int K, int* areaT, int* areaP, int* edges, int* conflict, int* degT,
                              int* degP, int* ntrue, int* npred, int* level, hipStream_t s) {
  if (B < 1) return 0;
  if (K < 1 || K > MAX_THR || nt < 1 || np < 1 || cap < 1) return (int)hipErrorInvalidValue;
  const long long nslots = (long long)B * cap;
  int blocks = (int)((nslots + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(ap_area_kernel, dim3(blocks), dim3(256), 0, s, keys, vals, nslots, cap, nt, np, areaT, areaP);
  hipLaunchKernelGGL(ap_nmax_kernel, dim3(B, 2), dim3(256), 0, s, areaT, areaP, nt, np, ntrue, npred);
  hipLaunchKernelGGL(ap_match_kernel, dim3(blocks), dim3(256), 0, s, keys, vals, nslots, cap, nt, np, thr, K, areaT,
                     areaP, edges, conflict, degT, degP, level);
  return BE_CHECK_LAUNCH();
}
