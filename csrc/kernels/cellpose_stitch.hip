// Cellpose z-stacks: stitch per-plane 2-D label images into volumetric labels (gfx950).
//
// Semantics: bioengine_worker_amd/cellpose/reference.py::stitch3d (the CPU oracle; the GPU tests
// compare exactly).  Four host entry points, queued back to back on one stream:
//
//   be_cp_stitch_overlap   all Z-1 adjacent plane pairs in ONE launch: sparse (b, a) -> common-pixel
//                          counts in a per-pair open-addressing hash table in global memory
//   be_cp_stitch_match     exact-IoU mutual-best matching over the occupied slots (4 small passes)
//   be_cp_stitch_number    global ids (one workgroup walks the planes), voxels per id, min_size ranks
//   be_cp_stitch_relabel   out[z][p] = lut[gid[z][M[z][p]]]
//
// Every loop is bounded: hash probing gives up after `capacity` probes (sets the overflow word and
// drops the increment; the caller re-runs the launch with a larger table), the compare-and-swap
// maxima only retry when another thread made progress, and no kernel waits on another workgroup.
// Integer atomics and total-order tie-breaks make the result independent of arrival order.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int OV_THREADS = 256;
constexpr int OV_ITERS = 8;                        // 256 lanes x 4 px x 8 = 8192 pixels per workgroup
constexpr int OV_SPAN = OV_THREADS * 4 * OV_ITERS;
constexpr int LDS_SLOTS = 1024;                    // 12 KiB: keys (8 B) + counts (4 B)
constexpr int LDS_PROBES = 16;
constexpr u64 NONUNI = ~0ULL;                      // lane whose 4 pixels do not share one key

__device__ __forceinline__ unsigned hash_key(u64 key) {
  unsigned h = (unsigned)(key >> 32) * 0x9E3779B1u ^ (unsigned)key * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0xC2B2AE3Du;
  h ^= h >> 13;
  return h;
}

// Bounded insert-or-add into pair `gk/gv` (capacity `cap`, a power of two; key 0 = empty slot).
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
  global_add(key, c, gk, gv, cap, overflow);  // crowded LDS table: straight to the pair's table
}

__device__ __forceinline__ u64 pair_key(int a, int b, int nlab) {
  return (a > 0 && b > 0 && a < nlab && b < nlab) ? ((u64)(unsigned)b << 32) | (unsigned)a : 0ULL;
}

// grid (chunks, Z-1): workgroup (x, y) counts pixels [x * OV_SPAN, +OV_SPAN) of planes y and y+1.
__global__ __launch_bounds__(OV_THREADS) void overlap_kernel(const int* __restrict__ M, int HW, int nlab,
                                                             u64* __restrict__ keys, int* __restrict__ vals, int cap,
                                                             int* __restrict__ overflow) {
  __shared__ u64 lk[LDS_SLOTS];
  __shared__ int lc[LDS_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < LDS_SLOTS; i += OV_THREADS) {
    lk[i] = 0;
    lc[i] = 0;
  }
  __syncthreads();
  const int pair = blockIdx.y;
  const int* __restrict__ Pa = M + (size_t)pair * HW;        // plane z-1
  const int* __restrict__ Pb = M + (size_t)(pair + 1) * HW;  // plane z
  u64* gk = keys + (size_t)pair * cap;
  int* gv = vals + (size_t)pair * cap;
  // 16-byte loads need both planes aligned (HW % 4 == 0 and an aligned base); otherwise scalar
  const bool aligned = ((((uintptr_t)Pa) | ((uintptr_t)Pb)) & 15) == 0;
  const long long base = (long long)blockIdx.x * OV_SPAN;
#pragma unroll 1
  for (int it = 0; it < OV_ITERS; ++it) {  // trip count is uniform: every lane reaches the shuffles
    const long long p = base + ((long long)it * OV_THREADS + tid) * 4;
    int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (p + 4 <= HW && aligned) {
      const int4 va = *reinterpret_cast<const int4*>(Pa + p);
      const int4 vb = *reinterpret_cast<const int4*>(Pb + p);
      a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
      b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p + i < HW) {
          a[i] = Pa[p + i];
          b[i] = Pb[p + i];
        }
    }
    u64 k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = pair_key(a[i], b[i], nlab);
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

// ---- matching ----------------------------------------------------------------------------------
// IoU = ov / u kept as the exact pair (ov << 32 | u); ov < 2^31 and u < 2^32, so the cross products
// fit 64 bits.
__device__ __forceinline__ bool ratio_gt(u64 x, u64 y) {  // x > y; y == 0 is "nothing yet"
  return y == 0 || (x >> 32) * (y & 0xffffffffULL) > (y >> 32) * (x & 0xffffffffULL);
}
__device__ __forceinline__ bool ratio_eq(u64 x, u64 y) {
  return y != 0 && (x >> 32) * (y & 0xffffffffULL) == (y >> 32) * (x & 0xffffffffULL);
}
__device__ __forceinline__ void ratio_max(u64* p, u64 x) {
  u64 old = *p;
  while (ratio_gt(x, old)) {  // retries only after another thread raised the slot: bounded
    const u64 seen = atomicCAS(p, old, x);
    if (seen == old) break;
    old = seen;
  }
}

// pass 0: bestA[z][a] = max IoU over the candidates of a;  pass 1: owner[z][a] = min b at that IoU;
// pass 2: bestB[z][b] = max IoU over the a that b owns;    pass 3: link[z][b] = min a at that IoU.
// owner / link hold ~label (0 = none) so that atomicMax is the minimum and zero-filling initialises.
__global__ __launch_bounds__(256) void match_kernel(const u64* __restrict__ keys, const int* __restrict__ vals,
                                                    long long nslots, int cap, const int* __restrict__ counts, int nlab,
                                                    double thr, u64* __restrict__ bestA, unsigned* __restrict__ owner,
                                                    u64* __restrict__ bestB, unsigned* __restrict__ link, int pass) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
    const u64 key = keys[s];
    if (key == 0) continue;
    const int z = (int)(s / cap) + 1;  // the pair's upper plane
    const int b = (int)(key >> 32), a = (int)(key & 0xffffffffULL);
    const unsigned ov = (unsigned)vals[s];
    const unsigned u = (unsigned)counts[(size_t)z * nlab + b] + (unsigned)counts[(size_t)(z - 1) * nlab + a] - ov;
    if (!(ov > 0 && (double)ov >= thr * (double)u)) continue;
    const u64 r = ((u64)ov << 32) | u;
    const size_t ia = (size_t)z * nlab + a, ib = (size_t)z * nlab + b;
    if (pass == 0) {
      ratio_max(bestA + ia, r);
    } else if (pass == 1) {
      if (ratio_eq(r, bestA[ia])) atomicMax(owner + ia, ~(unsigned)b);
    } else if (owner[ia] == ~(unsigned)b) {
      if (pass == 2)
        ratio_max(bestB + ib, r);
      else if (ratio_eq(r, bestB[ib]))
        atomicMax(link + ib, ~(unsigned)a);
    }
  }
}

// ---- numbering ---------------------------------------------------------------------------------
constexpr int NUM_THREADS = 1024;

// Exclusive prefix sum of one flag per thread over the workgroup; `total` is the workgroup's sum.
__device__ __forceinline__ int block_scan(int flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 m = __ballot(flag);
  const int before = __popcll(m & ((1ULL << lane) - 1));
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NUM_THREADS / 64; ++w) {
    const int v = wsum[w];
    off += w < wave ? v : 0;
    tot += v;
  }
  __syncthreads();  // wsum is reused by the next call
  total = tot;
  return off + before;
}

// One workgroup walks the planes: a linked label takes its link's id in plane z-1, every other
// label with pixels the next unused id in ascending label order.
__global__ __launch_bounds__(NUM_THREADS) void number_kernel(const int* __restrict__ counts,
                                                             const unsigned* __restrict__ link, int Z, int nlab,
                                                             int* __restrict__ gid) {
  __shared__ int wsum[NUM_THREADS / 64];
  int next = 0;  // ids handed out so far (uniform)
  for (int z = 0; z < Z; ++z) {
    const int* cz = counts + (size_t)z * nlab;
    int* gz = gid + (size_t)z * nlab;
    for (int l0 = 0; l0 < nlab; l0 += NUM_THREADS) {
      const int l = l0 + threadIdx.x;
      const bool exists = l > 0 && l < nlab && cz[l] > 0;
      const unsigned lk = (exists && z > 0) ? link[(size_t)z * nlab + l] : 0u;
      const bool fresh = exists && lk == 0;
      int total;
      const int rank = block_scan(fresh, wsum, total);
      if (l < nlab) gz[l] = fresh ? next + rank + 1 : (exists ? gid[(size_t)(z - 1) * nlab + (int)(~lk)] : 0);
      next += total;
    }
    __syncthreads();  // plane z+1 reads this plane's ids
  }
}

__global__ __launch_bounds__(256) void volume_kernel(const int* __restrict__ counts, const int* __restrict__ gid,
                                                     long long n, u64* __restrict__ vol) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = gid[i];
  if (g > 0) atomicAdd(vol + g, (u64)(unsigned)counts[i]);
}

// lut[g] = rank of instance g among those kept (all with voxels, and >= min_size if set), else 0.
__global__ __launch_bounds__(NUM_THREADS) void rank_kernel(const u64* __restrict__ vol, long long n, int min_size,
                                                           int* __restrict__ lut, int* __restrict__ kout) {
  __shared__ int wsum[NUM_THREADS / 64];
  int next = 0;
  for (long long g0 = 0; g0 < n; g0 += NUM_THREADS) {
    const long long g = g0 + threadIdx.x;
    const u64 v = (g > 0 && g < n) ? vol[g] : 0;
    const bool keep = v > 0 && (min_size <= 0 || v >= (u64)min_size);
    int total;
    const int rank = block_scan(keep, wsum, total);
    if (g < n) lut[g] = keep ? next + rank + 1 : 0;
    next += total;
  }
  if (threadIdx.x == 0) *kout = next;
}

// ---- relabel -----------------------------------------------------------------------------------
__device__ __forceinline__ int relabel_one(int m, long long z, int nlab, const int* __restrict__ gid,
                                           const int* __restrict__ lut) {
  return (m > 0 && m < nlab) ? lut[gid[z * nlab + m]] : 0;
}

__global__ __launch_bounds__(256) void relabel_kernel(const int* __restrict__ M, long long n, int HW, int nlab,
                                                      const int* __restrict__ gid, const int* __restrict__ lut,
                                                      int* __restrict__ out, int vec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nvec = vec ? n / 4 : 0;
  for (long long v = t; v < nvec; v += stride) {
    const long long p = v * 4;
    const int4 m = *reinterpret_cast<const int4*>(M + p);
    const long long z = p / HW;
    const long long left = (z + 1) * HW - p;  // pixels of plane z from p on: < 4 when the vector straddles
    int4 o;
    o.x = relabel_one(m.x, z, nlab, gid, lut);
    o.y = relabel_one(m.y, left > 1 ? z : (p + 1) / HW, nlab, gid, lut);
    o.z = relabel_one(m.z, left > 2 ? z : (p + 2) / HW, nlab, gid, lut);
    o.w = relabel_one(m.w, left > 3 ? z : (p + 3) / HW, nlab, gid, lut);
    *reinterpret_cast<int4*>(out + p) = o;
  }
  for (long long p = nvec * 4 + t; p < n; p += stride) out[p] = relabel_one(M[p], p / HW, nlab, gid, lut);
}

}  // namespace

// keys / vals: [Z-1, cap] zero-filled, cap a power of two; flags[0] is the overflow word.
extern "C" int be_cp_stitch_overlap(const int* M, int Z, int HW, int nlab, unsigned long long* keys, int* vals, int cap,
                                    int* flags, hipStream_t s) {
  if (Z < 2 || HW < 1 || nlab < 2) return 0;
  if (cap < 1 || (cap & (cap - 1))) return (int)hipErrorInvalidValue;
  if (Z - 1 > 65535) return (int)hipErrorInvalidValue;
  const int chunks = (HW + OV_SPAN - 1) / OV_SPAN;
  hipLaunchKernelGGL(overlap_kernel, dim3(chunks, Z - 1), dim3(OV_THREADS), 0, s, M, HW, nlab, keys, vals, cap, flags);
  return BE_CHECK_LAUNCH();
}

// counts [Z, nlab] pixels per label; bestA / bestB (64-bit) and owner / link (32-bit) [Z, nlab] zero-filled.
extern "C" int be_cp_stitch_match(const unsigned long long* keys, const int* vals, int Z, int cap, const int* counts,
                                  int nlab, double thr, unsigned long long* bestA, unsigned* owner,
                                  unsigned long long* bestB, unsigned* link, hipStream_t s) {
  if (Z < 2 || nlab < 2) return 0;
  const long long nslots = (long long)(Z - 1) * cap;
  int blocks = (int)((nslots + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  for (int pass = 0; pass < 4; ++pass)
    hipLaunchKernelGGL(match_kernel, dim3(blocks), dim3(256), 0, s, keys, vals, nslots, cap, counts, nlab, thr, bestA,
                       owner, bestB, link, pass);
  return BE_CHECK_LAUNCH();
}

// gid [Z, nlab]; vol (64-bit, zero-filled) and lut [Z * nlab + 1]; flags[1] receives K.
extern "C" int be_cp_stitch_number(const int* counts, const unsigned* link, int Z, int nlab, int min_size, int* gid,
                                   unsigned long long* vol, int* lut, int* flags, hipStream_t s) {
  if (Z < 1 || nlab < 1) return 0;
  const long long n = (long long)Z * nlab;
  hipLaunchKernelGGL(number_kernel, dim3(1), dim3(NUM_THREADS), 0, s, counts, link, Z, nlab, gid);
  hipLaunchKernelGGL(volume_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, counts, gid, n, vol);
  hipLaunchKernelGGL(rank_kernel, dim3(1), dim3(NUM_THREADS), 0, s, vol, n + 1, min_size, lut, flags + 1);
  return BE_CHECK_LAUNCH();
}

extern "C" int be_cp_stitch_relabel(const int* M, int Z, int HW, int nlab, const int* gid, const int* lut, int* out,
                                    hipStream_t s) {
  const long long n = (long long)Z * HW;
  if (n < 1) return 0;
  const int vec = ((((uintptr_t)M) | ((uintptr_t)out)) & 15) == 0;
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(relabel_kernel, dim3((unsigned)blocks), dim3(256), 0, s, M, n, HW, nlab, gid, lut, out, vec);
  return BE_CHECK_LAUNCH();
}
