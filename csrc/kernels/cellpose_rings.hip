// Cellpose: outlines of label images as closed rings of pixel-corner coordinates (gfx950).
//
// Semantics: bioengine_worker_amd/cellpose/reference.py::mask_rings (the CPU oracle; the GPU tests
// compare exactly).  Two host entry points; between them the Python wrapper reads V (the number of
// vertices) to size verts, after them R (the number of rings) and the error word:
//
//   be_cp_rings_count   init     boxes to (INT_MAX, -1, INT_MAX, -1), vertex counts to 0
//                       count    one pass over the (H + 1)(W + 1) pixel corners of every image: the
//                                number of turn vertices of a label is local (one or three members
//                                of the label in the corner's 2 x 2 block: 1 vertex; two diagonal
//                                members: 2), and so is its box.  A thread owns RL consecutive
//                                corners of a row and sends one atomic per run of equal labels
//                                (integer add / min / max: order independent, and they size
//                                buffers only).  One thread per corner with the votes collapsed
//                                per wave was measured too: 2.5 times slower (README).
//                       scan     one workgroup: exclusive prefix sums of nvert and of nvert / 4
//                                (a ring has at least four vertices) give every label its segment
//                                of verts and of the ring table; the totals go to totals[0..1].
//   be_cp_rings_trace   trace    ONE WAVE PER (image, label).  Its vertices go to
//                                verts[voff[job] + k] and its rings to the ring table at
//                                roff[job] + r, k and r counted by the one walking lane in ring
//                                order: no atomic decides an output position, so every array is
//                                bit-identical from run to run.
//                       scan     rings per label -> their prefix sum, R to totals[2]
//                       gather   one thread per label copies its rings from the table into the
//                                compact result arrays, ordered by (image, label, start);
//                                image_rings and the error word (totals[3]) come from here too.
//
// Which box takes which path.
//   * up to 64 x 64 pixels (every ordinary cell): the wave reads the box once (one coalesced row per
//     step, one ballot per row) into 64-bit membership words in LDS, counts the label's edges from
//     the words with popcounts, and lane 0 follows the cracks on LDS alone; the "top edge already
//     traced" marks are 64-bit words in LDS too.  No global load depends on a walk step.
//   * larger in either direction: the same walk, edge by edge, on the labels in global memory, with
//     the marks in a byte image `seen` (one byte per pixel, zeroed by the caller; a pixel belongs to
//     one label, so jobs never share a byte).  Right, not fast: a dependent L2 read per step.
// Ring starts are found by scanning the label's top edges (pixel in the label, pixel above not) in
// raster order and skipping marked ones: the first unmarked top edge is the raster-first top edge of
// a new ring, which is the oracle's canonical start and ring order.
//
// Bounded loops.  The walk consumes one directed edge per step and the wave has counted the label's
// edges beforehand, so all rings of a label together take exactly that many steps; the budget is
// the count plus one.  A walk that runs out of steps, vertices (nvert[job]) or ring slots
// (nvert[job] / 4: a ring has at least four turn vertices) stops, sets *err and the wrapper raises:
// labels that change under the kernel can never spin a wave or write outside a segment.
#include "common.h"

#include <limits.h>

namespace {

constexpr int RL = 16;  // corners per thread of the count kernel
constexpr int WPB = 4;  // waves (jobs) per workgroup of the trace kernel

enum { ERR_STEPS = 1, ERR_VERTS = 2, ERR_RINGS = 4, ERR_COUNT = 8 };

__global__ __launch_bounds__(256) void init_kernel(int* __restrict__ bbox, int* __restrict__ nvert, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * n) bbox[i] = (i & 1) ? -1 : INT_MAX;
  if (i < n) nvert[i] = 0;
}

// M [B, H, W]; labels outside 1..K are background.  bbox [B, K, 4] = (ymin, ymax, xmin, xmax) inclusive.
__global__ __launch_bounds__(256) void count_kernel(const int* __restrict__ M, int B, int H, int W, int K,
                                                    int* __restrict__ bbox, int* __restrict__ nvert) {
  const int segs = (W + 1 + RL - 1) / RL;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)B * (H + 1) * segs) return;
  const int seg = (int)(gid % segs);
  const long long row = gid / segs;  // b * (H + 1) + cy
  const int b = (int)(row / (H + 1)), cy = (int)(row % (H + 1));
  const int* Mb = M + (size_t)b * H * W;
  const int* up = cy > 0 ? Mb + (size_t)(cy - 1) * W : nullptr;
  const int* dn = cy < H ? Mb + (size_t)cy * W : nullptr;
  auto px = [&](const int* r, int x) {
    if (r == nullptr || x < 0 || x >= W) return 0;
    const int v = r[x];
    return (v > 0 && v <= K) ? v : 0;
  };
  int* nvb = nvert + (size_t)b * K;
  int vl = 0, vn = 0;  // vertices: one pending (label, count)
  auto add = [&](int lab, int n) {
    if (lab != vl) {
      if (vl > 0 && vn > 0) atomicAdd(nvb + vl - 1, vn);
      vl = lab;
      vn = 0;
    }
    vn += n;
  };
  int bl = 0, bs = 0;  // box: the current run of the lower row
  auto flush_box = [&](int lab, int xa, int xe) {
    if (lab <= 0) return;
    int* bb = bbox + ((size_t)b * K + lab - 1) * 4;
    if (cy < bb[0]) atomicMin(bb + 0, cy);  // a stale plain read can only ask for an unneeded atomic
    if (cy > bb[1]) atomicMax(bb + 1, cy);
    if (xa < bb[2]) atomicMin(bb + 2, xa);
    if (xe > bb[3]) atomicMax(bb + 3, xe);
  };
  const int x0 = seg * RL, x1 = min(x0 + RL, W + 1);
  int a = px(up, x0 - 1), c = px(dn, x0 - 1);
  for (int cx = x0; cx < x1; ++cx) {
    const int bq = px(up, cx), d = px(dn, cx);
    if (!(a == bq && c == d && a == c)) {
      auto vote = [&](int q, bool first) {  // every distinct positive label of the block once
        if (q <= 0 || !first) return;
        const int n = (q == a) + (q == bq) + (q == c) + (q == d);
        if (n == 1 || n == 3) add(q, 1);
        else if (n == 2 && ((q == a && q == d) || (q == bq && q == c))) add(q, 2);
      };
      vote(a, true);
      vote(bq, bq != a);
      vote(c, c != a && c != bq);
      vote(d, d != a && d != bq && d != c);
    }
    if (cx < W && d != bl) {
      flush_box(bl, bs, cx - 1);
      bl = d;
      bs = cx;
    }
    a = bq;
    c = d;
  }
  flush_box(bl, bs, min(x1, W) - 1);
  if (vl > 0 && vn > 0) atomicAdd(nvb + vl - 1, vn);
}

// Exclusive prefix sums of in[0..n) (-> out_a) and of in[i] / 4 (-> out_b, may be null) by ONE
// workgroup, 1024 items per step; the totals go to tot_a / tot_b.  Labels are few (thousands): one
// or a few steps.
__global__ __launch_bounds__(1024) void scan_kernel(const int* __restrict__ in, long long n, long long* __restrict__ out_a,
                                                    long long* __restrict__ out_b, long long* __restrict__ tot_a,
                                                    long long* __restrict__ tot_b) {
  __shared__ long long s_a[16], s_b[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long ca = 0, cb = 0;  // carried totals, the same in every thread
  for (long long base = 0; base < n; base += 1024) {
    const long long i = base + tid;
    const long long va = i < n ? in[i] : 0, vb = va / 4;
    long long a = va, b = vb;  // inclusive scans inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long ta = __shfl_up(a, o, 64), tb = __shfl_up(b, o, 64);
      if (lane >= o) a += ta, b += tb;
    }
    if (lane == 63) s_a[wv] = a, s_b[wv] = b;
    __syncthreads();
    long long pa = 0, pb = 0, ta = 0, tb = 0;
    for (int k = 0; k < 16; ++k) {
      if (k < wv) pa += s_a[k], pb += s_b[k];
      ta += s_a[k], tb += s_b[k];
    }
    if (i < n) {
      out_a[i] = ca + pa + a - va;
      if (out_b) out_b[i] = cb + pb + b - vb;
    }
    ca += ta, cb += tb;
    __syncthreads();
  }
  if (tid == 0) {
    *tot_a = ca;
    if (tot_b) *tot_b = cb;
  }
}

// ---- membership and marks: LDS words (boxes up to 64 x 64) or global memory -------------------------

struct LdsIn {
  const unsigned long long* rows;  // rows[r + 1] = box row r, bit c = column x0 + c; rows[0] = rows[65] = 0
  int y0, x0;
  __device__ __forceinline__ bool operator()(int y, int x) const {
    const int r = y - y0 + 1, c = x - x0;
    if ((unsigned)r > 65u || (unsigned)c > 63u) return false;
    return (rows[r] >> c) & 1ull;
  }
};
struct LdsSeen {
  unsigned long long* w;  // one word per box row
  int y0, x0;
  __device__ __forceinline__ bool get(int y, int x) const { return (w[y - y0] >> (x - x0)) & 1ull; }
  __device__ __forceinline__ void set(int y, int x) const { w[y - y0] |= 1ull << (x - x0); }
};
struct GlobalIn {
  const int* Mb;
  int H, W, lab;
  __device__ __forceinline__ bool operator()(int y, int x) const {
    return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && Mb[(size_t)y * W + x] == lab;
  }
};
struct GlobalSeen {
  unsigned char* p;
  int W;
  __device__ __forceinline__ bool get(int y, int x) const { return p[(size_t)y * W + x] != 0; }
  __device__ __forceinline__ void set(int y, int x) const { p[(size_t)y * W + x] = 1; }
};

struct Walk {
  int2* vout;         // the label's segment of verts
  int nv, k;          // its size, vertices written
  long long steps;    // edges left in the label's budget
  int err;
};

// One ring from its raster-first top edge, the top edge of pixel (sy, sx).  Directions: 0 = +x (top
// edge), 1 = +y (right), 2 = -x (bottom), 3 = -y (left); the label is on the right hand.
template <class In, class Seen>
__device__ bool walk_ring(const In& in, const Seen& seen, int sy, int sx, Walk& w, long long& area2) {
  if (w.k >= w.nv) {
    w.err |= ERR_VERTS;
    return false;
  }
  w.vout[w.k++] = make_int2(sy, sx);
  int py = sy, px = sx, d = 0;
  long long a2 = 0;
  for (;;) {
    if (w.steps-- <= 0) {
      w.err |= ERR_STEPS;
      return false;
    }
    if (d == 0) seen.set(py, px);
    const int dy = (d == 1) - (d == 3), dx = (d == 0) - (d == 2);
    const int ty = py + (d >= 2), tx = px + (d == 1 || d == 2);  // the edge's tail
    a2 += (long long)tx * dy - (long long)dx * ty;                 // x * y' - x' * y of a unit edge
    const int ay = py + dy, ax = px + dx;
    int nd = d;
    if (!in(ay, ax)) {
      nd = (d + 1) & 3;
    } else {
      const int l = (d + 3) & 3;
      const int by = ay + (l == 1) - (l == 3), bx = ax + (l == 0) - (l == 2);
      if (in(by, bx)) {
        py = by, px = bx, nd = l;
      } else {
        py = ay, px = ax;
      }
    }
    if (py == sy && px == sx && nd == 0) break;
    if (nd != d) {
      if (w.k >= w.nv) {
        w.err |= ERR_VERTS;
        return false;
      }
      w.vout[w.k++] = make_int2(py + (nd >= 2), px + (nd == 1 || nd == 2));
    }
    d = nd;
  }
  area2 = a2;
  return true;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * WPB) void trace_kernel(const int* __restrict__ M, int B, int H, int W, int K,
                                                         const int* __restrict__ bbox, const int* __restrict__ nvert,
                                                         const long long* __restrict__ voff,
                                                         const long long* __restrict__ roff, unsigned char* seen,
                                                         int2* __restrict__ verts, long long* __restrict__ ring_first,
                                                         long long* __restrict__ ring_area2, int* __restrict__ nrings,
                                                         int* __restrict__ err) {
  __shared__ unsigned long long s_rows[WPB][66];
  __shared__ unsigned long long s_seen[WPB][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long job = (long long)blockIdx.x * WPB + wv;
  if (job >= (long long)B * K) return;  // whole waves leave; the kernel has no workgroup barrier
  const int b = (int)(job / K), lab = (int)(job % K) + 1;
  const int* bb = bbox + job * 4;
  const int y0 = bb[0], y1 = bb[1], x0 = bb[2], x1 = bb[3];
  const int nv = nvert[job];
  if (y1 < y0 || y0 < 0 || x0 < 0 || y1 >= H || x1 >= W || x1 < x0) {  // a label without pixels
    if (lane == 0) {
      nrings[job] = 0;
      if (nv != 0) atomicOr(err, ERR_COUNT);
    }
    return;
  }
  const int ly = y1 - y0 + 1, lx = x1 - x0 + 1;
  const int* Mb = M + (size_t)b * H * W;
  const long long r0 = roff[job];
  const int rcap = nv / 4;
  Walk w;
  w.vout = verts + voff[job];
  w.nv = nv;
  w.k = 0;
  w.err = 0;
  int nr = 0;
  auto ring = [&](auto& in, auto& sn, int sy, int sx) {  // lane 0 only
    if (nr >= rcap) {
      w.err |= ERR_RINGS;
      return;
    }
    const int kf = w.k;
    long long a2 = 0;
    if (!walk_ring(in, sn, sy, sx, w, a2)) return;
    ring_first[r0 + nr] = voff[job] + kf;
    ring_area2[r0 + nr] = a2;
    ++nr;
  };
  if (ly <= 64 && lx <= 64) {
    unsigned long long* rows = s_rows[wv];
    unsigned long long mine = 0;
    for (int r0 = 0; r0 < ly; r0 += 8) {  // eight row loads in flight, then their ballots
      int v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (r0 + j < ly && lane < lx) ? Mb[(size_t)(y0 + r0 + j) * W + x0 + lane] : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned long long word = __ballot(v[j] == lab);
        if (lane == r0 + j) mine = word;
      }
    }
    rows[lane + 1] = mine;
    if (lane == 0) rows[0] = 0;
    if (lane == 1) rows[65] = 0;
    s_seen[wv][lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned long long upw = rows[lane], dnw = rows[lane + 2];
    const long long e = __popcll(mine & ~upw) + __popcll(mine & ~dnw) + __popcll(mine & ~(mine << 1)) +
                        __popcll(mine & ~(mine >> 1));
    w.steps = wave_sum_ll(e) + 1;
    if (lane == 0) {
      LdsIn in{rows, y0, x0};
      LdsSeen sn{s_seen[wv], y0, x0};
      for (int r = 0; r < ly && !w.err; ++r) {
        const unsigned long long top = rows[r + 1] & ~rows[r];
        for (;;) {
          const unsigned long long cand = top & ~s_seen[wv][r];
          if (!cand || w.err) break;
          ring(in, sn, y0 + r, x0 + __builtin_ctzll(cand));  // marks its start first: the scan advances
        }
      }
    }
  } else {
    GlobalIn in{Mb, H, W, lab};
    GlobalSeen sn{seen + (size_t)b * H * W, W};
    long long e = 0;
    for (int r = 0; r < ly; ++r)
      for (int c = lane; c < lx; c += 64) {
        const int y = y0 + r, x = x0 + c;
        if (in(y, x)) e += !in(y - 1, x) + !in(y + 1, x) + !in(y, x - 1) + !in(y, x + 1);
      }
    w.steps = wave_sum_ll(e) + 1;
    for (int r = 0; r < ly; ++r)
      for (int c0 = 0; c0 < lx; c0 += 64) {
        const int y = y0 + r, x = x0 + c0 + lane;
        unsigned long long top = __ballot(c0 + lane < lx && in(y, x) && !in(y - 1, x));
        if (lane == 0)
          for (; top && !w.err; top &= top - 1) {
            const int sx = x0 + c0 + __builtin_ctzll(top);
            if (!sn.get(y, sx)) ring(in, sn, y, sx);
          }
      }
  }
  if (lane == 0) {
    if (!w.err && w.k != nv) w.err |= ERR_COUNT;
    nrings[job] = w.err ? 0 : nr;
    if (w.err) atomicOr(err, w.err);
  }
}

// One thread per (image, label): its rings from the table to the compact arrays.  Thread b <= B also
// writes image_rings[b]; thread 0 closes ring_offsets and hands the error word to the host's read.
__global__ __launch_bounds__(256) void gather_kernel(long long n, int B, int K, const int* __restrict__ nvert,
                                                     const int* __restrict__ nrings, const long long* __restrict__ roff,
                                                     const long long* __restrict__ rstart,
                                                     const long long* __restrict__ ring_first,
                                                     const long long* __restrict__ ring_area2, const int* __restrict__ err,
                                                     long long* __restrict__ totals, long long* __restrict__ out_off,
                                                     long long* __restrict__ out_area2, int* __restrict__ out_label,
                                                     int* __restrict__ out_image, long long* __restrict__ image_rings) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long R = totals[2];
  if (j == 0) {
    out_off[R] = totals[0];
    totals[3] = *err;
  }
  if (j <= B) image_rings[j] = j < B ? rstart[j * K] : R;
  if (j >= n) return;
  const int nr = min(nrings[j], nvert[j] / 4);  // never beyond the label's slots
  const long long src = roff[j], dst = rstart[j];
  for (int r = 0; r < nr; ++r) {
    out_off[dst + r] = ring_first[src + r];
    out_area2[dst + r] = ring_area2[src + r];
    out_label[dst + r] = (int)(j % K) + 1;
    out_image[dst + r] = (int)(j / K);
  }
}

}  // namespace

extern "C" {

// bbox [B, K, 4], nvert [B, K], voff / roff [B, K] and totals[0..1] (V and the ring table's size) are
// written here; nothing needs initialising by the caller.
int be_cp_rings_count(const int* M, int B, int H, int W, int K, int* bbox, int* nvert, long long* voff, long long* roff,
                      long long* totals, hipStream_t s) {
  const long long n = (long long)B * K;
  if (n == 0 || H == 0 || W == 0) return 0;
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, s, bbox, nvert, n);
  const long long t = (long long)B * (H + 1) * ((W + 1 + RL - 1) / RL);
  hipLaunchKernelGGL(count_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, M, B, H, W, K, bbox, nvert);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, nvert, n, voff, roff, totals, totals + 1);
  return BE_CHECK_LAUNCH();
}

// seen [B, H, W] bytes and err (one int), both zeroed by the caller.  verts [V, 2] int32 (y, x);
// ring_first / ring_area2 [V / 4]: the ring table; nrings / rstart [B, K].  Results, each with room
// for V / 4 rings: out_off [V / 4 + 1], out_area2, out_label, out_image; image_rings [B + 1];
// totals[2] = R, totals[3] = the error word.
int be_cp_rings_trace(const int* M, int B, int H, int W, int K, const int* bbox, const int* nvert, const long long* voff,
                      const long long* roff, unsigned char* seen, int* verts, long long* ring_first, long long* ring_area2,
                      int* nrings, long long* rstart, int* err, long long* totals, long long* out_off, long long* out_area2,
                      int* out_label, int* out_image, long long* image_rings, hipStream_t s) {
  const long long n = (long long)B * K;
  if (n == 0) return 0;
  hipLaunchKernelGGL(trace_kernel, dim3((unsigned)((n + WPB - 1) / WPB)), dim3(64 * WPB), 0, s, M, B, H, W, K, bbox, nvert,
                     voff, roff, seen, reinterpret_cast<int2*>(verts), ring_first, ring_area2, nrings, err);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, nrings, n, rstart, (long long*)nullptr, totals + 2,
                     (long long*)nullptr);
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, n, B, K, nvert, nrings, roff, rstart,
                     ring_first, ring_area2, err, totals, out_off, out_area2, out_label, out_image, image_rings);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
