// Label volumes to surfaces: per-label quad meshes, surface-net vertices and surface statistics (gfx950).
//
// Semantics: bioengine_worker_amd/cellpose/reference.py::label_surface / surface_stats (the CPU oracle;
// the GPU tests compare exactly).  L is [Z, H, W] int32; corners live on the (Z+1, H+1, W+1) lattice
// and are addressed by their raster index c < 2^31 (the caller checks).  Thread t of tile T owns corner
// 256 T + t: its vertices (one per distinct label among the 8 voxels around it that holds fewer than 8
// of them, in label order) and the quads of the voxel whose low corner it is (all six sides, in side
// order 2a + s), so raster order of the corners is (voxel raster, side) order of the quads.
//
//   be_surf_count   per tile: vertex and quad totals (no per-corner array is ever written)
//   (host)          prefix sum over the tiles; reads V and F
//   be_surf_emit    recounts, scans inside the workgroup and writes the (corner, label) key of every
//                   vertex and the (corner, side, label) key of every quad at tile offset + rank: no
//                   atomic chooses a position.  Every write is bounded by the counted totals; a tile
//                   whose recount differs (labels changed under the kernel) sets the error word
//   (host)          stable sort of the label keys -> (label, raster) order and its permutation
//   be_surf_gather  label offsets from the sorted labels; vertices (corner, surface-net position,
//                   sorted corner key)
//   be_surf_remap   quads: the four (corner, label) keys are looked up by binary search in the
//                   label's sorted corner keys
//   be_surf_faces   per label: quads per axis and the voxel count from the x-axis quads (int64; block
//                   partials added with integer atomics, which are order independent)
//   be_surf_stats   per label: area and signed volume of the scaled surface-net mesh in fp64.  SL
//                   workgroups per label walk its quads in fixed chunks, reduce in a fixed tree and
//                   store partials; one thread per label adds them in slice order: no float atomic,
//                   bit-identical from run to run
#include "common.h"

namespace {

constexpr int TILE = 256;  // corners per workgroup
constexpr int SL = 8;      // workgroups per label of the statistics kernels

enum { ERR_EMIT = 1, ERR_KEY = 2, ERR_LOOKUP = 4 };

struct Dims {
  int Z, H, W, K;
};

__device__ __forceinline__ int voxel(const int* __restrict__ L, const Dims& d, int z, int y, int x) {
  const bool in = z >= 0 && z < d.Z && y >= 0 && y < d.H && x >= 0 && x < d.W;
  return in ? L[((size_t)z * d.H + y) * d.W + x] : 0;
}

// the 8 voxels around corner (cz, cy, cx), index 4 dz + 2 dy + dx, d = 0 the voxel below the corner
__device__ __forceinline__ void around(const int* __restrict__ L, const Dims& d, int cz, int cy, int cx, int v[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = voxel(L, d, cz - 1 + (i >> 2), cy - 1 + ((i >> 1) & 1), cx - 1 + (i & 1));
}

struct CornerWork {
  int nv;        // vertices of the corner
  int first;     // bit i: v[i] is the first occurrence of a label that gets a vertex
  int rank[8];   // for those: its rank among the corner's sorted distinct labels
  int own;       // label of the voxel whose low corner this is (0: none to mesh)
  int faces;     // bit 2a + s: that voxel owns a quad on the side
};

__device__ __forceinline__ void corner_work(const int* __restrict__ L, const Dims& d, long long c, long long NC, int v[8],
                                            int& cz, int& cy, int& cx, CornerWork& w) {
  w.nv = 0;
  w.first = 0;
  w.own = 0;
  w.faces = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) w.rank[i] = 0;
  cz = cy = cx = 0;
  if (c >= NC) return;
  const int W1 = d.W + 1, H1 = d.H + 1;
  cx = (int)(c % W1);
  const long long r = c / W1;
  cy = (int)(r % H1);
  cz = (int)(r / H1);
  around(L, d, cz, cy, cx, v);
  bool same = true;
#pragma unroll
  for (int i = 1; i < 8; ++i) same = same && v[i] == v[0];
  if (!same) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      bool f = v[i] >= 1 && v[i] <= d.K;
#pragma unroll
      for (int j = 0; j < i; ++j) f = f && v[j] != v[i];
      if (f) w.first |= 1 << i;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int rk = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) rk += (j != i && ((w.first >> j) & 1) && v[j] < v[i]) ? 1 : 0;
      w.rank[i] = rk;
    }
    w.nv = __popc(w.first);
  }
  if (cz < d.Z && cy < d.H && cx < d.W) {
    const int own = v[7];
    if (own >= 1 && own <= d.K) {
      w.own = own;
      const int nb[6] = {v[3], voxel(L, d, cz + 1, cy, cx), v[5], voxel(L, d, cz, cy + 1, cx),
                         v[6], voxel(L, d, cz, cy, cx + 1)};
#pragma unroll
      for (int s = 0; s < 6; ++s) w.faces |= (nb[s] != own) ? (1 << s) : 0;
    }
  }
}

// inclusive scan of a packed pair (vertices low 16 bits, quads high 16 bits: at most 2048 and 1536 per
// tile) over the 256 threads of the workgroup; `total` is the workgroup's sum
__device__ __forceinline__ int block_scan_packed(int x, int& total) {
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int s = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(s, o, 64);
    if (lane >= o) s += t;
  }
  if (lane == 63) wsum[wv] = s;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) base += k < wv ? wsum[k] : 0;
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return s + base;
}

__global__ __launch_bounds__(TILE) void count_kernel(const int* __restrict__ L, Dims d, long long NC,
                                                     int* __restrict__ tile_cnt) {
  const long long c = (long long)blockIdx.x * TILE + threadIdx.x;
  int v[8], cz, cy, cx;
  CornerWork w;
  corner_work(L, d, c, NC, v, cz, cy, cx, w);
  int total;
  block_scan_packed(w.nv | (__popc(w.faces) << 16), total);
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x] = total & 0xffff;
    tile_cnt[(size_t)gridDim.x + blockIdx.x] = total >> 16;
  }
}

// tile_inc [2, NT] int64: inclusive prefix sums of the rows of tile_cnt
__global__ __launch_bounds__(TILE) void emit_kernel(const int* __restrict__ L, Dims d, long long NC,
                                                    const long long* __restrict__ tile_inc, long long V, long long F,
                                                    int* __restrict__ vcorner, int* __restrict__ vlabel,
                                                    int* __restrict__ qcorner, unsigned char* __restrict__ qside,
                                                    int* __restrict__ qlabel, int* __restrict__ err) {
  const long long c = (long long)blockIdx.x * TILE + threadIdx.x;
  int v[8], cz, cy, cx;
  CornerWork w;
  corner_work(L, d, c, NC, v, cz, cy, cx, w);
  const int mine = w.nv | (__popc(w.faces) << 16);
  int total;
  const int incl = block_scan_packed(mine, total);
  const int excl = incl - mine;
  const long long* __restrict__ vinc = tile_inc;
  const long long* __restrict__ qinc = tile_inc + gridDim.x;
  const long long v0 = blockIdx.x ? vinc[blockIdx.x - 1] : 0, q0 = blockIdx.x ? qinc[blockIdx.x - 1] : 0;
  const long long v1 = min(vinc[blockIdx.x], V), q1 = min(qinc[blockIdx.x], F);
  bool bad = false;
  if (threadIdx.x == 0) bad = v0 + (total & 0xffff) != v1 || q0 + (total >> 16) != q1;
  const long long vb = v0 + (excl & 0xffff), qb = q0 + (excl >> 16);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if ((w.first >> i) & 1) {
      const long long p = vb + w.rank[i];
      if (p >= v0 && p < v1) {
        vcorner[p] = (int)c;
        vlabel[p] = v[i];
      } else {
        bad = true;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    if ((w.faces >> s) & 1) {
      const long long p = qb + __popc(w.faces & ((1 << s) - 1));
      if (p >= q0 && p < q1) {
        qcorner[p] = (int)c;
        qside[p] = (unsigned char)s;
        qlabel[p] = w.own;
      } else {
        bad = true;
      }
    }
  }
  if (bad) atomicOr(err, ERR_EMIT);
}

// lab [n] sorted labels -> off [K + 1]: off[j] = number of entries with a label <= j
__global__ __launch_bounds__(256) void offsets_kernel(const int* __restrict__ lab, long long n, int K,
                                                      long long* __restrict__ off) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = i ? min(max(lab[i - 1], 0), K) : 0;
  const int cur = min(max(lab[i], 0), K);
  for (int j = p; j < cur; ++j) off[j] = i;
  if (i == n - 1)
    for (int j = cur; j <= K; ++j) off[j] = n;
}

__global__ __launch_bounds__(256) void verts_kernel(const int* __restrict__ L, Dims d, long long NC, long long V,
                                                    const long long* __restrict__ perm, const int* __restrict__ vcorner,
                                                    const int* __restrict__ vlab, int* __restrict__ corner,
                                                    float* __restrict__ verts, int* __restrict__ vkey,
                                                    int* __restrict__ err) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const long long src = perm[i];
  const int l = vlab[i];
  long long c = (src >= 0 && src < V) ? vcorner[src] : -1;
  bool bad = c < 0 || c >= NC;
  if (bad) c = 0;
  const int W1 = d.W + 1, H1 = d.H + 1;
  const int cx = (int)(c % W1);
  const long long r = c / W1;
  const int cy = (int)(r % H1), cz = (int)(r / H1);
  int v[8];
  around(L, d, cz, cy, cx, v);
  // surface nets: the 12 edges of the 2 x 2 x 2 block of voxel centres; an edge crosses when exactly
  // one end carries l; its midpoint is 0 along its own axis and -+1 half voxels along the other two
  int ns[3] = {0, 0, 0}, nc = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int bit = 4 >> a;  // index bit of axis a (z: 4, y: 2, x: 1)
#pragma unroll
    for (int i8 = 0; i8 < 8; ++i8) {
      if (i8 & bit) continue;
      const bool cross = (v[i8] == l) != (v[i8 | bit] == l);
      if (cross) {
        ++nc;
#pragma unroll
        for (int o = 0; o < 3; ++o) {
          const int ob = 4 >> o;
          if (o != a) ns[o] += (i8 & ob) ? 1 : -1;
        }
      }
    }
  }
  bad = bad || nc == 0;
  const int cc[3] = {cz, cy, cx};
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    corner[i * 3 + o] = cc[o];
    const double q = nc ? (double)ns[o] / (double)(2 * nc) : 0.0;
    verts[i * 3 + o] = (float)((double)cc[o] + q);
  }
  vkey[i] = (int)c;
  if (bad) atomicOr(err, ERR_KEY);
}

__global__ __launch_bounds__(256) void quads_kernel(Dims d, long long NC, long long V, long long F,
                                                    const long long* __restrict__ perm, const int* __restrict__ qcorner,
                                                    const unsigned char* __restrict__ qside, const int* __restrict__ qlab,
                                                    const long long* __restrict__ label_verts, const int* __restrict__ vkey,
                                                    int4* __restrict__ quads, int* __restrict__ err) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F) return;
  const long long src = perm[i];
  const int l = qlab[i];
  long long c = -1;
  int side = 0;
  if (src >= 0 && src < F) {
    c = qcorner[src];
    side = qside[src];
  }
  const int W1 = d.W + 1, H1 = d.H + 1;
  bool bad = c < 0 || c >= NC || side > 5 || l < 1 || l > d.K;
  int out[4] = {0, 0, 0, 0};
  if (!bad) {
    int p[3];
    p[2] = (int)(c % W1);
    const long long r = c / W1;
    p[1] = (int)(r % H1);
    p[0] = (int)(r / H1);
    bad = p[0] >= d.Z || p[1] >= d.H || p[2] >= d.W;
    const int a = side >> 1, s = side & 1;
    const int b = a == 2 ? 0 : a + 1, cax = b == 2 ? 0 : b + 1;
    const long long lo0 = min(max(label_verts[l - 1], 0LL), V), hi0 = min(max(label_verts[l], lo0), V);
    auto stride = [&](int ax) -> long long { return ax == 0 ? (long long)H1 * W1 : (ax == 1 ? W1 : 1); };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // (b, c) offsets (0,0),(1,0),(1,1),(0,1) on the high side, (0,0),(0,1),(1,1),(1,0) on the low side
      const int o1 = (k == 1 || k == 2) ? 1 : 0, o2 = (k == 2 || k == 3) ? 1 : 0;
      const int ob = s ? o1 : o2, oc = s ? o2 : o1;
      const long long key = c + s * stride(a) + ob * stride(b) + oc * stride(cax);
      long long lo = lo0, hi = hi0;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (vkey[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < hi0 && vkey[lo] == key) out[k] = (int)lo; else bad = true;
    }
  }
  quads[i] = make_int4(out[0], out[1], out[2], out[3]);
  if (bad) atomicOr(err, ERR_LOOKUP);
}

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// grid (K, SL).  faces [K, 3], voxels [K] zeroed by the caller
__global__ __launch_bounds__(256) void faces_kernel(Dims d, long long NC, long long F, const long long* __restrict__ perm,
                                                    const int* __restrict__ qcorner, const unsigned char* __restrict__ qside,
                                                    const long long* __restrict__ label_quads,
                                                    unsigned long long* __restrict__ faces,
                                                    unsigned long long* __restrict__ voxels) {
  __shared__ long long sh[256];
  const int l = blockIdx.x;
  const long long q0 = min(max(label_quads[l], 0LL), F), q1 = min(max(label_quads[l + 1], q0), F);
  if (q0 + (long long)blockIdx.y * 256 >= q1) return;  // workgroup-uniform
  long long f[3] = {0, 0, 0}, vox = 0;
  for (long long q = q0 + (long long)blockIdx.y * 256 + threadIdx.x; q < q1; q += (long long)SL * 256) {
    const long long src = perm[q];
    if (src < 0 || src >= F) continue;
    const int side = qside[src];
    const long long c = qcorner[src];
    const int a = side >> 1, s = side & 1;
    f[0] += a == 0;
    f[1] += a == 1;
    f[2] += a == 2;
    if (a == 2 && c >= 0 && c < NC) {
      const long long plane = c % (d.W + 1) + s;
      vox += s ? plane : -plane;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const long long t = block_sum(f[a], sh);
    if (threadIdx.x == 0 && t) atomicAdd(faces + (size_t)l * 3 + a, (unsigned long long)t);
  }
  const long long t = block_sum(vox, sh);
  if (threadIdx.x == 0 && t) atomicAdd(voxels + l, (unsigned long long)t);
}

// grid (K, SL): part [K, SL, 2] = (area, signed volume) of the slice's quads of the scaled mesh
__global__ __launch_bounds__(256) void stats_kernel(long long V, long long F, const float* __restrict__ verts,
                                                    const int4* __restrict__ quads,
                                                    const long long* __restrict__ label_quads, double sz, double sy,
                                                    double sx, double* __restrict__ part) {
  __shared__ double sh[256];
  const int l = blockIdx.x;
  const long long q0 = min(max(label_quads[l], 0LL), F), q1 = min(max(label_quads[l + 1], q0), F);
  double area = 0.0, vol = 0.0;
  const double sp[3] = {sz, sy, sx};
  for (long long q = q0 + (long long)blockIdx.y * 256 + threadIdx.x; q < q1; q += (long long)SL * 256) {
    const int4 qd = quads[q];
    const int idx[4] = {qd.x, qd.y, qd.z, qd.w};
    double p[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long vi = min(max((long long)idx[k], 0LL), V - 1);
#pragma unroll
      for (int o = 0; o < 3; ++o) p[k][o] = (double)verts[vi * 3 + o] * sp[o];
    }
    double e[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int o = 0; o < 3; ++o) e[k][o] = p[k + 1][o] - p[0][o];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const double* u = e[t];
      const double* w = e[t + 1];
      const double n0 = u[1] * w[2] - u[2] * w[1], n1 = u[2] * w[0] - u[0] * w[2], n2 = u[0] * w[1] - u[1] * w[0];
      area += 0.5 * sqrt(n0 * n0 + n1 * n1 + n2 * n2);
      vol += (p[0][0] * n0 + p[0][1] * n1 + p[0][2] * n2) / 6.0;
    }
  }
  const double a = block_sum(area, sh);
  const double v = block_sum(vol, sh);
  if (threadIdx.x == 0) {
    part[((size_t)l * SL + blockIdx.y) * 2] = a;
    part[((size_t)l * SL + blockIdx.y) * 2 + 1] = v;
  }
}

__global__ __launch_bounds__(256) void stats_combine_kernel(int K, const double* __restrict__ part,
                                                            double* __restrict__ out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= K) return;
  double a = 0.0, v = 0.0;
  for (int s = 0; s < SL; ++s) {
    a += part[((size_t)l * SL + s) * 2];
    v += part[((size_t)l * SL + s) * 2 + 1];
  }
  out[(size_t)l * 2] = a;
  out[(size_t)l * 2 + 1] = v;
}

bool dims_ok(int Z, int H, int W, int K, long long& NC) {
  if (Z <= 0 || H <= 0 || W <= 0 || K <= 0) return false;
  if (Z > (1 << 15) || H > (1 << 15) || W > (1 << 15)) return false;
  NC = (long long)(Z + 1) * (H + 1) * (W + 1);
  return NC < (1LL << 31);
}

unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

// L [Z, H, W] int32, labels 1..K are meshed.  tile_cnt [2, NT] int32, NT = ceil((Z+1)(H+1)(W+1) / 256):
// vertices (row 0) and quads (row 1) of every tile of 256 corners (every element written).
int be_surf_count(const int* L, int Z, int H, int W, int K, int* tile_cnt, hipStream_t s) {
  long long NC;
  if (!dims_ok(Z, H, W, K, NC)) return (int)hipErrorInvalidValue;
  const Dims d{Z, H, W, K};
  hipLaunchKernelGGL(count_kernel, dim3(blocks(NC, TILE)), dim3(TILE), 0, s, L, d, NC, tile_cnt);
  return BE_CHECK_LAUNCH();
}

// tile_inc [2, NT] int64: inclusive prefix sums along the rows of tile_cnt; V, F: its last column.  Writes the keys of
// the V vertices (vcorner, vlabel) and F quads (qcorner, qside, qlabel) in (corner raster, label) /
// (voxel raster, side) order; err (zeroed by the caller) gets ERR_EMIT when a tile's recount differs.
int be_surf_emit(const int* L, int Z, int H, int W, int K, const long long* tile_inc, long long V, long long F,
                 int* vcorner, int* vlabel, int* qcorner, unsigned char* qside, int* qlabel, int* err, hipStream_t s) {
  long long NC;
  if (!dims_ok(Z, H, W, K, NC) || V < 0 || F < 0 || V >= (1LL << 31) || F >= (1LL << 31)) return (int)hipErrorInvalidValue;
  const Dims d{Z, H, W, K};
  hipLaunchKernelGGL(emit_kernel, dim3(blocks(NC, TILE)), dim3(TILE), 0, s, L, d, NC, tile_inc, V, F, vcorner, vlabel,
                     qcorner, qside, qlabel, err);
  return BE_CHECK_LAUNCH();
}

// vlab [V] / qlab [F]: the label keys sorted (stable), vperm / qperm [V] / [F] int64: the sort's
// permutation.  Outputs: label_verts / label_quads [K + 1] int64, corner [V, 3] int32, verts [V, 3]
// fp32, vkey [V] int32 (the sorted corner keys, read by be_surf_remap).
int be_surf_gather(const int* L, int Z, int H, int W, int K, long long V, long long F, const long long* vperm,
                   const int* vcorner, const int* vlab, const int* qlab, long long* label_verts, long long* label_quads,
                   int* corner, float* verts, int* vkey, int* err, hipStream_t s) {
  long long NC;
  if (!dims_ok(Z, H, W, K, NC) || V <= 0 || F <= 0 || V >= (1LL << 31) || F >= (1LL << 31)) return (int)hipErrorInvalidValue;
  const Dims d{Z, H, W, K};
  hipLaunchKernelGGL(offsets_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, vlab, V, K, label_verts);
  hipLaunchKernelGGL(offsets_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, qlab, F, K, label_quads);
  hipLaunchKernelGGL(verts_kernel, dim3(blocks(V, 256)), dim3(256), 0, s, L, d, NC, V, vperm, vcorner, vlab, corner, verts,
                     vkey, err);
  return BE_CHECK_LAUNCH();
}

// After be_surf_gather on the same stream: quads [F, 4] int32 (16-byte aligned), every corner of every
// quad as its index in the label's segment label_verts[l - 1]:label_verts[l] of vkey.
int be_surf_remap(int Z, int H, int W, int K, long long V, long long F, const long long* qperm, const int* qcorner,
                  const unsigned char* qside, const int* qlab, const long long* label_verts, const int* vkey, int* quads,
                  int* err, hipStream_t s) {
  long long NC;
  if (!dims_ok(Z, H, W, K, NC) || V <= 0 || F <= 0 || V >= (1LL << 31) || F >= (1LL << 31)) return (int)hipErrorInvalidValue;
  const Dims d{Z, H, W, K};
  hipLaunchKernelGGL(quads_kernel, dim3(blocks(F, 256)), dim3(256), 0, s, d, NC, V, F, qperm, qcorner, qside, qlab,
                     label_verts, vkey, (int4*)quads, err);
  return BE_CHECK_LAUNCH();
}

// faces [K, 3] and voxels [K] int64, zeroed by the caller.
int be_surf_faces(int Z, int H, int W, int K, long long F, const long long* qperm, const int* qcorner,
                  const unsigned char* qside, const long long* label_quads, long long* faces, long long* voxels,
                  hipStream_t s) {
  long long NC;
  if (!dims_ok(Z, H, W, K, NC) || F <= 0 || F >= (1LL << 31)) return (int)hipErrorInvalidValue;
  const Dims d{Z, H, W, K};
  hipLaunchKernelGGL(faces_kernel, dim3(K, SL), dim3(256), 0, s, d, NC, F, qperm, qcorner, qside, label_quads,
                     (unsigned long long*)faces, (unsigned long long*)voxels);
  return BE_CHECK_LAUNCH();
}

// verts [V, 3] fp32, quads [F, 4] int32 (16-byte aligned), label_quads [K + 1]; part [K, 8, 2] fp64
// workspace; out [K, 2] fp64: area and signed volume of every label's mesh scaled by (sz, sy, sx).
int be_surf_stats(int K, long long V, long long F, const float* verts, const int* quads, const long long* label_quads,
                  double sz, double sy, double sx, double* part, double* out, hipStream_t s) {
  if (K <= 0) return 0;
  if (V <= 0 || F <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(stats_kernel, dim3(K, SL), dim3(256), 0, s, V, F, verts, (const int4*)quads, label_quads, sz, sy, sx,
                     part);
  hipLaunchKernelGGL(stats_combine_kernel, dim3(blocks(K, 256)), dim3(256), 0, s, K, part, out);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
