// UMAP for the cell-search landscape view (gfx950): smooth-kNN calibration and the layout epoch.
//
// Semantics: bioengine_worker_amd/search/reference.py (smooth_knn, memberships, layout_epoch); the GPU
// tests compare stage by stage.  Host entry points:
//
//   be_umap_smooth_knn  one row of k <= 64 neighbour distances per group of 16 lanes: rho, the
//                       bisection of sigma (fp64, as the oracle's rule precision), the floor, and
//                       the k-1 directed memberships
//   be_umap_epoch       ONE synchronous layout epoch: reads positions Yin, writes Yout
//   be_umap_layout      epochs [ep0, ep1) queued back to back, ping-ponging two position buffers
//
// Transform of new points onto a fitted layout (reference.py: smooth_knn_query, memberships_query,
// transform_epoch):
//
//   be_umap_smooth_knn_query  the same bisection over k columns WITHOUT a self column: rho is the row
//                             minimum (zero included), every column is summed, the floor is the row's
//                             own mean, k memberships per row
//   be_umap_transform         every epoch of [ep0, ep1) in ONE launch: the training positions are
//                             fixed and a query reads nothing but its own <= 64 edges, so its whole
//                             optimisation is a closed loop in the registers of its 16 lanes
//
// The epoch is a GATHER: a fixed group of 16 lanes owns a vertex, walks its CSR row, evaluates the
// active edges and their negative samples, updates next / nneg of its own edges in place (each
// directed edge has exactly one writer), reduces the partial sums with a fixed xor butterfly and
// writes y + delta.  No float atomic anywhere, no wait on another workgroup, no allocation and no
// synchronisation in the launch functions: two runs give the same bits, and a caller may capture the
// loop in a graph.  The schedule arithmetic uses explicitly rounded operations (hipcc would contract
// m * epn + nneg into an FMA, which the float32 oracle does not do): the activity mask and the
// sample counts equal the oracle's exactly.
#include "common.h"

namespace {

constexpr int GROUP = 16;                 // lanes per row / vertex
constexpr int THREADS = 256;              // 4 waves, 16 groups
constexpr int GROUPS = THREADS / GROUP;
constexpr int MAX_K = 64;
constexpr int PER_LANE = MAX_K / GROUP;   // distances held by one lane

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // commutative: every lane gets the same bits
  return v;
}
__device__ __forceinline__ float group_min(float v) {
#pragma unroll
  for (int o = GROUP / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// dist [n, k] float32 (column 0 the point itself), idx [n, k]; gmean: the mean of all distances (one
// double on the device).  rho / sigma [n] float32, memb [n, k-1] float32.
//
// QUERY: the rows are new points against a training set.  There is no self column: rho is the row
// minimum, all k columns are summed and written (memb [n, k]), the floor is 1e-3 of the row's own mean;
// idx and gmean are not read.  The fit's entry point cannot serve here: it zeroes a membership where
// idx == row, and a query's row number colliding with a training index would silently drop an edge.
template <bool QUERY>
__global__ __launch_bounds__(THREADS) void smooth_knn_kernel(const float* __restrict__ dist, const int* __restrict__ idx,
                                                             int n, int k, const double* __restrict__ gmean,
                                                             float* __restrict__ rho, float* __restrict__ sigma,
                                                             float* __restrict__ memb) {
  const int sub = threadIdx.x & (GROUP - 1);
  const long long row = (long long)blockIdx.x * GROUPS + (threadIdx.x / GROUP);
  const bool live = row < n;  // a dead group still takes part in the shuffles
  double d[PER_LANE];
  float rmin = INFINITY;
  double rsum = 0.0;
#pragma unroll
  for (int t = 0; t < PER_LANE; ++t) {
    const int j = sub + t * GROUP;
    const float v = (live && j < k) ? dist[row * k + j] : 0.0f;
    d[t] = (double)v;
    rsum += (double)v;
    if (QUERY ? (live && j < k) : (v > 0.0f)) rmin = fminf(rmin, v);
  }
  rmin = group_min(rmin);
  rsum = group_sum(rsum);
  const double r = (rmin == INFINITY) ? 0.0 : (double)rmin;
  const double target = log2((double)k);
  constexpr int J0 = QUERY ? 0 : 1;  // first summed column
  double lo = 0.0, hi = INFINITY, mid = 1.0;
#pragma unroll 1
  for (int it = 0; it < 64; ++it) {  // every lane of a group takes the same decisions
    double ps = 0.0;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
      const int j = sub + t * GROUP;
      if (j >= J0 && j < k) {
        const double g = d[t] - r;
        ps += (g > 0.0) ? exp(-(g / mid)) : 1.0;
      }
    }
    ps = group_sum(ps);
    if (fabs(ps - target) < 1e-5) break;
    if (ps > target) {
      hi = mid;
      mid = (lo + hi) * 0.5;
    } else {
      lo = mid;
      mid = (hi == INFINITY) ? mid * 2.0 : (lo + hi) * 0.5;
    }
  }
  const double floor_ = 1e-3 * ((QUERY || r > 0.0) ? rsum / (double)k : gmean[0]);
  const double sg = fmax(mid, floor_);
  if (!live) return;
  if (sub == 0) {
    rho[row] = (float)r;
    sigma[row] = (float)sg;
  }
#pragma unroll
  for (int t = 0; t < PER_LANE; ++t) {
    const int j = sub + t * GROUP;
    if (j >= J0 && j < k) {
      const double g = d[t] - r;
      double a = (g <= 0.0 || sg == 0.0) ? 1.0 : exp(-(g / sg));
      if (QUERY) {
        memb[row * k + j] = (float)a;
      } else {
        if ((long long)idx[row * k + j] == row) a = 0.0;  // a listed self contributes nothing
        memb[row * (k - 1) + (j - 1)] = (float)a;
      }
    }
  }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ float clip4(float v) { return fminf(fmaxf(v, -4.0f), 4.0f); }

// One epoch.  row_ptr [n+1] int64, col [nnz]; eps / epn read, next / nneg updated in place.
__global__ __launch_bounds__(THREADS) void epoch_kernel(const float2* __restrict__ Yin, float2* __restrict__ Yout, int n,
                                                        const long long* __restrict__ row_ptr,
                                                        const int* __restrict__ col, long long nnz,
                                                        const float* __restrict__ eps, const float* __restrict__ epn,
                                                        float* __restrict__ next, float* __restrict__ nneg, int ep,
                                                        float alpha, float a, float b, float gamma, uint32_t seed) {
  const int sub = threadIdx.x & (GROUP - 1);
  const long long vtx = (long long)blockIdx.x * GROUPS + (threadIdx.x / GROUP);
  const bool live = vtx < n;
  const float epf = (float)ep;
  double sx = 0.0, sy = 0.0;  // fp64 partial sums: a hub row adds hundreds of terms
  float2 yj = make_float2(0.f, 0.f);
  if (live) {
    yj = Yin[vtx];
    long long e0 = row_ptr[vtx], e1 = row_ptr[vtx + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nnz) e1 = nnz;  // never past the edge arrays, whatever the row pointers say
#pragma unroll 1
    for (long long e = e0 + sub; e < e1; e += GROUP) {
      const float nx = next[e];
      if (!(nx <= epf)) continue;
      const int kk = col[e];
      const float es = eps[e], en = epn[e], ng = nneg[e];
      if ((unsigned)kk < (unsigned)n) {
        const float2 yk = Yin[kk];
        const float dx = yj.x - yk.x, dy = yj.y - yk.y;
        const float d2 = dx * dx + dy * dy;
        if (d2 > 0.0f) {
          const float pw = powf(d2, b);
          const float c = -2.0f * a * b * (pw / d2) / (a * pw + 1.0f);
          sx += (double)(2.0f * clip4(c * dx) * alpha);
          sy += (double)(2.0f * clip4(c * dy) * alpha);
        }
      }
      int m = (int)__fdiv_rn(__fsub_rn(epf, ng), en);
      if (m < 0) m = 0;
      const uint32_t h = mix32(mix32((uint32_t)e ^ seed) + (uint32_t)ep);
#pragma unroll 1
      for (int p = 0; p < m; ++p) {
        const uint32_t v = mix32(h + (uint32_t)p) % (uint32_t)n;
        if ((long long)v == vtx) continue;
        const float2 yv = Yin[v];
        const float dx = yj.x - yv.x, dy = yj.y - yv.y;
        const float d2 = dx * dx + dy * dy;
        if (!(d2 > 0.0f)) continue;
        const float pw = powf(d2, b);
        const float c = 2.0f * gamma * b / ((0.001f + d2) * (a * pw + 1.0f));
        sx += (double)(clip4(c * dx) * alpha);
        sy += (double)(clip4(c * dy) * alpha);
      }
      next[e] = __fadd_rn(nx, es);
      nneg[e] = __fadd_rn(ng, __fmul_rn((float)m, en));
    }
  }
  sx = group_sum(sx);
  sy = group_sum(sy);
  if (live && sub == 0) Yout[vtx] = make_float2((float)((double)yj.x + sx), (float)((double)yj.y + sy));
}

inline int epoch_launch(const float2* Yin, float2* Yout, int n, const long long* row_ptr, const int* col,
                        long long nnz, const float* eps, const float* epn, float* next, float* nneg, int ep,
                        float alpha, float a, float b, float gamma, int seed, hipStream_t s) {
  const int blocks = (n + GROUPS - 1) / GROUPS;
  hipLaunchKernelGGL(epoch_kernel, dim3(blocks), dim3(THREADS), 0, s, Yin, Yout, n, row_ptr, col, nnz, eps, epn, next,
                     nneg, ep, alpha, a, b, gamma, (uint32_t)seed);
  return BE_CHECK_LAUNCH();
}

constexpr int MAX_DRAWS = 4096;  // negative samples of one slot in one epoch (reference.TRANSFORM_MAX_DRAWS)

// Transform: query q of m sits in a group of 16 lanes; lane `sub` holds slots sub, sub + 16, ... of the
// query's k <= 64 edges to FIXED training positions.  A slot's schedule (eps = 1 / w, epn = eps / nsr,
// next, nneg) and the query's position live in registers across all epochs [ep0, ep1).  Every lane of a
// group ends an epoch with the same position bits (the butterfly is commutative), so nothing is
// broadcast.  A dead group (q >= m) runs the same epochs with no slot and takes part in every shuffle.
__global__ __launch_bounds__(THREADS) void transform_kernel(const float2* __restrict__ Ytrain, int n,
                                                            const int* __restrict__ idx, const float* __restrict__ w,
                                                            int m, int k, float2* __restrict__ Y,
                                                            float* __restrict__ next, float* __restrict__ nneg,
                                                            int ep0, int ep1, int n_epochs, float lr4, float a, float b,
                                                            float gamma, float nsr, uint32_t seed) {
  const int sub = threadIdx.x & (GROUP - 1);
  const long long q = (long long)blockIdx.x * GROUPS + (threadIdx.x / GROUP);
  const bool live = q < m;
  const float thr = __fdiv_rn(1.0f, (float)n_epochs);  // a slot below it never fires
  int col[PER_LANE];
  float es[PER_LANE], en[PER_LANE], nx[PER_LANE], ng[PER_LANE];
  bool on[PER_LANE];
  float2 y = make_float2(0.f, 0.f);
  uint32_t key0 = 0;
  if (live) {
    y = Y[q];
    key0 = (uint32_t)idx[q * k] * 64u;  // intrinsic to the query: its nearest training point
  }
#pragma unroll
  for (int t = 0; t < PER_LANE; ++t) {
    const int j = sub + t * GROUP;
    on[t] = false;
    col[t] = 0;
    es[t] = en[t] = nx[t] = ng[t] = INFINITY;
    if (live && j < k) {
      const float wv = w[q * k + j];
      col[t] = idx[q * k + j];
      es[t] = __fdiv_rn(1.0f, wv);
      en[t] = __fdiv_rn(es[t], nsr);
      nx[t] = next ? next[q * k + j] : es[t];
      ng[t] = nneg ? nneg[q * k + j] : en[t];
      on[t] = (wv >= thr) && ((unsigned)col[t] < (unsigned)n);  // never index past the training set
    }
  }
#pragma unroll 1
  for (int ep = ep0; ep < ep1; ++ep) {
    const float epf = (float)ep;
    const float alpha = (float)((double)lr4 * (1.0 - (double)ep / (double)n_epochs));
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
      if (!(on[t] && nx[t] <= epf)) continue;
      {
        const float2 yk = Ytrain[col[t]];
        const float dx = y.x - yk.x, dy = y.y - yk.y;
        const float d2 = dx * dx + dy * dy;
        if (d2 > 0.0f) {
          const float pw = powf(d2, b);
          const float c = -2.0f * a * b * (pw / d2) / (a * pw + 1.0f);
          sx += (double)(clip4(c * dx) * alpha);  // factor 1: one direction, the other end is fixed
          sy += (double)(clip4(c * dy) * alpha);
        }
      }
      int ns = (int)__fdiv_rn(__fsub_rn(epf, ng[t]), en[t]);
      ns = ns < 0 ? 0 : (ns > MAX_DRAWS ? MAX_DRAWS : ns);
      const uint32_t h = mix32(mix32((key0 + (uint32_t)(sub + t * GROUP)) ^ seed) + (uint32_t)ep);
#pragma unroll 1
      for (int p = 0; p < ns; ++p) {
        const uint32_t v = mix32(h + (uint32_t)p) % (uint32_t)n;
        const float2 yv = Ytrain[v];
        const float dx = y.x - yv.x, dy = y.y - yv.y;
        const float d2 = dx * dx + dy * dy;
        if (!(d2 > 0.0f)) continue;
        const float pw = powf(d2, b);
        const float c = 2.0f * gamma * b / ((0.001f + d2) * (a * pw + 1.0f));
        sx += (double)(clip4(c * dx) * alpha);
        sy += (double)(clip4(c * dy) * alpha);
      }
      nx[t] = __fadd_rn(nx[t], es[t]);
      ng[t] = __fadd_rn(ng[t], __fmul_rn((float)ns, en[t]));
    }
    sx = group_sum(sx);
    sy = group_sum(sy);
    y = make_float2((float)((double)y.x + sx), (float)((double)y.y + sy));
  }
  if (!live) return;
  if (sub == 0) Y[q] = y;
  if (next && nneg) {
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
      const int j = sub + t * GROUP;
      if (j < k) {
        next[q * k + j] = nx[t];
        nneg[q * k + j] = ng[t];
      }
    }
  }
}

}  // namespace

extern "C" int be_umap_smooth_knn(const float* dist, const int* idx, int n, int k, const double* gmean, float* rho,
                                  float* sigma, float* memb, hipStream_t s) {
  if (n < 1) return 0;
  if (k < 2 || k > MAX_K) return (int)hipErrorInvalidValue;
  const int blocks = (n + GROUPS - 1) / GROUPS;
  hipLaunchKernelGGL(smooth_knn_kernel<false>, dim3(blocks), dim3(THREADS), 0, s, dist, idx, n, k, gmean, rho, sigma,
                     memb);
  return BE_CHECK_LAUNCH();
}

// dist [m, k] float32, ascending, no self column.  rho / sigma [m], memb [m, k].
extern "C" int be_umap_smooth_knn_query(const float* dist, int m, int k, float* rho, float* sigma, float* memb,
                                        hipStream_t s) {
  if (m < 1) return 0;
  if (k < 1 || k > MAX_K) return (int)hipErrorInvalidValue;
  const int blocks = (m + GROUPS - 1) / GROUPS;
  hipLaunchKernelGGL(smooth_knn_kernel<true>, dim3(blocks), dim3(THREADS), 0, s, dist, (const int*)nullptr, m, k,
                     (const double*)nullptr, rho, sigma, memb);
  return BE_CHECK_LAUNCH();
}

// Yin != Yout, both [n] float2.  alpha is the caller's float32 lr * (1 - ep / n_epochs).
extern "C" int be_umap_epoch(const float* Yin, float* Yout, int n, const long long* row_ptr, const int* col,
                             long long nnz, const float* eps, const float* epn, float* next, float* nneg, int ep,
                             float alpha, float a, float b, float gamma, int seed, hipStream_t s) {
  if (n < 1) return 0;
  if (Yin == Yout || nnz < 0 || ep < 0) return (int)hipErrorInvalidValue;
  return epoch_launch((const float2*)Yin, (float2*)Yout, n, row_ptr, col, nnz, eps, epn, next, nneg, ep, alpha, a, b,
                      gamma, seed, s);
}

// Epochs ep0 .. ep1-1 of n_epochs: epoch ep reads Y0 when (ep - ep0) is even, else Y1, and writes the
// other; the result is in Y0 when (ep1 - ep0) is even, else in Y1.
extern "C" int be_umap_layout(float* Y0, float* Y1, int n, const long long* row_ptr, const int* col, long long nnz,
                              const float* eps, const float* epn, float* next, float* nneg, int ep0, int ep1,
                              int n_epochs, float lr, float a, float b, float gamma, int seed, hipStream_t s) {
  if (n < 1 || ep1 <= ep0) return 0;
  if (Y0 == Y1 || nnz < 0 || ep0 < 0 || n_epochs < ep1) return (int)hipErrorInvalidValue;
  for (int ep = ep0; ep < ep1; ++ep) {
    const float alpha = (float)((double)lr * (1.0 - (double)ep / (double)n_epochs));
    float* in = ((ep - ep0) & 1) ? Y1 : Y0;
    float* out = ((ep - ep0) & 1) ? Y0 : Y1;
    const int rc = epoch_launch((const float2*)in, (float2*)out, n, row_ptr, col, nnz, eps, epn, next, nneg, ep,
                                alpha, a, b, gamma, seed, s);
    if (rc) return rc;
  }
  return 0;
}

// Epochs ep0 .. ep1-1 of n_epochs for m queries against n fixed training positions, in one launch.
// Ytrain [n] float2, idx / w [m, k] (the query table and its memberships), Y [m] float2: the start on
// entry, the result on exit (each query has one reader and one writer).  next / nneg [m, k]: the
// schedule state, read on entry and written on exit; both null means the initial state (next = eps,
// nneg = epn), needs ep0 == 0, and writes nothing.  No atomic, no LDS, no wait on another group, no
// host read.  The training positions (8 bytes per point) are gathered through L2 and not staged in LDS:
// measured at 10^6 queries, folding every gather onto 16 training points changes the time by 1 %
// (tools/umap_transform_bench.py, layout_16_train); the powf chains bound the kernel.
extern "C" int be_umap_transform(const float* Ytrain, int n, const int* idx, const float* w, int m, int k, float* Y,
                                 float* next, float* nneg, int ep0, int ep1, int n_epochs, float lr, float a, float b,
                                 float gamma, int nsr, int seed, hipStream_t s) {
  if (k < 1 || k > MAX_K || n < 1 || m < 0 || nsr < 1 || ep0 < 0 || n_epochs < ep1) return (int)hipErrorInvalidValue;
  if ((next == nullptr) != (nneg == nullptr) || (next == nullptr && ep0 > 0)) return (int)hipErrorInvalidValue;
  if (m < 1 || ep1 <= ep0) return 0;
  const int blocks = (m + GROUPS - 1) / GROUPS;
  hipLaunchKernelGGL(transform_kernel, dim3(blocks), dim3(THREADS), 0, s, (const float2*)Ytrain, n, idx, w, m, k,
                     (float2*)Y, next, nneg, ep0, ep1, n_epochs, lr * 0.25f, a, b, gamma, (float)nsr, (uint32_t)seed);
  return BE_CHECK_LAUNCH();
}
