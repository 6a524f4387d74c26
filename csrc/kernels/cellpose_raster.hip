// Cellpose: polygon annotations rasterised to label images (gfx950).
//
// Semantics: bioengine_worker_amd/cellpose/reference.py::rasterize_rings (the CPU oracle; the GPU
// tests compare exactly).  The rule is in integers only: the host quantises the vertices to 1/256
// pixel, sorts the rings by (image, label) so that the edges of one label of one image (a *group*)
// are a contiguous run, takes every group's pixel box and cuts it into jobs.  One entry point:
//
//   be_cp_raster   raster   ONE WAVE PER JOB.  A job is (group, band of 64 rows, chunk of 64 * CW
//                           columns); lane r owns row r of the band and keeps the chunk's even-odd
//                           parity of that row in CW 64-bit words in registers.
//
// Edges.  The wave walks the group's edges 64 at a time: one coalesced 16-byte load per lane
// (Y0, X0, Y1, X1), then every edge is broadcast from its lane (v_readlane, the loop counter is
// uniform).  An edge that misses the band's centre lines altogether is skipped by the whole wave.
// A lane whose row the edge crosses -- (Y0 <= Cy) != (Y1 <= Cy) -- computes the first column whose
// centre is at or right of the crossing.  With the edge turned so that D = |Y1 - Y0| > 0 and
// N = (Cy - Y0) * (+-(X1 - X0)), the rule "(Cy - Y0)(X1 - X0) <= (Cx - X0)(Y1 - Y0)" (">=" for a
// falling edge) reads Cx >= X0 + ceil(N / D), so the column is (X0 + ceil(N / D) + 127) >> 8.
// |N| < 2^50 and D < 2^26, so both are exact doubles: the quotient comes from one fp64 division and
// an integer correction step makes it the exact floor (the rounded quotient is off by one at most).
// The lane then XORs "this column and everything right of it, within the chunk" into its words; a
// crossing left of the chunk flips the whole row of the chunk, one right of it flips nothing.
//
// Commit.  When the edges are done the wave takes the rows one by one: the row's words are
// broadcast from its lane, the 64 lanes take 64 consecutive columns and commit
// atomicMax(out[b, y, x], label) where their bit is set: coalesced 256-byte segments, no returned
// value.  XOR and max commute, so no launch order or geometry can change a result.  The output is
// zeroed by the caller.
//
// Bounded loops and memory.  Every loop runs to a count the host computed (edges of the group, rows
// and columns of the job); there is no spin, no retry and no data-dependent while.  Every store is
// checked against [0, H) x [0, W) of its own image and every edge read against the group's segment
// and the edge array's length, whatever the job table says.  No LDS, no scratch.
#include "common.h"

namespace {

constexpr int WPB = 4;  // waves (jobs) per workgroup
constexpr int CW = 4;   // 64-bit words per row of a job: a chunk is 64 * CW = 256 columns
constexpr int SUB = 256, HALF = 128;  // RASTER_SUBPIX of reference.py and the centre's offset

struct Job {  // 32 bytes, written by gpu.py::_raster_plan
  int e0, ne;     // the group's edges
  int b, label;   // image and label
  int y0, nrows;  // band: rows y0 .. y0 + nrows - 1, nrows <= 64
  int x0, ncols;  // chunk: columns x0 .. x0 + ncols - 1, ncols <= 64 * CW
};

// floor(n / d) for d > 0, |n| < 2^52, d < 2^31: the fp64 quotient is within one of it.
__device__ __forceinline__ long long floor_div(long long n, long long d) {
  long long q = (long long)floor((double)n / (double)d);
  long long r = n - q * d;
  if (r < 0) { q -= 1; r += d; }
  if (r >= d) q += 1;
  return q;
}

__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__global__ __launch_bounds__(64 * WPB) void raster_kernel(const int4* __restrict__ edges, long long n_edges,
                                                          const Job* __restrict__ jobs, long long n_jobs,
                                                          int* __restrict__ out, int B, int H, int W) {
  const int lane = threadIdx.x & 63;
  const long long j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long long)blockIdx.x * WPB;
  if (j >= n_jobs) return;
  const Job job = jobs[j];
  const int nrows = min(job.nrows, 64), ncols = min(job.ncols, 64 * CW);
  if ((unsigned)job.b >= (unsigned)B || nrows <= 0 || ncols <= 0 || job.ne <= 0 || job.e0 < 0) return;
  const long long e_end = min((long long)job.e0 + job.ne, n_edges);
  const int ne = (int)max(e_end - job.e0, 0ll);

  const bool active = lane < nrows;
  const int cy = (job.y0 + lane) * SUB + HALF;          // |y0| <= 2^15: far inside int
  const int cy_lo = job.y0 * SUB + HALF, cy_hi = (job.y0 + nrows - 1) * SUB + HALF;
  unsigned long long w[CW];
#pragma unroll
  for (int k = 0; k < CW; ++k) w[k] = 0ull;

  for (int base = 0; base < ne; base += 64) {
    int4 e = make_int4(0, 0, 0, 0);  // a zero-length edge crosses nothing
    if (base + lane < ne) e = edges[(long long)job.e0 + base + lane];
    const int n = min(64, ne - base);
    for (int i = 0; i < n; ++i) {
      const int Y0 = bcast(e.x, i), X0 = bcast(e.y, i), Y1 = bcast(e.z, i), X1 = bcast(e.w, i);
      // the edge crosses the rows with min(Y0, Y1) <= Cy < max(Y0, Y1): none of this band?
      if (min(Y0, Y1) > cy_hi || max(Y0, Y1) <= cy_lo) continue;
      if (active && ((Y0 <= cy) != (Y1 <= cy))) {
        const bool up = Y1 > Y0;
        const long long D = up ? (long long)Y1 - Y0 : (long long)Y0 - Y1;
        const long long dX = up ? (long long)X1 - X0 : (long long)X0 - X1;
        const long long N = ((long long)cy - Y0) * dX;
        const long long T = -floor_div(-N, D);                   // ceil(N / D)
        const long long rel = ((X0 + T + (HALF - 1)) >> 8) - job.x0;  // first column, in the chunk's frame
#pragma unroll
        for (int k = 0; k < CW; ++k) {
          const long long lo = rel - 64 * k;
          const unsigned long long m = lo <= 0 ? ~0ull : (lo >= 64 ? 0ull : (~0ull << (int)lo));
          w[k] ^= m;
        }
      }
    }
  }

  int* __restrict__ img = out + (size_t)job.b * H * W;
#pragma unroll
  for (int k = 0; k < CW; ++k) {
    if (64 * k >= ncols) break;
    const int c = 64 * k + lane, x = job.x0 + c;
    const bool col_ok = c < ncols && (unsigned)x < (unsigned)W;
    const int wlo = (int)(unsigned)w[k], whi = (int)(unsigned)(w[k] >> 32);
    for (int r = 0; r < nrows; ++r) {
      const unsigned long long row = (unsigned)bcast(wlo, r) | ((unsigned long long)(unsigned)bcast(whi, r) << 32);
      if (row == 0ull) continue;
      const int y = job.y0 + r;
      if (col_ok && (unsigned)y < (unsigned)H && ((row >> lane) & 1ull)) atomicMax(&img[(size_t)y * W + x], job.label);
    }
  }
}

}  // namespace

extern "C" {

// edges [n_edges, 4] int32 (Y0, X0, Y1, X1) on the 1/256-pixel lattice, jobs [n_jobs, 8] int32 (see
// Job), out [B, H, W] int32 zeroed by the caller.
int be_cp_raster(const int* edges, long long n_edges, const int* jobs, long long n_jobs, int* out, int B, int H, int W,
                 hipStream_t s) {
  if (n_jobs <= 0 || n_edges <= 0 || B <= 0 || H <= 0 || W <= 0) return 0;
  const long long blocks = (n_jobs + WPB - 1) / WPB;
  if (blocks >= (1ll << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(raster_kernel, dim3((unsigned)blocks), dim3(64 * WPB), 0, s, reinterpret_cast<const int4*>(edges), n_edges,
                     reinterpret_cast<const Job*>(jobs), n_jobs, out, B, H, W);
  return BE_CHECK_LAUNCH();
}

}  // extern "C"
