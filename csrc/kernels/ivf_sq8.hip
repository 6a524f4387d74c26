// IVF-SQ8: a list-sorted int8 copy of the vectors (one byte per dimension and one fp32 scale per row), its encoder
// and its list scan with the top-k selected inside, as in ivf_scan_topk.hip.
//
//   be_sq8_encode         src [N, D] bf16, gathered through `order` -> codes [n, D] int8, scales [n] fp32
//   be_ivf_sq8_scan_topk  per (query, slot range) the kk best (score, list-sorted row) pairs of the int8 scores
// The ranges' partial lists [Q, P, kk] are joined and mapped to ids by be_topk_merge (topk_merge.hip).
//
// Code format (the contract; numpy reproduces it bit for bit in float32).  For a row x of D values, taken as fp32:
//   amax = max_i |x_i|;  inv = 127 / amax and scale = amax / 127, each one correctly rounded fp32 division;
//   c_i = clamp(rintf(x_i * inv), -127, 127), the product rounded to fp32, ties to even;  amax == 0: codes 0, scale 0.
// Score of a row against a query: scale * sum_i q_i c_i (below).
//
// be_sq8_encode, MI355X design: one 16-lane group per output row, 16 rows per workgroup of 256 threads.  A lane
// reads dims 256 c + 16 sub .. + 15 of row order[r] (the gather is here: no list-sorted bf16 copy exists) as two
// 16-byte loads per c, takes the max-abs over its D / 16 values, the group's by xor-shuffle (8, 4, 2, 1), and writes
// its 16 codes of every c packed four to a dword as one 16-byte store: 16 lanes write 256 contiguous bytes.  Lane 0
// of the group writes the scale (a vector store).  The rows stay in registers between the two passes (8 D / 256
// dwords).
//
// be_ivf_sq8_scan_topk, MI355X design.  Contract, grid, cursor (list_cursor.h) and selection (topk_select.h) are
// those of be_ivf_scan_topk; the row fetch and the score are new.
//  * A workgroup of 256 threads (16 lane groups of 16) owns one query and one of P equal slot ranges of the query's
//    candidate row; the grid is Q P.
//  * A row is read by one lane group as D / 256 16-byte loads per lane (16 lanes cover 256 contiguous bytes); the
//    lane owns dims 256 c + 16 sub .. + 15 of load c and keeps the matching fp32 query slice in registers (D / 16
//    values: 48 at D = 768).  The range is swept in chunks of 16 R slots; the loads of chunk v + 1 are issued before
//    the arithmetic, the selection and the barrier of chunk v, into a second register set that swaps roles with the
//    first.  R = 8 / 8 / 4 / 4 at D / 256 = 1 / 2 / 3 / 4 (at D = 768: 12 loads per set, 96 KiB in flight per
//    workgroup, what the bf16 kernel keeps in flight).  The row's scale is loaded with the row's data, by the lane
//    of the group with sub == 0.
//  * Score: every code converts to fp32 exactly; one fmaf chain per lane in ascending dimension order, the 16-lane
//    xor butterfly at offsets 8, 4, 2, 1, then one fp32 multiply by the scale: scale * sum_i q_i c_i.
//    The compiler converts a dword's four signed bytes with v_cvt_f32_i32_sdwa (sext, src0_sel BYTE_0 .. BYTE_3): one
//    VALU instruction per code next to its v_fmac_f32, no separate extract or shift.  A lane spends 2 D / 16
//    instructions on a row (96 at D = 768: 48 conversions, 48 fmac), as many as on a bf16 row (a shift or a mask
//    per value, and its fmac): the VALU work per row is unchanged while the bytes halve, so per byte it doubles.
//  * No MFMA: every row is used once by one query, a bandwidth-bound GEMV.
//  * No global atomic, no host read, no grid barrier.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; launch bound 256 threads, 2 waves per SIMD planned,
// i.e. two workgroups on a CU, which 256 VGPRs allow):
//    sq8_scan_topk_kernel, D / 256      1     2     3     4
//    VGPRs                            170   250   201   249
//    SGPRs                             62    62    61    60
//    occupancy                          2     2     2     2   waves per SIMD
//    sq8_encode_kernel, VGPRs          39    56    59    81   (16 SGPRs, occupancy 8 / 8 / 8 / 5)
//  scratch 0 and no AGPRs in every instantiation.  The scan's LDS is dynamic (select_lds_bytes: 2 KiB up to kk = 128,
//  16 KiB at kk = 1024) plus 256 bytes of the barrier vote; the encoder uses none.  In the sweep loop at D = 768 the
//  arithmetic waits with vmcnt(23) .. vmcnt(12): the next chunk's 12 row loads stay in flight across the selection
//  and the barrier.  (A scale register written on both sides of the sub == 0 branch made the compiler wait for the
//  loads before the next chunk's were issued; hence the scale is read only inside the key of that lane.)
#include "common.h"
#include "list_cursor.h"
#include "topk_select.h"

namespace {

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------------------- encode
template <int CH>  // D = 256 * CH
__global__ __launch_bounds__(NT) void sq8_encode_kernel(const bf16_t* __restrict__ src,
                                                        const long long* __restrict__ order, long long n,
                                                        int8_t* __restrict__ codes, float* __restrict__ scales) {
  constexpr int D = 256 * CH;
  const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long long r = (long long)blockIdx.x * 16 + grp;
  if (r >= n) return;  // a whole lane group: the shuffles below stay inside one
  const long long from = order ? order[r] : r;
  const bf16_t* x = src + (size_t)from * D + sub * 16;
  u32x4 w[CH][2];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    w[c][0] = *reinterpret_cast<const u32x4*>(x + c * 256);
    w[c][1] = *reinterpret_cast<const u32x4*>(x + c * 256 + 8);
  }
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        amax = fmaxf(amax, fmaxf(fabsf(lo_bf(w[c][h][j])), fabsf(hi_bf(w[c][h][j]))));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 16));
  const bool zero = amax == 0.f;
  const float inv = zero ? 0.f : __fdiv_rn(127.f, amax);
  auto code = [&](float v) {
    const float t = fminf(fmaxf(rintf(__fmul_rn(v, inv)), -127.f), 127.f);
    return (uint32_t)(int)t & 0xffu;
  };
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {  // output dword d: dims 4 d .. 4 d + 3 of the lane's 16, i.e. input dwords 2 d, 2 d + 1
      const uint32_t a = w[c][d >> 1][(d & 1) * 2], b = w[c][d >> 1][(d & 1) * 2 + 1];
      o[d] = code(lo_bf(a)) | code(hi_bf(a)) << 8 | code(lo_bf(b)) << 16 | code(hi_bf(b)) << 24;
    }
    *reinterpret_cast<u32x4*>(codes + (size_t)r * D + c * 256 + sub * 16) = o;
  }
  if (sub == 0) scales[r] = zero ? 0.f : __fdiv_rn(amax, 127.f);
}

// ------------------------------------------------------------------------------------------------------------ scan
template <int CH>
struct RowsInFlight { static constexpr int R = CH <= 2 ? 8 : 4; };

__device__ __forceinline__ float code_f32(uint32_t w, int j) { return (float)(int)(int8_t)(w >> (8 * j)); }

template <int CH>  // D = 256 * CH
__global__ __launch_bounds__(NT, 2) void sq8_scan_topk_kernel(
    const float* __restrict__ q, const int* __restrict__ probes, const long long* __restrict__ list_off,
    const long long* __restrict__ cand_off, const int8_t* __restrict__ codes, const float* __restrict__ scales,
    int nprobe, int kk, int cap, int P, float* __restrict__ out_s, int* __restrict__ out_r) {
  constexpr int D = 256 * CH, R = RowsInFlight<CH>::R;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int sub = tid & 15, grp = tid >> 4;  // 16 lanes per row, 16 rows per sweep step
  const int qi = blockIdx.x / P, split = blockIdx.x - qi * P;
  float* os = out_s + (size_t)blockIdx.x * kk;
  int* orow = out_r + (size_t)blockIdx.x * kk;

  ListCursor<false> cur(cand_off, probes, list_off, nullptr, qi, nprobe);
  long long lo, hi;
  cur.range(split, P, lo, hi);
  if (lo >= hi) {  // the whole workgroup: nothing selected
    select_nothing<NT>(kk, tid, os, orow);
    return;
  }
  const Selector sel(smem, cap, kk, tid);

  float qv[CH][16];
  const float* qq = q + (size_t)qi * D + sub * 16;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 a = *reinterpret_cast<const float4*>(qq + c * 256 + 4 * j);
      qv[c][4 * j] = a.x; qv[c][4 * j + 1] = a.y; qv[c][4 * j + 2] = a.z; qv[c][4 * j + 3] = a.w;
    }
  __syncthreads();

  if (lo + grp < hi) cur.seek(lo + grp);  // this lane group's position in the row

  // rows of the chunk at c0, their loads and (sub == 0) their scales; a slot past the range has row -1 and loads
  // row 0 (tot > 0, so it exists), its score is never looked at
  auto fetch = [&](long long c0, int* row, u32x4 (*v)[CH], float* sc) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long slot = c0 + r * 16 + grp;
      row[r] = -1;
      if (slot < hi) row[r] = cur.row(slot);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t at = (size_t)(row[r] < 0 ? 0 : row[r]);
      const int8_t* src = codes + at * D + sub * 16;
#pragma unroll
      for (int c = 0; c < CH; ++c) v[r][c] = *reinterpret_cast<const u32x4*>(src + c * 256);
      if (sub == 0) sc[r] = scales[at];  // read by that lane alone (the key below); no value for the others
    }
  };

  // one chunk: the loads of the chunk after it go out first, into the other register set, even past the range's
  // end (16 R reads of row 0), as in ivf_scan_topk.hip
  auto step = [&](long long c0, const int* row, const u32x4 (*v)[CH], const float* sc, int* rown, u32x4 (*vn)[CH],
                  float* scn) {
    fetch(c0 + 16 * R, rown, vn, scn);
    float s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s[r] = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int j = 0; j < 4; ++j) s[r] = fmaf(code_f32(v[r][c][d], j), qv[c][4 * d + j], s[r]);
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] += __shfl_xor(s[r], off, 16);
    unsigned todo = 0;
    if (sub == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) todo |= row[r] >= 0 ? 1u << r : 0u;
    }
    select_offer<NT, R>(sel, todo, [&](int r) { return make_key(__fmul_rn(s[r], sc[r]), row[r]); }, tid);
  };

  // two register sets that swap roles (a copy between them would wait for the loads just issued)
  int row0[R], row1[R];
  float sc0[R], sc1[R];
  u32x4 v0[R][CH], v1[R][CH];
  fetch(lo, row0, v0, sc0);
#pragma unroll 1
  for (long long c0 = lo; c0 < hi; c0 += 32 * R) {
    step(c0, row0, v0, sc0, row1, v1, sc1);
    if (c0 + 16 * R >= hi) break;
    step(c0 + 16 * R, row1, v1, sc1, row0, v0, sc0);
  }

  select_finish<NT>(sel, tid, os, orow, nullptr);
}

template <int CH>
int launch_sq8_scan(const float* q, const int* probes, const long long* list_off, const long long* cand_off,
                    const int8_t* codes, const float* scales, int Q, int nprobe, int kk, int P, float* part_s,
                    int* part_r, hipStream_t s) {
  const int cap = select_cap(kk);
  hipLaunchKernelGGL(sq8_scan_topk_kernel<CH>, dim3((unsigned)(Q * P)), dim3(NT), select_lds_bytes(cap), s, q, probes,
                     list_off, cand_off, codes, scales, nprobe, kk, cap, P, part_s, part_r);
  return BE_CHECK_LAUNCH();
}

template <int CH>
int launch_sq8_encode(const bf16_t* src, const long long* order, long long n, int8_t* codes, float* scales,
                      hipStream_t s) {
  hipLaunchKernelGGL(sq8_encode_kernel<CH>, dim3((unsigned)((n + 15) / 16)), dim3(NT), 0, s, src, order, n, codes,
                     scales);
  return BE_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// src [N, D] bf16; order [n] int64 rows of src, or null for the identity; codes [n, D] int8; scales [n] fp32.
int be_sq8_encode(const void* src, const long long* order, long long n, int D, void* codes, float* scales,
                  hipStream_t s) {
  if (n < 0 || (n + 15) / 16 >= (1LL << 31)) return -1;
  if (D < 256 || D % 256 || D > 1024) return -6;
  if (n == 0) return 0;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(src);
  int8_t* c = reinterpret_cast<int8_t*>(codes);
  switch (D / 256) {
    case 1: return launch_sq8_encode<1>(x, order, n, c, scales, s);
    case 2: return launch_sq8_encode<2>(x, order, n, c, scales, s);
    case 3: return launch_sq8_encode<3>(x, order, n, c, scales, s);
    default: return launch_sq8_encode<4>(x, order, n, c, scales, s);
  }
}

// q [Q, D] fp32; probes / cand_off [Q, nprobe] (cand_off the exclusive prefix sum of the probed lists' sizes);
// list_off [nlist + 1]; codes [N, D] int8 and scales [N] fp32, list-sorted; part_s / part_r [Q, P, kk].
int be_ivf_sq8_scan_topk(const float* q, const int* probes, const long long* list_off, const long long* cand_off,
                         const void* codes, const float* scales, long long N, int Q, int nprobe, int D, int kk, int P,
                         float* part_s, int* part_r, hipStream_t s) {
  if (kk < 1 || kk > 1024) return -1;
  if (N < 0 || N >= (1LL << 31)) return -2;
  if (P < 1 || P > 65535) return -3;
  if (Q < 0 || nprobe < 1) return -4;
  if ((long long)Q * P >= (1LL << 31)) return -5;
  if (D < 256 || D % 256 || D > 1024) return -6;
  if (Q == 0) return 0;
  const int8_t* c = reinterpret_cast<const int8_t*>(codes);
#define SQ8_LAUNCH(CH) \
  case CH: return launch_sq8_scan<CH>(q, probes, list_off, cand_off, c, scales, Q, nprobe, kk, P, part_s, part_r, s)
  switch (D / 256) {
    SQ8_LAUNCH(1);
    SQ8_LAUNCH(2);
    SQ8_LAUNCH(3);
    SQ8_LAUNCH(4);
    default: return -6;
  }
#undef SQ8_LAUNCH
}

}  // extern "C"
