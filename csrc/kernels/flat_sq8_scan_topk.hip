// Flat (exhaustive) search over SQ8 rows for a few queries: an int8 MFMA scan of the whole collection with the top-k
// selected inside the kernel.  No value is converted and no fmac is issued per code: the queries are int8 too.
//
//   be_flat_sq8_scan_topk  per (query, row range) the kk best (score, row) pairs of q [Q, D] fp32 against
//                          codes [N, D] int8 / scales [N] fp32 (the code format of ivf_sq8.hip, rows in id order)
// The ranges' partial lists [Q, P, kk] are joined by be_topk_merge (topk_merge.hip), called without an id table.
//
// Score contract (numpy reproduces it bit for bit in float32).  A query q [D] is split into two int8 vectors, by the
// rule of the rows:  amax = max_i |q_i|;  inv = 127 / amax and sq = amax / 127, each one fp32 division;
//   t_i = q_i * inv (rounded to fp32);  h_i = clamp(rint(t_i), -127, 127), ties to even;  r_i = t_i - h_i (exact);
//   l_i = clamp(rint(256 r_i), -127, 127);  amax == 0: h = l = 0 and sq = 0.
// With H = sum_i c_i h_i and L = sum_i c_i l_i (int32, exact in any order):
//   t = float(H) + float(L) * 2^-8 (one fp32 rounding);  w = scale * sq (fp32);  s = w * t (fp32).
// float(H) and float(L) are exact: |H|, |L| <= D 127^2 = 16 516 096 < 2^24 at D = 1024.  A score does not depend on
// how the work is split.  Order: (score descending, row ascending), the 64-bit keys of topk_select.h.
// The file is built with -ffp-contract=off: q_i * inv - h_i must not become one fma.
//
// MI355X design.  Frame (grid, tiles, stages, selection) as in flat_scan_topk.hip; the data path is this kernel's.
//  * Work split.  grid.x = P contiguous ranges of 256-row tiles, grid.y = groups of 16 G queries, G = 1 / 2 a
//    template parameter.  A workgroup of 256 threads (4 waves), wave w owns rows 64 w .. 64 w + 63 of every tile:
//    4 row fragments x G pairs of query fragments of v_mfma_i32_16x16x64_i8, 32 G int32 accumulators per lane.
//  * Query fragments.  A query is the same column of a pair of 16-wide fragments, one of h and one of l, so
//    accH[i][t][e] and accL[i][t][e] of a lane are H and L of the same (row, query): combined without a shuffle.
//  * Query encoding, inside the kernel while the group is staged into LDS: wave w encodes queries w, w + 4, ..;
//    lane j < D / 16 holds values 16 j .. 16 j + 15 (four 16-byte loads), one wave_max gives amax, the lane writes
//    its 16 h and 16 l codes as one 16-byte store each.  No encode launch, no global buffer.
//  * LDS: two int8 images (h, then l) of 16 G D bytes each (48 KiB at 32 x 768), in 64-deep k-steps of 64-byte
//    rows: byte 64 (s 16 G + r) + 16 (c ^ ((r >> 2) & 3)) holds values 64 s + 16 c .. + 15 of query r, the swizzle of
//    flat_scan_topk.hip (the 16 lanes that read one chunk index of 16 queries hit 16 distinct 16-byte slots of a
//    256-byte bank row).  Then the lists of flat_select.h, then sq per query.  Queries past Q are zeros.
//  * Rows: global memory -> registers -> MFMA, no LDS hop.  Lane (r, g) = (lane & 15, lane >> 4) loads 16 bytes of
//    row 16 i + r at chunk g of the k-step: the four lanes of a row read 64 contiguous bytes per load instruction,
//    one k-step of 64 int8 values, so k is not permuted (A and B fragments share the lane -> k map).  A stage is 4
//    k-steps (256 dims; D % 256 == 0, so no partial stage): 16 loads of 16 bytes per lane, 16 KiB per wave.  Two
//    register sets swap roles: the next stage, also across a tile's end, is in flight during the MFMAs, the
//    selection and the barriers.  The fetch is unconditional: a row past N re-reads row N - 1 and is never offered.
//  * Scales: lane l of wave w loads the scale of row 64 w + l of the fetch's tile with every stage (one dword load
//    next to 16 of 16 bytes, so a set is complete in itself); the offer takes row 16 i + 4 g + e's from lane
//    16 i + 4 g + e of the last stage's set (ds_bpermute), 16 per tile.
//  * Selection: flat_select.h, shared with flat_scan_topk.hip.  cap by its rule against the LDS that is left.
//  * No scratch, no global atomic, no grid barrier, no host read.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; __launch_bounds__(256, 2) at G = 1 and (256, 1) at
// G = 2, where (256, 2) left 180 bytes of scratch per lane):
//    G              1     2
//    VGPRs        239   249
//    AGPRs          0    88   (the 64 accumulators and copies)
//    SGPRs         89    89
//    occupancy      2     1   waves per SIMD
//  scratch 0 in both; LDS dynamic (above) plus 256 static bytes of the barrier vote.  In the sweep the MFMAs of a
//  stage wait with vmcnt(32) .. vmcnt(17): the 17 loads of the next stage (16 of rows, one scale) stay in flight
//  across them, the selection and the barriers; a scheduling barrier after each fetch keeps the loads there.  The
//  flaw of flat_scan_topk.hip is here too: before one of the loop's two fetches (the first at G = 1, the second at
//  G = 2) the compiler waits with vmcnt(0), so every second stage is requested only once the stage before it has
//  arrived, and the MFMAs of that stage then wait for nothing.
#include "common.h"
#include "flat_select.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int flat_sq8_lds_bytes(int qr, int D, int cap) { return qr * (2 * D + 4) + flat_lists_bytes(qr, cap); }

__device__ __forceinline__ uint32_t sq8_byte(float v) {
  return (uint32_t)(int)fminf(fmaxf(rintf(v), -127.f), 127.f) & 0xffu;
}

template <int G>
__global__ __launch_bounds__(NT, 3 - G) void flat_sq8_scan_topk_kernel(const float* __restrict__ q,
                                                                   const int8_t* __restrict__ codes,
                                                                   const float* __restrict__ scales, int N, int Q,
                                                                   int D, int kk, int cap, int P,
                                                                   float* __restrict__ out_s, int* __restrict__ out_r) {
  constexpr int QR = 16 * G;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* img = smem;       // h; the l image follows at LOFF
  const int LOFF = QR * D;
  const FlatLists lists(smem + (size_t)2 * QR * D, QR, cap, kk);
  float* sq = reinterpret_cast<float*>(lists.cnt + QR);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int p = blockIdx.x, qbase = blockIdx.y * QR;
  const int nq = Q - qbase < QR ? Q - qbase : QR;
  const int T = (N + TILE - 1) / TILE;
  const int t_lo = (int)((long long)p * T / P), t_hi = (int)((long long)(p + 1) * T / P);
  auto out_of = [&](int qq) { return ((size_t)(qbase + qq) * P + p) * kk; };

  if (t_lo >= t_hi) {  // the whole workgroup: nothing selected
    for (int qq = wave; qq < nq; qq += 4) write_topk<64, int>(nullptr, 0, kk, lane, out_s + out_of(qq), out_r + out_of(qq), nullptr);
    return;
  }

  // ---- the queries, encoded into the two images; sq; empty lists
  const bool mine = lane < (D >> 4);  // the lane's 16 values exist
  for (int r = wave; r < QR; r += 4) {  // wave-uniform
    float x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = 0.f;
    if (mine && r < nq) {
      const float* src = q + (size_t)(qbase + r) * D + lane * 16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(src + 4 * j);
        x[4 * j] = a.x; x[4 * j + 1] = a.y; x[4 * j + 2] = a.z; x[4 * j + 3] = a.w;
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(x[j]));
    amax = wave_max(amax);
    const bool zero = amax == 0.f;
    const float inv = zero ? 0.f : __fdiv_rn(127.f, amax);
    u32x4 ph, pl;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t wh = 0, wl = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = __fmul_rn(x[4 * d + j], inv);
        const float h = fminf(fmaxf(rintf(t), -127.f), 127.f);
        wh |= ((uint32_t)(int)h & 0xffu) << (8 * j);
        wl |= sq8_byte((t - h) * 256.f) << (8 * j);
      }
      ph[d] = wh;
      pl[d] = wl;
    }
    if (mine) {
      const int at = (((lane >> 2) * QR + r) << 6) + (((lane & 3) ^ ((r >> 2) & 3)) << 4);
      *reinterpret_cast<u32x4*>(img + at) = ph;
      *reinterpret_cast<u32x4*>(img + LOFF + at) = pl;
    }
    if (lane == 0) sq[r] = zero ? 0.f : __fdiv_rn(amax, 127.f);
  }
  lists.clear(QR, tid);
  __syncthreads();

  const int S = D >> 8;  // stages of a tile: 4 k-steps of 64 each
  const unsigned char* qfrag = img + (fr << 6) + ((fg ^ ((fr >> 2) & 3)) << 4);
  float sqv[G];
#pragma unroll
  for (int t = 0; t < G; ++t) sqv[t] = sq[16 * t + fr];

  // the rows of this lane in the tile at row0, as pointers to its chunk of k-step 0, and its scale's
  auto row_ptrs = [&](int row0, const int8_t** fp, const float*& sp) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = row0 + wave * 64 + i * 16 + fr;
      row = row < N ? row : N - 1;
      fp[i] = codes + (size_t)row * D + fg * 16;
    }
    int row = row0 + wave * 64 + lane;
    row = row < N ? row : N - 1;
    sp = scales + row;
  };
  // stage st of those rows: k-steps 4 st .. 4 st + 3
  auto fetch = [&](const int8_t* const* fp, const float* sp, int st, u32x4 (*v)[4], float& sc) {
    sc = *sp;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[u][i] = *reinterpret_cast<const u32x4*>(fp[i] + (st * 4 + u) * 64);
  };

  i32x4 accH[4][G], accL[4][G];  // [row fragment i][query fragment pair t]
  auto clear = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < G; ++t) accH[i][t] = accL[i][t] = (i32x4){0, 0, 0, 0};
  };
  auto multiply = [&](int st, const u32x4 (*v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned char* qs = qfrag + (size_t)(st * 4 + u) * (QR * 64);
      i32x4 fh[G], fl[G];
#pragma unroll
      for (int t = 0; t < G; ++t) {
        fh[t] = *reinterpret_cast<const i32x4*>(qs + t * 16 * 64);
        fl[t] = *reinterpret_cast<const i32x4*>(qs + LOFF + t * 16 * 64);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const i32x4 fv = __builtin_bit_cast(i32x4, v[u][i]);
#pragma unroll
        for (int t = 0; t < G; ++t) {
          accH[i][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fv, fh[t], accH[i][t], 0, 0, 0);
          accL[i][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fv, fl[t], accL[i][t], 0, 0, 0);
        }
      }
    }
  };

  // the complete accumulators of the tile at row0 become scores (sc: the scale of row 64 wave + lane of that tile)
  // and are offered to the queries' lists
  auto offer = [&](int row0, float sc) {
    float s[4][G][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float rs = __shfl(sc, 16 * i + 4 * fg + e, 64);
#pragma unroll
        for (int t = 0; t < G; ++t) {
          const float tv = __fadd_rn((float)accH[i][t][e], __fmul_rn((float)accL[i][t][e], 0x1p-8f));
          s[i][t][e] = __fmul_rn(__fmul_rn(rs, sqv[t]), tv);
        }
      }
    flat_offer<G>(lists, nq, N, row0, wave, lane, [&](int i, int t, int e) { return s[i][t][e]; });
  };

  // ---- the sweep: two register sets that swap roles (a copy between them would wait for the loads just issued)
  const int8_t* fp[4];
  const float* sp;
  u32x4 v0[4][4], v1[4][4];
  float sc0, sc1;
  int frow = t_lo * TILE, fst = 0;  // the fetch's tile and stage
  int crow = frow, cst = 0;         // the arithmetic's
  int left = t_hi - t_lo;
  row_ptrs(frow, fp, sp);
  fetch(fp, sp, 0, v0, sc0);
  clear();
  auto advance = [&]() {
    if (++fst == S) {
      fst = 0;
      frow += TILE;
      row_ptrs(frow, fp, sp);
    }
  };
  // after the stage's MFMAs: whether the sweep ends here
  auto stage_end = [&](float sc) -> bool {
    if (++cst < S) return false;
    offer(crow, sc);
    clear();
    cst = 0;
    crow += TILE;
    return --left == 0;
  };
#pragma unroll 1
  for (;;) {
    advance();
    fetch(fp, sp, fst, v1, sc1);
    __builtin_amdgcn_sched_barrier(0);  // the loads go out before the MFMAs, not where the scheduler sinks them
    multiply(cst, v0);
    if (stage_end(sc0)) break;
    advance();
    fetch(fp, sp, fst, v0, sc0);
    __builtin_amdgcn_sched_barrier(0);
    multiply(cst, v1);
    if (stage_end(sc1)) break;
  }

  // ---- every list sorted (the vote that ended the last offer is the barrier before this), and written
  flat_finish(lists, nq, wave, lane, out_of, out_s, out_r);
}

template <int G>
int launch_flat_sq8(const float* q, const int8_t* codes, const float* scales, int N, int Q, int D, int kk, int P,
                    float* part_s, int* part_r, hipStream_t s) {
  constexpr int QR = 16 * G;
  const int cap = flat_cap(QR, (long long)QR * (2 * D + 4), kk);
  if (!cap) return -8;
  static bool attr[BE_MAX_DEV] = {};
  if (!attr[be_cur_dev()]) {
    if (hipFuncSetAttribute((const void*)flat_sq8_scan_topk_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_BUDGET) != hipSuccess)
      return -30;
    attr[be_cur_dev()] = true;
  }
  const dim3 grid((unsigned)P, (unsigned)((Q + QR - 1) / QR));
  hipLaunchKernelGGL(flat_sq8_scan_topk_kernel<G>, grid, dim3(NT), flat_sq8_lds_bytes(QR, D, cap), s, q, codes, scales,
                     N, Q, D, kk, cap, P, part_s, part_r);
  return BE_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// q [Q, D] fp32 (16-byte aligned), codes [N, D] int8 (16-byte aligned) and scales [N] fp32 in id order;
// part_s / part_r [Q, P, kk]: per query and row range the kk largest scores of the contract above with their rows,
// (score descending, row ascending), padded with -inf / -1.  group = 16 / 32 queries per workgroup; -8 where the
// group's images and kk + 16 keys per query do not fit the LDS (never at D <= 1024).
int be_flat_sq8_scan_topk(const float* q, const void* codes, const float* scales, long long N, int Q, int D, int kk,
                          int P, int group, float* part_s, int* part_r, hipStream_t s) {
  if (kk < 1 || kk > FLAT_MAX_K) return -1;
  if (N < 1 || N >= (1LL << 31) - 2 * TILE) return -2;  // the fetch runs one tile past the range
  if (P < 1 || P > 65535) return -3;
  if (Q < 0) return -4;
  if (D < 256 || D % 256 || D > 1024) return -6;
  if (group != 16 && group != 32) return -7;
  if (((uintptr_t)q | (uintptr_t)codes) & 15) return -9;
  if (Q == 0) return 0;
  if ((Q + group - 1) / group > 65535) return -5;
  const int8_t* c = reinterpret_cast<const int8_t*>(codes);
  return group == 16 ? launch_flat_sq8<1>(q, c, scales, (int)N, Q, D, kk, P, part_s, part_r, s)
                     : launch_flat_sq8<2>(q, c, scales, (int)N, Q, D, kk, P, part_s, part_r, s);
}

}  // extern "C"
