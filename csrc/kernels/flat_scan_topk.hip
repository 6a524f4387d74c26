// Flat (exhaustive) search for a few queries against many rows: a bf16 MFMA scan of the whole collection with the
// top-k selected inside the kernel, so no score ever reaches HBM.
//
//   be_flat_scan_topk  per (query, row range) the kk best (score, row) pairs of q [Q, D] . vecs [N, D]^T, bf16
// The ranges' partial lists [Q, P, kk] are joined by be_topk_merge (topk_merge.hip), called without an id table.
//
// Order everywhere: (score descending, row ascending), the 64-bit keys of topk_select.h (make_key, key_score,
// write_topk are used from it unchanged; the bitonic reselect is not: see "Selection").  The selection code is in
// flat_select.h, shared with flat_sq8_scan_topk.hip.
//
// be_flat_scan_topk, MI355X design:
//  * Work split.  grid.x = P contiguous ranges of 256-row tiles (tile t of range p: p T / P <= t < (p + 1) T / P),
//    grid.y = groups of 16 QT queries, QT = 1 / 2 / 4 a template parameter.  A workgroup of 256 threads (4 waves)
//    holds all of its group's queries, so within a group a row is fetched from HBM once for all of them.  Wave w
//    of the workgroup owns rows 64 w .. 64 w + 63 of every tile: 4 row fragments x QT query fragments of
//    v_mfma_f32_16x16x32_bf16, 16 QT fp32 accumulators per lane.  One query costs one 16-wide MFMA column.
//  * Queries: staged once into LDS as bf16, 32 QT D bytes (96 KiB at 64 x 768), in 32-deep k-steps of 64-byte
//    rows: byte 64 (s 16 QT + r) + 16 (c ^ ((r >> 2) & 3)) holds 16-byte chunk c of k-step s of query r.  The 16
//    lanes that read one chunk index of 16 queries hit 16 distinct 16-byte slots of a 256-byte bank row: no
//    conflict (the 128-byte-row swizzle of knn_topk.hip, folded to 64-byte rows so that D % 32 == 0 needs no
//    zero half step).  Rows of a partial last tile of queries are zeros and are never offered.
//  * Rows: global memory -> registers -> MFMA, no LDS hop (a row fragment is used by one wave).  Lane (r, g) =
//    (lane & 15, lane >> 4) loads 16 bytes of row 16 i + r at k-chunk g of the k-step: the four lanes of a row
//    read 64 contiguous bytes per load instruction, which is the longest run the fragment allows (a lane's row is
//    fixed by lane & 15 and a lane moves 16 bytes), so k is left unpermuted and the query image above matches it.
//    A stage is 4 k-steps (128 dims): 16 loads of 16 bytes per lane, 16 KiB per wave.  Two register sets swap
//    roles: the loads of the next stage, which may belong to the next tile, are issued before the MFMAs, the
//    selection and the barriers of the current one, so 64 KiB per workgroup stay in flight.  The fetch is
//    unconditional and free of branches: a k-step past D re-reads the last one and is multiplied as zeros, a row
//    past N re-reads row N - 1 and is never offered, the stage after the last re-reads valid rows.
//  * Selection.  Per query in LDS: `cap` keys, a count and a threshold, the current kk-th key (all ones while
//    fewer than kk were selected).  acc[i][t][e] of lane (r, g) is row 64 w + 16 i + 4 g + e against query
//    16 t + r, so a lane reads one threshold per query fragment.  When a tile's accumulators are complete a key
//    is appended (LDS atomic on the query's count) only if it is below the threshold.  A query whose list is
//    full is re-selected by one wave by rank counting (select_row of knn_topk.hip on 64-bit keys; keys are
//    unique, so ranks are a permutation and the list comes out sorted); the lanes that found no slot retry.
//    The workgroup vote is a 0 / 1 value.  What is kept never depends on the arrival order.  The bitonic
//    reselect of topk_select.h is not used: it sorts one list with the whole workgroup and wants a power-of-two
//    cap >= 256, 128 KiB for 64 queries.
//  * LDS: 32 QT D (image) + 16 QT (8 cap + 12) bytes.  cap is what the budget of 160 KiB less 256 bytes allows, at
//    most max(kk + 16, min(2 kk + 16, 320)), a multiple of 8 and at least kk + 16, below which the launcher refuses.  D = 768: 64
//    queries in one group up to kk = 104; kk = 256 (FLAT_MAX_K) in groups of 64 up to D = 160, of 32 up to D =
//    1440, of 16 up to D = 4000.  The result does not depend on cap.
//  * No scratch, no global atomic, no grid barrier, no host read.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; launch bound 256 threads, one workgroup per CU):
//    QT             1     2     4
//    VGPRs        187   199   255
//    AGPRs         16    32    80   (the accumulators; 16 more hold copies at QT = 4)
//    SGPRs        105   106    89
//    occupancy      2     2     1   waves per SIMD
//  scratch 0 in every instantiation; LDS dynamic (above) plus 256 static bytes of the barrier vote.  In the sweep
//  the MFMAs of a stage wait with vmcnt(31) .. vmcnt(16): the 16 loads of the next stage stay in flight across
//  them, the selection and the barriers.  A scheduling barrier after each fetch keeps the loads there (without it
//  the scheduler sank them below the MFMAs).  One flaw is left: at the head of the loop the compiler waits with
//  vmcnt(0) before the first of the two fetches, because it reuses registers of that set for addresses, so every
//  second stage is requested only once the stage before it has arrived.
#include "common.h"
#include "flat_select.h"

namespace {

constexpr int flat_lds_bytes(int qr, int D, int cap) { return qr * D * 2 + flat_lists_bytes(qr, cap); }

template <int QT>
__global__ __launch_bounds__(NT, 1) void flat_scan_topk_kernel(const bf16_t* __restrict__ q,
                                                               const bf16_t* __restrict__ vecs, int N, int Q, int D,
                                                               int kk, int cap, int P, float* __restrict__ out_s,
                                                               int* __restrict__ out_r) {
  constexpr int QR = 16 * QT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* img = smem;
  const FlatLists lists(smem + (size_t)QR * D * 2, QR, cap, kk);
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

  // ---- the query image, and empty lists
  const int KS = D >> 5, CPR = D >> 3;  // k-steps; 16-byte chunks of a row
  for (int o = tid; o < QR * CPR; o += NT) {
    const int r = o / CPR, j = o - r * CPR;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r < nq) v = *reinterpret_cast<const u32x4*>(q + (size_t)(qbase + r) * D + j * 8);
    *reinterpret_cast<u32x4*>(img + (((j >> 2) * QR + r) << 6) + (((j & 3) ^ ((r >> 2) & 3)) << 4)) = v;
  }
  lists.clear(QR, tid);
  __syncthreads();

  const int S = (KS + 3) >> 2;  // stages of a tile
  const unsigned char* qfrag = img + (fr << 6) + ((fg ^ ((fr >> 2) & 3)) << 4);

  // the rows of this lane in the tile at row0, as pointers to its k-chunk of k-step 0
  auto row_ptrs = [&](int row0, const bf16_t** fp) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = row0 + wave * 64 + i * 16 + fr;
      row = row < N ? row : N - 1;
      fp[i] = vecs + (size_t)row * D + fg * 8;
    }
  };
  // stage st of those rows: k-steps 4 st .. 4 st + 3, one past D re-reads the last
  auto fetch = [&](const bf16_t* const* fp, int st, u32x4 (*v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int s = st * 4 + u;
      s = s < KS ? s : KS - 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[u][i] = *reinterpret_cast<const u32x4*>(fp[i] + s * 32);
    }
  };

  f32x4 acc[4][QT];  // [row fragment i][query fragment t]
  auto clear = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < QT; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  auto multiply = [&](int st, const u32x4 (*v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = st * 4 + u;
      const bool in = s < KS;
      const unsigned char* qs = qfrag + (size_t)(in ? s : KS - 1) * (QR * 64);
      bf16x8 fq[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) fq[t] = *reinterpret_cast<const bf16x8*>(qs + t * 16 * 64);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4 w = in ? v[u][i] : (u32x4){0u, 0u, 0u, 0u};
        const bf16x8 fv = __builtin_bit_cast(bf16x8, w);
#pragma unroll
        for (int t = 0; t < QT; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, fq[t], acc[i][t], 0, 0, 0);
      }
    }
  };

  // the complete accumulators of the tile at row0 are offered to the queries' lists
  auto offer = [&](int row0) {
    flat_offer<QT>(lists, nq, N, row0, wave, lane, [&](int i, int t, int e) { return acc[i][t][e]; });
  };

  // ---- the sweep: two register sets that swap roles (a copy between them would wait for the loads just issued)
  const bf16_t* fp[4];
  u32x4 v0[4][4], v1[4][4];
  int frow = t_lo * TILE, fst = 0;  // the fetch's tile and stage
  int crow = frow, cst = 0;         // the arithmetic's
  int left = t_hi - t_lo;
  row_ptrs(frow, fp);
  fetch(fp, 0, v0);
  clear();
  auto advance = [&]() {
    if (++fst == S) {
      fst = 0;
      frow += TILE;
      row_ptrs(frow, fp);
    }
  };
  // after the stage's MFMAs: whether the sweep ends here
  auto stage_end = [&]() -> bool {
    if (++cst < S) return false;
    offer(crow);
    clear();
    cst = 0;
    crow += TILE;
    return --left == 0;
  };
#pragma unroll 1
  for (;;) {
    advance();
    fetch(fp, fst, v1);
    __builtin_amdgcn_sched_barrier(0);  // the loads go out before the MFMAs, not where the scheduler sinks them
    multiply(cst, v0);
    if (stage_end()) break;
    advance();
    fetch(fp, fst, v0);
    __builtin_amdgcn_sched_barrier(0);
    multiply(cst, v1);
    if (stage_end()) break;
  }

  // ---- every list sorted (the vote that ended the last offer is the barrier before this), and written
  flat_finish(lists, nq, wave, lane, out_of, out_s, out_r);
}

template <int QT>
int launch_flat(const bf16_t* q, const bf16_t* vecs, int N, int Q, int D, int kk, int P, float* part_s, int* part_r,
                hipStream_t s) {
  constexpr int QR = 16 * QT;
  const int cap = flat_cap(QR, (long long)QR * D * 2, kk);
  if (!cap) return -8;
  const int lds = flat_lds_bytes(QR, D, cap);
  static bool attr[BE_MAX_DEV] = {};
  if (!attr[be_cur_dev()]) {
    if (hipFuncSetAttribute((const void*)flat_scan_topk_kernel<QT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_BUDGET) != hipSuccess)
      return -30;
    attr[be_cur_dev()] = true;
  }
  const dim3 grid((unsigned)P, (unsigned)((Q + QR - 1) / QR));
  hipLaunchKernelGGL(flat_scan_topk_kernel<QT>, grid, dim3(NT), lds, s, q, vecs, N, Q, D, kk, cap, P, part_s, part_r);
  return BE_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// q [Q, D], vecs [N, D] bf16 row-major; part_s / part_r [Q, P, kk]: per query and row range the kk largest
// q[i].vecs[j] with their rows, (score descending, row ascending), padded with -inf / -1.  group = 16 / 32 / 64
// queries per workgroup; -8 where the group's query image and kk + 16 keys per query do not fit the LDS.
int be_flat_scan_topk(const void* q, const void* vecs, long long N, int Q, int D, int kk, int P, int group,
                      float* part_s, int* part_r, hipStream_t s) {
  if (kk < 1 || kk > FLAT_MAX_K) return -1;
  if (N < 1 || N >= (1LL << 31) - 2 * TILE) return -2;  // the fetch runs one tile past the range
  if (P < 1 || P > 65535) return -3;
  if (Q < 0) return -4;
  if (D < 32 || D % 32) return -6;
  if (group != 16 && group != 32 && group != 64) return -7;
  if (Q == 0) return 0;
  if ((Q + group - 1) / group > 65535) return -5;
  const bf16_t* a = reinterpret_cast<const bf16_t*>(q);
  const bf16_t* b = reinterpret_cast<const bf16_t*>(vecs);
  switch (group) {
    case 16: return launch_flat<1>(a, b, (int)N, Q, D, kk, P, part_s, part_r, s);
    case 32: return launch_flat<2>(a, b, (int)N, Q, D, kk, P, part_s, part_r, s);
    default: return launch_flat<4>(a, b, (int)N, Q, D, kk, P, part_s, part_r, s);
  }
}

}  // extern "C"
