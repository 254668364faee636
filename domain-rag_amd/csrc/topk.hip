// topk.hip — exact inner-product top-k over a resident fp32 corpus (gfx950).
//
// Replaces faiss.IndexFlatIP.add/search as used by clip_first_stage_retrieval
// (retrieval/clip100_resnet_style_all_shots.py:425-434): scores = corpus · query, the k largest,
// descending.  faiss leaves the accumulation order (BLAS sgemm) and the tie order unspecified;
// this implementation DEFINES both so that results are bit-reproducible (oracle/topk.c is the
// CPU restatement of exactly this order):
//   score(n, q) = fp32 fma chain, c = 0, over k in the order
//                 for blk in 0..d/16:  for s in 0..3:  for g in 0..3:  k = 16*blk + 4*g + s
//   ties -> lower corpus index first.
//
// Scan kernel (HBM-bound: N*d*4 bytes per pass): each wave streams groups of 16 corpus rows
// HBM -> LDS with LDS-DMA (full 256-B row segments, XOR-swizzled; the next group's first chunk is
// already in flight while the current group's last chunk is multiplied), then feeds
// v_mfma_f32_16x16x4_f32 (exact fp32, bitwise an fmaf chain) with 16 rows x 16 queries; the
// reduction over d happens inside the matrix core, no cross-lane shuffles.
//
// Round 3 — ONE corpus pass for up to 64 queries, and selection that never sees the corpus:
//   * query tiles: a launch carries ceil(Q/16) <= 4 tiles of 16 queries.  The workgroups b, b+8, b+16, b+24 land on the
//     SAME XCD (the dispatcher deals workgroups round-robin over the 8 XCDs), walk the SAME corpus rows and differ only in
//     their query tile: the first of them pulls a row chunk from HBM into that XCD's L2, the other three hit it there.
//     HBM traffic stays N*d*4 per launch whatever Q <= 64 (the reference re-builds its index and re-reads the corpus per
//     query, retrieval/...:419-430).  At Q = 64 the launch is bound by the exact-f32 matrix core, not by HBM:
//     2*N*d*Q = 7.75 GFLOP at N = 118 287 is 49 us at the 157 TFLOP/s f32 MFMA peak, against 38 us for the bytes.
//   * threshold pre-filter: a first, small launch scores a strided SAMPLE of 8192 rows (512 groups spread evenly over the
//     corpus); the k-th largest (score, index) composite of the sample is a valid lower bound T_q of the final k-th largest
//     (those k rows are in the corpus).  For k <= 128 only the best composite of each sampled group is kept and T_q is the
//     k-th best of those 512 group maxima: still k different rows, ~10 % more candidates, a 16x smaller selection (-7.5 us).  The main scan then keeps a score only if its composite is >= T_q — about k*N/8192
//     rows per query (1 400 of 118 287 for k = 100) — and appends it to the query's candidate list; the score matrix
//     [Q, N] is never written or re-read.  Every WAVE owns a region of each query's list sized for all the rows it visits
//     and counts its appends in a register (ballot + popcount: no atomics — a first version with one global atomic per
//     candidate ran the Q = 16 call in 235 us, the counters shared a cache line and 23 000 atomics queued on it); a wave
//     stores its per-query counts once, at its end.  The final selection (prefix sum over the regions' counts, radix select +
//     bitonic sort + decode, one workgroup per query) works on the candidates alone.  The regions have room for all N rows,
//     so a sample that misrepresents the corpus costs time, never correctness, and the whole call is deterministic.
// Selection: (score, index) -> unique 64-bit composite key; radix select in LDS over slices of the input, bitonic sort.
//
// Round 4 — the call as TWO launches where every group maximum of a query fits one workgroup's registers (k <= 128, 513 .. 8192 groups
// of 16 rows: N <= 131 072, the reference's COCO corpus among them): the scan writes the scores and each group's best composite
// (SCAN_SCORES_GMAX), select_groups_kernel takes the k-th best group maximum as the bound — exactly k groups reach it and the answer
// lives in their 16 k rows — gathers those scores and ranks them.  No sample, no threshold launch, no candidate regions; the work does
// not depend on the score distribution.  Q = 1 call at N = 118 287: 61.5 -> 47.2 us for a 37.7 us scan.
#include "drag_launch.h"
#include <float.h>

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ unsigned okey(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;  // NaN ranks below every real score
  if (u == 0x80000000u) u = 0u;                     // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}
// composite: score order in the high word, lower index wins ties in the low word; never 0 for a real row (0 = empty slot)
__device__ __forceinline__ u64 composite(float score, unsigned row) { return ((u64)okey(score) << 32) | (u64)(~row); }

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  return ((u64)(unsigned)__shfl((int)(v >> 32), src, 64) << 32) | (unsigned)__shfl((int)(unsigned)v, src, 64);
}

// ------------------------------------------------------------------ scan
enum { SCAN_SCORES = 0, SCAN_KEYS_DENSE = 1, SCAN_KEYS_FILTER = 2, SCAN_GROUP_MAX = 3, SCAN_SCORES_GMAX = 4 };
struct ScanArgs {
  const float* corpus;
  const float* queries;  // [Q, d], Q <= 64 in one launch
  long long N;
  int d, Q, ntile;       // ntile = ceil(Q / 16)
  int mode;
  // which groups of 16 rows this launch visits: group(i) = i * gstride, i < niter  (gstride 1 = the whole corpus)
  long long gstride, niter;
  // SCAN_SCORES
  float* scores;         // [Q, npad]
  long long npad;
  // SCAN_KEYS_DENSE: keys[q * kstride + 16 * i + r] = composite(score, row), 0 for rows >= N
  // SCAN_GROUP_MAX: keys[q * kstride + i] = the best composite among the 16 rows of group(i) (0 if the group has no row)
  // SCAN_SCORES_GMAX: both of SCAN_SCORES and SCAN_GROUP_MAX in one pass (the two-launch top-k call)
  // SCAN_KEYS_FILTER: wave v = worker * 4 + w appends the composites >= thresh[q] it finds to its own region
  //   keys[q * kstride + v * region_cap + n], n = 0, 1, ...; counts[q * nregions + v] = how many
  u64* keys;
  long long kstride;
  const u64* thresh;
  unsigned* counts;
  long long region_cap;
  int nregions;
};

// QT: query tiles (of 16 queries) a workgroup keeps in LDS and runs against every row group it streams (each K fragment read
// from LDS feeds QT MFMAs).  QT = 1 is the HBM-bound form (two workgroups per CU); QT > 1 trades the second workgroup for
// LDS (32 KiB per tile at d = 512) when the launch is matrix-core-bound anyway.
template <int NBUF, int QT>
__global__ __launch_bounds__(256, 2) void ip_scan_kernel(ScanArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // layout: query image of this workgroup's QT tiles [QT][d/64][16][256 B] | per wave: NBUF x 4 KiB staging ring
  const int nch = p.d / 64;
  char* sQ = smem;
  const int w = wave_id(), l = lane_id();
  char* sA = smem + QT * nch * 4096 + w * (NBUF * 4096);

  // workgroups b, b+8, ..., b+8*(ntile-1) sit on one XCD: same rows, different group of QT query tiles (L2 serves the re-reads)
  const int grp8 = (int)blockIdx.x >> 3;
  const int tile = grp8 % p.ntile;
  const long long worker = (long long)(grp8 / p.ntile) * 8 + ((int)blockIdx.x & 7);
  const long long nworkers = (long long)(gridDim.x / (8 * p.ntile)) * 8;
  const int q0 = tile * 16 * QT;

  // ---- query image (rows past Q are zero) ----
  for (int i = threadIdx.x; i < QT * 16 * (p.d / 4); i += 256) {
    const int q = i / (p.d / 4), k4 = i - q * (p.d / 4);  // query within the workgroup's QT * 16, float4 index within the row
    const int t = q >> 4, qq = q & 15;
    const int c = k4 >> 4, slot = k4 & 15;
    f32x4_t v = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if (q0 + q < p.Q) v = *(const f32x4_t*)(p.queries + (long long)(q0 + q) * p.d + k4 * 4);
    *(f32x4_t*)(sQ + (t * nch + c) * 4096 + qq * 256 + ((slot ^ qq) & 15) * 16) = v;
  }
  __syncthreads();

  const int g = l >> 4, r16 = l & 15;
  const int rd_base = r16 * 256;
  // this lane's DMA role inside a group chunk: instruction i covers rows 4i + (l>>4)
  // physical slot l&15 holds logical slot (l&15) ^ (row&15)
  unsigned lane_off[4];
  int lane_row[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lane_row[i] = 4 * i + (l >> 4);
    lane_off[i] = (unsigned)((((l & 15) ^ (lane_row[i] & 15)) & 15) * 16);
  }
  // per tile t: this lane's query q0 + 16 t + r16 (valid while < Q)
  u64 T[QT];
  unsigned ncand[QT];                    // filter mode: candidates of the lane's query appended by this wave so far (same in its 4 lanes)
  u64* region[QT];
  const long long step = nworkers * 4;
  const long long first = worker * 4 + w;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int q = q0 + 16 * t + r16;
    T[t] = ~0ull; ncand[t] = 0; region[t] = nullptr;
    if (p.mode == SCAN_KEYS_FILTER && q < p.Q) {
      T[t] = p.thresh[q];
      region[t] = p.keys + (long long)q * p.kstride + (worker * 4 + w) * p.region_cap;
    }
  }
  if (first >= p.niter) {                // a wave without rows still owns a region per query: say that it is empty
    if (p.mode == SCAN_KEYS_FILTER) {
#pragma unroll
      for (int t = 0; t < QT; ++t)
        if (l < 16 && q0 + 16 * t + l < p.Q) p.counts[(long long)(q0 + 16 * t + l) * p.nregions + worker * 4 + w] = 0u;
    }
    return;
  }

  // ---- the wave's work is ONE stream of (group, 256-byte chunk) steps; the LDS-DMA runs NBUF - 1 steps ahead of the MFMAs,
  // across group boundaries too (the next group's first chunks fly under this group's last ones) ----
  const long long nmine = (p.niter - first + step - 1) / step;
  const long long total = nmine * nch;
  // issue side
  __amdgpu_buffer_rsrc_t rs;
  unsigned voff[4];
  long long is_it = first;               // group iteration of the next chunk to issue
  int is_c = 0, is_buf = 0;
  auto issue = [&]() {
    if (is_c == 0) {                     // the DMA descriptor of a group: base of its 16 rows, clamped row offsets for a ragged last group
      const long long row0 = is_it * p.gstride * 16;
      const int nvalid = (int)min((long long)16, p.N - row0);
      rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.corpus + row0 * p.d), 0, (unsigned)(nvalid * p.d * 4), 0x00020000);
#pragma unroll
      for (int i = 0; i < 4; ++i) voff[i] = (unsigned)(min(lane_row[i], nvalid - 1) * p.d * 4) + lane_off[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (DRAG_LDS void*)((DRAG_LDS char*)sA + is_buf * 4096 + i * 1024), 16, voff[i],
                                               is_c * 256, 0, 0);
    is_buf = is_buf + 1 == NBUF ? 0 : is_buf + 1;
    if (++is_c == nch) { is_c = 0; is_it += step; }
  };
  constexpr int D = NBUF - 1;
  for (int i = 0; i < D && i < total; ++i) issue();

  long long it = first;
  int c = 0, buf = 0;
  f32x4_t acc[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (long long sidx = 0; sidx < total; ++sidx) {
    if (sidx + D < total) {
      issue();
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * D) : "memory");
    } else {                             // the tail: fewer chunks ahead of this one than the ring holds
      const int ahead = (int)(total - 1 - sidx);
      if (D >= 3 && ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (D >= 2 && ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const char* a = sA + buf * 4096 + rd_base;
    const char* q = sQ + c * 4096 + rd_base;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      const int so = (((4 * cc + g) ^ r16) & 15) * 16;
      const f32x4_t av = *(const f32x4_t*)(a + so);
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const f32x4_t qv = *(const f32x4_t*)(q + t * nch * 4096 + so);
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ss], qv[ss], acc[t], 0, 0, 0);
      }
    }
    // the next step's DMA overwrites this buffer's predecessor in the ring, whose reads were consumed by the MFMAs above
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    buf = buf + 1 == NBUF ? 0 : buf + 1;
    if (++c < nch) continue;
    c = 0;

    // ---- a group is complete: acc[t][r] = score[row0 + 4g + r][query q0 + 16 t + r16]
    const long long row0 = it * p.gstride * 16;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const int qq = q0 + 16 * t + r16;
      if (p.mode == SCAN_KEYS_FILTER) {
        // the query lives in lanes r16, r16 + 16, r16 + 32, r16 + 48: slots are handed out with ballots, no atomics
        u64 key[4];
        bool pass[4], any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row0 + 4 * g + r;
          key[r] = composite(acc[t][r], (unsigned)row);
          pass[r] = row < p.N && key[r] >= T[t];        // T = ~0 in lanes without a query
          any = any || pass[r];
        }
        if (__ballot(any) != 0ull) {
          const u64 mine = 0x0001000100010001ull << r16;
          const u64 below = (1ull << l) - 1ull;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const u64 m = __ballot(pass[r]) & mine;
            if (pass[r]) region[t][ncand[t] + __popcll(m & below)] = key[r];
            ncand[t] += (unsigned)__popcll(m);
          }
        }
      } else if (p.mode == SCAN_GROUP_MAX || p.mode == SCAN_SCORES_GMAX) {
        if (p.mode == SCAN_SCORES_GMAX && qq < p.Q) *(f32x4_t*)(p.scores + (long long)qq * p.npad + row0 + 4 * g) = acc[t];
        u64 m = 0ull;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row0 + 4 * g + r;
          const u64 key = row < p.N ? composite(acc[t][r], (unsigned)row) : 0ull;
          m = key > m ? key : m;
        }
        // the query's 16 rows live in lanes r16, r16 + 16, r16 + 32, r16 + 48
        { const u64 o = shfl64(m, l ^ 16); m = o > m ? o : m; }
        { const u64 o = shfl64(m, l ^ 32); m = o > m ? o : m; }
        if (l < 16 && qq < p.Q) p.keys[(long long)qq * p.kstride + it] = m;
      } else if (qq < p.Q) {
        if (p.mode == SCAN_SCORES) {
          *(f32x4_t*)(p.scores + (long long)qq * p.npad + row0 + 4 * g) = acc[t];
        } else {
          u64* dst = p.keys + (long long)qq * p.kstride + it * 16 + 4 * g;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const long long row = row0 + 4 * g + r;
            dst[r] = row < p.N ? composite(acc[t][r], (unsigned)row) : 0ull;
          }
        }
      }
      acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    it += step;
  }
  if (p.mode == SCAN_KEYS_FILTER) {
#pragma unroll
    for (int t = 0; t < QT; ++t)
      if (l < 16 && q0 + 16 * t + l < p.Q) p.counts[(long long)(q0 + 16 * t + l) * p.nregions + worker * 4 + w] = ncand[t];
  }
}

// ------------------------------------------------------------------ scan, d = 512: the queries in REGISTERS (round 5)
// ip_scan_kernel reads every query fragment from the workgroup's LDS image again for every corpus chunk: 4 KiB of query reads next to the
// 4 KiB of corpus reads and the 4 KiB the LDS-DMA writes, per wave and chunk — 8 waves of a CU keep the LDS ~75 % busy, and at 64 queries
// per pass (four sibling workgroups per row range, the exact-f32 matrix core the bound) the scan reached only half of the matrix peak.
// A tile of 16 queries x 512 dimensions is 128 floats per lane in the MFMA's own operand layout (lane (g, r16): query q0 + r16, the four
// floats at d = 64 c + 16 cc + 4 g of every chunk c and quarter cc): with two waves per SIMD there are 256 registers per lane, so the
// tile lives in registers for the whole launch, loaded once straight from global memory (L2 after the first workgroup).  No query image,
// no start-up barrier, half the LDS reads, 32 KiB of LDS per workgroup instead of 64.  The chunk index has to be a compile-time constant
// for that (register arrays cannot be indexed at run time), so a group's eight chunks are unrolled; the LDS-DMA stream is the same one
// (chunk by chunk, one ahead, across group boundaries), the MFMA order per output is the same: same bits (every top-k / score test runs
// on this kernel by default; "topk_qreg" = 1 switches back to ip_scan_kernel for the A/B).  Same grid, same row -> wave assignment, same
// output modes.
__global__ __launch_bounds__(256, 2) void ip_scan_q512_kernel(ScanArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 2 * 4096];     // per wave: two 4 KiB chunk buffers
  constexpr int nch = 8;
  const int w = wave_id(), l = lane_id();
  char* sA = smem + w * (2 * 4096);
  const int grp8 = (int)blockIdx.x >> 3;
  const int tile = grp8 % p.ntile;
  const long long worker = (long long)(grp8 / p.ntile) * 8 + ((int)blockIdx.x & 7);
  const long long nworkers = (long long)(gridDim.x / (8 * p.ntile)) * 8;
  const int q0 = tile * 16;
  const int g = l >> 4, r16 = l & 15;
  const int rd_base = r16 * 256;
  unsigned lane_off[4];
  int lane_row[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lane_row[i] = 4 * i + (l >> 4);
    lane_off[i] = (unsigned)((((l & 15) ^ (lane_row[i] & 15)) & 15) * 16);
  }
  const int qq = q0 + r16;
  u64 T = ~0ull;
  unsigned ncand = 0;
  u64* region = nullptr;
  const long long step = nworkers * 4;
  const long long first = worker * 4 + w;
  if (p.mode == SCAN_KEYS_FILTER && qq < p.Q) {
    T = p.thresh[qq];
    region = p.keys + (long long)qq * p.kstride + (worker * 4 + w) * p.region_cap;
  }
  if (first >= p.niter) {                // a wave without rows still owns a region per query: say that it is empty
    if (p.mode == SCAN_KEYS_FILTER && l < 16 && q0 + l < p.Q) p.counts[(long long)(q0 + l) * p.nregions + worker * 4 + w] = 0u;
    return;
  }
  // ---- the first chunk's DMA goes out before the query tile is fetched (both latencies overlap)
  const long long nmine = (p.niter - first + step - 1) / step;
  __amdgpu_buffer_rsrc_t rs;
  unsigned voff[4];
  auto descriptor = [&](long long it_) {     // base of a group's 16 rows, clamped row offsets for a ragged last group
    const long long row0 = it_ * p.gstride * 16;
    const int nvalid = (int)min((long long)16, p.N - row0);
    rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.corpus + row0 * 512), 0, (unsigned)(nvalid * 512 * 4), 0x00020000);
#pragma unroll
    for (int i = 0; i < 4; ++i) voff[i] = (unsigned)(min(lane_row[i], nvalid - 1) * 512 * 4) + lane_off[i];
  };
  auto issue = [&](int buf, int c) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (DRAG_LDS void*)((DRAG_LDS char*)sA + buf * 4096 + i * 1024), 16, voff[i], c * 256, 0, 0);
  };
  descriptor(first);
  issue(0, 0);
  f32x4_t qv[nch][4];
  {
    const float* qp = p.queries + (long long)min(qq, p.Q - 1) * 512 + 4 * g;
#pragma unroll
    for (int c = 0; c < nch; ++c)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        qv[c][cc] = *(const f32x4_t*)(qp + 64 * c + 16 * cc);
        if (qq >= p.Q) qv[c][cc] = (f32x4_t){0.f, 0.f, 0.f, 0.f};          // rows past Q are zero (as in the LDS image)
      }
  }
  long long it = first;
  for (long long j = 0; j < nmine; ++j, it += step) {
    const bool more = j + 1 < nmine;
    f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < nch; ++c) {
      // chunk c sits (or lands) in buffer c & 1; the next chunk of the stream goes to the other buffer, whose reads the MFMAs of the
      // previous chunk consumed (lgkmcnt(0) below)
      if (c + 1 < nch) {
        issue((c + 1) & 1, c + 1);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else if (more) {
        descriptor(it + step);
        issue(0, 0);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      const char* a = sA + (c & 1) * 4096 + rd_base;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const f32x4_t av = *(const f32x4_t*)(a + ((((4 * cc + g) ^ r16) & 15) * 16));
#pragma unroll
        for (int ss = 0; ss < 4; ++ss) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ss], qv[c][cc][ss], acc, 0, 0, 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // ---- a group is complete: acc[r] = score[row0 + 4g + r][query q0 + r16]
    const long long row0 = it * p.gstride * 16;
    if (p.mode == SCAN_KEYS_FILTER) {
      u64 key[4];
      bool pass[4], any = false;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = row0 + 4 * g + r;
        key[r] = composite(acc[r], (unsigned)row);
        pass[r] = row < p.N && key[r] >= T;        // T = ~0 in lanes without a query
        any = any || pass[r];
      }
      if (__ballot(any) != 0ull) {
        const u64 mine = 0x0001000100010001ull << r16;
        const u64 below = (1ull << l) - 1ull;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const u64 m = __ballot(pass[r]) & mine;
          if (pass[r]) region[ncand + __popcll(m & below)] = key[r];
          ncand += (unsigned)__popcll(m);
        }
      }
    } else if (p.mode == SCAN_GROUP_MAX || p.mode == SCAN_SCORES_GMAX) {
      if (p.mode == SCAN_SCORES_GMAX && qq < p.Q) *(f32x4_t*)(p.scores + (long long)qq * p.npad + row0 + 4 * g) = acc;
      u64 m = 0ull;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = row0 + 4 * g + r;
        const u64 key = row < p.N ? composite(acc[r], (unsigned)row) : 0ull;
        m = key > m ? key : m;
      }
      { const u64 o = shfl64(m, l ^ 16); m = o > m ? o : m; }
      { const u64 o = shfl64(m, l ^ 32); m = o > m ? o : m; }
      if (l < 16 && qq < p.Q) p.keys[(long long)qq * p.kstride + it] = m;
    } else if (qq < p.Q) {
      if (p.mode == SCAN_SCORES) {
        *(f32x4_t*)(p.scores + (long long)qq * p.npad + row0 + 4 * g) = acc;
      } else {
        u64* dst = p.keys + (long long)qq * p.kstride + it * 16 + 4 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row0 + 4 * g + r;
          dst[r] = row < p.N ? composite(acc[r], (unsigned)row) : 0ull;
        }
      }
    }
  }
  if (p.mode == SCAN_KEYS_FILTER && l < 16 && q0 + l < p.Q) p.counts[(long long)(q0 + l) * p.nregions + worker * 4 + w] = ncand;
}

// ------------------------------------------------------------------ selection
constexpr int LMAX = 8192;   // elements a selection workgroup holds in LDS
constexpr int KMAX = 2048;
constexpr int SAMPLE_GROUPS = 512;   // 8192 sampled rows

struct SelArgs {
  const u64* keys;        // [Q, kstride]
  long long kstride;
  // input form 1 (counts == null): keys[q * kstride + 0 .. fixed_count)
  // input form 2: nregions regions of region_cap slots, region v holds counts[q * nregions + v] keys
  const unsigned* counts;
  long long fixed_count;
  long long region_cap;
  int nregions;
  int k, kpad;
  // outputs: either the threshold ...
  u64* thresh;
  // ... or the decoded top-k
  float* out_d;
  long long* out_i;
};

// One workgroup (1024 threads) per query.  Streams the query's keys through LDS in slices: the k best so far stay at the
// head of the list, up to LMAX - k new keys join them, a radix select keeps the k best again.  With a single slice
// (the normal case: ~1 500 candidates, or the 8192-row sample) this is one select.
// What the first version paid for (11 us per 8192-key threshold, 19 us per final selection) and what replaced it:
//   * candidates all share their sign / exponent / leading mantissa bits, so the first radix digits put EVERY key into one
//     histogram bin — thousands of LDS atomics on one address.  The bits common to all keys (AND vs OR) are skipped and the
//     first digit starts at the highest bit in which two keys differ;
//   * the bitonic sort's 28 barriers for 128 keys -> a rank sort (keys are unique: rank = number of larger keys), one barrier;
//   * the prefix sum over the candidate regions' counts by wave shuffles (2 barriers instead of 20).
template <int NT>      // threads per workgroup: 1024; 256 for the 512-key threshold selection (cheaper barriers: 5 us)
__global__ __launch_bounds__(NT) void select_kernel(SelArgs p) {
  __shared__ u64 lst[LMAX];
  __shared__ u64 srt[KMAX];
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_need, sh_cnt, sh_done;
  __shared__ u64 sh_prefix;
  __shared__ u64 red_or[NT / 64], red_and[NT / 64];
  __shared__ unsigned wsum[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = blockIdx.x;
  const u64* src = p.keys + (long long)q * p.kstride;
  // ---- regions: this thread owns regions [r0, r1); base = number of keys in the regions before them
  int r0 = 0, r1 = 0;
  long long base = 0, total = p.fixed_count;
  if (p.counts) {
    const unsigned* cnt = p.counts + (long long)q * p.nregions;
    const int rpt = (p.nregions + NT - 1) / NT;
    r0 = min(tid * rpt, p.nregions); r1 = min(r0 + rpt, p.nregions);
    unsigned mine = 0;
    for (int r = r0; r < r1; ++r) mine += cnt[r];
    unsigned incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
      const unsigned v = wsum[i];
      before += i < wv ? v : 0u;
      all += v;
    }
    base = (long long)before + incl - mine;
    total = all;
  }

  long long done = 0;
  int have = 0;                          // keys at the head of lst carried over from the previous slice
  u64 T = 0ull;
  int nsel = 0;                          // valid entries in srt
  bool first = true;
  while (first || done < total) {
    first = false;
    const int take = (int)min((long long)(LMAX - have), total - done);
    u64 vor = 0ull, vand = ~0ull;        // over the keys this thread brings in (and, below, the carried ones)
    if (!p.counts) {
      for (int i = tid; i < take; i += NT) {
        const u64 x = src[done + i];
        lst[have + i] = x; vor |= x; vand &= x;
      }
    } else {                             // keys with ordinals [done, done + take) out of this thread's regions
      const unsigned* cnt = p.counts + (long long)q * p.nregions;
      long long o = base;
      for (int r = r0; r < r1 && o < done + take; ++r) {
        const unsigned n = cnt[r];
        if (o + n > done) {
          const u64* reg = src + (long long)r * p.region_cap;
          for (unsigned e = (unsigned)max(0ll, done - o); e < n && o + e < done + take; ++e) {
            const u64 x = reg[e];
            lst[have + (int)(o + e - done)] = x; vor |= x; vand &= x;
          }
        }
        o += n;
      }
    }
    done += take;
    const int L = have + take;
    for (int i = tid; i < have; i += NT) { const u64 x = lst[i]; vor |= x; vand &= x; }
    if (L <= p.k) {
      __syncthreads();
      for (int i = tid; i < p.kpad; i += NT) srt[i] = i < L ? lst[i] : 0ull;
      nsel = L;
      T = 0ull;
    } else {
      // ---- bits shared by all L keys: OR / AND over the workgroup
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) { vor |= shfl64(vor, lane ^ m); vand &= shfl64(vand, lane ^ m); }
      if (lane == 0) { red_or[wv] = vor; red_and[wv] = vand; }
      if (tid == 0) { sh_need = (unsigned)p.k; sh_done = 0u; }
      __syncthreads();
      u64 aor = 0ull, aand = ~0ull;
#pragma unroll
      for (int i = 0; i < NT / 64; ++i) { aor |= red_or[i]; aand &= red_and[i]; }
      const u64 diff = aor ^ aand;
      // ---- radix select of the k-th largest composite, 8 bits per pass from the highest bit in which two keys differ.
      // Early exit: once the bin that holds the k-th element contains EXACTLY the number of elements still needed,
      // every element with that prefix is selected and the remaining low bits need not be resolved (with distinct
      // scores this happens after 2-3 passes; only exact score ties ever reach the index bits).
      if (diff == 0ull) {                // L copies of one key (only empty slots can repeat): that key is the k-th best
        T = aand;
      } else {
        const int hb = 63 - __builtin_clzll(diff);
        u64 mask = hb == 63 ? 0ull : ~((2ull << hb) - 1ull);
        if (tid == 0) sh_prefix = aand & mask;
        int sh = max(hb - 7, 0), width = hb - sh + 1;
        while (true) {
          if (tid < 256) hist[tid] = 0u;
          __syncthreads();
          if (sh_done) break;
          const u64 prefix = sh_prefix;
          const unsigned need = sh_need;
          const unsigned dm = (1u << width) - 1u;
          for (int i = tid; i < L; i += NT) {
            const u64 x = lst[i];
            if ((x & mask) == prefix) atomicAdd(&hist[(unsigned)(x >> sh) & dm], 1u);
          }
          __syncthreads();
          // wave 0 scans the 256 bins from the top: lane i owns bins 255-4i .. 252-4i
          if (tid < 64) {
            unsigned h[4], s4 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * tid - j]; s4 += h[j]; }
            unsigned incl = s4;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
              const unsigned v = __shfl_up(incl, off, 64);
              if (tid >= off) incl += v;
            }
            unsigned run = incl - s4;                       // elements in bins above this lane's first bin
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (run < need && need <= run + h[j]) {
                sh_need = need - run;
                sh_prefix = prefix | ((u64)(255 - 4 * tid - j) << sh);
                if (h[j] == need - run) sh_done = 1u;       // the whole bin is selected
              }
              run += h[j];
            }
          }
          mask |= ((u64)dm << sh);
          __syncthreads();
          if (sh == 0) break;
          const int nsh = max(sh - 8, 0);
          width = sh - nsh;
          sh = nsh;
        }
        T = sh_prefix;                   // every selected key is >= T, exactly k keys are
      }
      if (tid == 0) sh_cnt = 0u;
      __syncthreads();
      for (int i = tid; i < L; i += NT) {
        const u64 x = lst[i];
        if (x > T) srt[atomicAdd(&sh_cnt, 1u)] = x;
      }
      __syncthreads();
      const int cgt = (int)sh_cnt;       // k, or fewer when keys equal T bit for bit (one real key, or repeated empty slots)
      for (int i = cgt + tid; i < p.kpad; i += NT) srt[i] = i < p.k ? T : 0ull;
      nsel = p.k;
    }
    __syncthreads();
    if (done < total) {                  // carry the k best into the next slice
      for (int i = tid; i < nsel; i += NT) lst[i] = srt[i];
      have = nsel;
      __syncthreads();
    }
  }

  if (p.thresh) {                        // threshold mode: the sample's k-th best is a lower bound of the corpus' k-th best
    if (tid == 0) p.thresh[q] = nsel < p.k ? 0ull : T;
    return;
  }
  // ---- rank sort, descending: real keys are unique, so a key's rank is the number of larger keys; empty slots (0) go last
  for (int i = tid; i < p.k; i += NT) {
    const long long o = (long long)q * p.k + i;
    if (i >= nsel) { p.out_d[o] = -FLT_MAX; p.out_i[o] = -1; }     // faiss' padding for k > ntotal
  }
  for (int i = tid; i < nsel; i += NT) {
    const u64 x = srt[i];
    int rank = 0;
    if (x == 0ull) {                     // an empty slot inside the selection (dense input with rows >= N): after every real key,
      for (int j = 0; j < nsel; ++j) rank += (srt[j] != 0ull) || (j < i);   // ordered among themselves by position
    } else {
      for (int j = 0; j < nsel; ++j) rank += srt[j] > x;
    }
    const long long o = (long long)q * p.k + rank;
    if (x == 0ull) { p.out_d[o] = -FLT_MAX; p.out_i[o] = -1; }
    else { p.out_d[o] = okey_inv((unsigned)(x >> 32)); p.out_i[o] = (long long)(~(unsigned)(x & 0xffffffffull)); }
  }
}

// ------------------------------------------------------------------ selection through the row groups' maxima (two-launch call)
// The scan left every score [Q, npad] and the best composite of every group of 16 rows [Q, gstride] (ngroups <= LMAX, k <= 128).
// The k-th best GROUP maximum T is a lower bound of the answer's k-th best composite (k different rows reach it), and — keys
// being unique — exactly k groups have a maximum >= T: every row of the answer lives in one of those k groups.  So the
// selection reads ngroups keys, then 16 k scores, and never more: no sample launch, no threshold launch, no candidate regions,
// and the worst case is the common case (a corpus that defeats a strided sample does not exist for this form).
struct GroupSelArgs {
  const u64* gmax;        // [Q, gstride]
  long long gstride;
  int ngroups;
  const float* scores;    // [Q, npad]
  long long npad, N;
  int k;
  float* out_d;
  long long* out_i;
};

struct KthScratch {
  unsigned hist[256];
  unsigned need, done;
  u64 prefix;
  u64 red_or[16], red_and[16], red_min[16];
};

// the k-th largest of more than k unique keys spread over the workgroup's threads: T with exactly k keys >= T (the radix select of
// select_kernel: bits common to all keys skipped, 8 bits per pass, early exit when the bin that holds the k-th key holds exactly what
// is still needed).  each(f) calls f(x) for every key the thread holds (registers or LDS); vor / vand = OR / AND over those keys.
// Called by all NT threads; ends behind a barrier.
template <int NT, class Each>
__device__ __forceinline__ u64 kth_largest(Each each, int k, KthScratch& s, u64 vor, u64 vand) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { vor |= shfl64(vor, lane ^ m); vand &= shfl64(vand, lane ^ m); }
  if (lane == 0) { s.red_or[wv] = vor; s.red_and[wv] = vand; }
  if (tid == 0) { s.need = (unsigned)k; s.done = 0u; }
  __syncthreads();
  u64 aor = 0ull, aand = ~0ull;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) { aor |= s.red_or[i]; aand &= s.red_and[i]; }
  const u64 diff = aor ^ aand;
  if (diff == 0ull) { __syncthreads(); return aand; }
  const int hb = 63 - __builtin_clzll(diff);
  u64 mask = hb == 63 ? 0ull : ~((2ull << hb) - 1ull);
  if (tid == 0) s.prefix = aand & mask;
  int sh = max(hb - 7, 0), width = hb - sh + 1;
  while (true) {
    if (tid < 256) s.hist[tid] = 0u;
    __syncthreads();
    if (s.done) break;
    const u64 prefix = s.prefix;
    const unsigned need = s.need;
    const unsigned dm = (1u << width) - 1u;
    // wave-aggregated: when all of a wave's keys under the prefix fall into ONE bin (a query with a near-duplicate in the corpus puts
    // one key far above the rest: the digits between them hold every other key in a single bin — 7 000 atomics on one LDS address,
    // 3-4 us per pass), one lane adds their count
    // each() may call this from divergent code (`if (r[j]) f(r[j])`, a ragged `for i < C`): __ballot then covers the ACTIVE lanes only,
    // `leader` is the first lane of that ballot and therefore active — the one constraint __shfl has on its source lane
    each([&](u64 x) {
      const bool in = (x & mask) == prefix;
      const unsigned bin = (unsigned)(x >> sh) & dm;
      const u64 act = __ballot(in);
      if (act != 0ull) {
        const int leader = __ffsll((long long)act) - 1;
        const unsigned b0 = (unsigned)__shfl((int)bin, leader, 64);
        if (__ballot(in && bin == b0) == act) {
          if (lane == leader) atomicAdd(&s.hist[b0], (unsigned)__popcll(act));
        } else if (in) {
          atomicAdd(&s.hist[bin], 1u);
        }
      }
    });
    __syncthreads();
    if (tid < 64) {                       // wave 0 scans the 256 bins from the top: lane i owns bins 255-4i .. 252-4i
      unsigned h[4], s4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = s.hist[255 - 4 * tid - j]; s4 += h[j]; }
      unsigned incl = s4;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off, 64);
        if (tid >= off) incl += v;
      }
      unsigned run = incl - s4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (run < need && need <= run + h[j]) {
          s.need = need - run;
          s.prefix = prefix | ((u64)(255 - 4 * tid - j) << sh);
          if (h[j] == need - run) s.done = 1u;
        }
        run += h[j];
      }
    }
    mask |= ((u64)dm << sh);
    __syncthreads();
    if (sh == 0) break;
    const int nsh = max(sh - 8, 0);
    width = sh - nsh;
    sh = nsh;
  }
  const u64 T = s.prefix;
  __syncthreads();                        // the scratch may be reused
  return T;
}

constexpr int GSEL_NT = 1024;
constexpr int GSEL_KMAX = 128;
constexpr int GSEL_R = LMAX / GSEL_NT;    // group maxima per thread, in registers
constexpr int GSEL_RANK_MAX = 512;        // candidates up to which ranks are counted directly (no second radix select)
// M: row groups per key ("super-group", a power of two <= 8): a thread folds M consecutive group maxima into each of its registers, so
// 8192 keys cover 8192 M groups = 131 072 M rows; exactly k super-groups reach the bound and their 16 M k rows are the candidates
// (LDS for all of them: 128 KiB at M = 8, N <= 1 048 576).
template <int M>
__global__ __launch_bounds__(GSEL_NT) void select_groups_kernel(GroupSelArgs p) {
  // gfx950 only (160 KiB of LDS per workgroup): M = 8 takes 128 KiB for the candidates alone — checked here because the four instantiations
  // are compiled unconditionally
  static_assert(M == 1 || M == 2 || M == 4 || M == 8, "row groups per key: a power of two <= 8");
  static_assert(sizeof(u64) * (16 * M * GSEL_KMAX + GSEL_KMAX) + sizeof(unsigned) * (GSEL_KMAX + 3) + sizeof(KthScratch) <= 160 * 1024,
                "select_groups_kernel: LDS budget of gfx950 exceeded");
  __shared__ u64 cand[16 * M * GSEL_KMAX];   // the rows of the k best super-groups that reach T
  __shared__ u64 srt[GSEL_KMAX];
  __shared__ unsigned grp[GSEL_KMAX];
  __shared__ KthScratch ks;
  __shared__ unsigned n_grp, n_cand, n_sel;
  const int tid = threadIdx.x, q = blockIdx.x;
  const int L = p.ngroups, k = p.k;
  const u64* src = p.gmax + (long long)q * p.gstride;
  // every load of the thread in flight at once (a loop of load -> use would pay the memory latency GSEL_R times)
  u64 r[GSEL_R];
#pragma unroll
  for (int j = 0; j < GSEL_R; ++j) {
    u64 best = 0ull;                      // 0 = no key (a real composite is never 0)
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const int gi = (tid + j * GSEL_NT) * M + i;
      const u64 x = gi < L ? src[gi] : 0ull;
      best = x > best ? x : best;
    }
    r[j] = best;
  }
  if (tid == 0) { n_grp = 0u; n_cand = 0u; n_sel = 0u; }
  // Keys that cannot be among the k best leave the selection here: every thread that holds keys holds its own maximum, at least
  // SAMPLE_GROUPS + 1 > k threads do, so the SMALLEST of the threads' maxima is a lower bound of the k-th best key.  What this buys
  // is the radix select's first digit: it starts at the highest bit in which two keys differ, and ONE group of 16 all-negative scores
  // (2^-16 per group: one query in nine at N = 118 287) or a NaN row puts that at the sign bit — 7 000 keys in two or three bins, 3 passes and
  // thousands of LDS atomics per address (+6.5 us on the call).  With the low outliers gone the digit starts inside the exponent.
  {
    u64 tmax = 0ull;
#pragma unroll
    for (int j = 0; j < GSEL_R; ++j) tmax = r[j] > tmax ? r[j] : tmax;
    u64 m = tmax ? tmax : ~0ull;          // threads without keys do not vote
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const u64 v = shfl64(m, (tid & 63) ^ o); m = v < m ? v : m; }
    if ((tid & 63) == 0) ks.red_min[tid >> 6] = m;
    __syncthreads();
    u64 lb = ~0ull;
#pragma unroll
    for (int i = 0; i < GSEL_NT / 64; ++i) { const u64 v = ks.red_min[i]; lb = v < lb ? v : lb; }
#pragma unroll
    for (int j = 0; j < GSEL_R; ++j) r[j] = r[j] < lb ? 0ull : r[j];
  }
  u64 vor = 0ull, vand = ~0ull;
#pragma unroll
  for (int j = 0; j < GSEL_R; ++j)
    if (r[j]) { vor |= r[j]; vand &= r[j]; }
  const u64 T = kth_largest<GSEL_NT>([&](auto f) {
#pragma unroll
    for (int j = 0; j < GSEL_R; ++j)
      if (r[j]) f(r[j]);
  }, k, ks, vor, vand);                   // more than SAMPLE_GROUPS >= k keys
#pragma unroll
  for (int j = 0; j < GSEL_R; ++j)
    if (r[j] >= T && r[j]) grp[atomicAdd(&n_grp, 1u)] = ((~(unsigned)(r[j] & 0xffffffffull)) >> 4) / M;   // the super-group of the key's row: exactly k of them
  __syncthreads();
  const float* sc = p.scores + (long long)q * p.npad;
  constexpr int RPS = 16 * M;             // rows per super-group
  constexpr int GB = M == 1 ? 2 : 4;      // loads of a thread in flight (16 k <= 2048 scores at M = 1: both)
  for (int i0 = 0; i0 < RPS * k; i0 += GB * GSEL_NT) {
    float v[GB];
    long long row[GB];
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int i = i0 + tid + j * GSEL_NT;
      row[j] = i < RPS * k ? (long long)grp[i / RPS] * RPS + (i % RPS) : p.N;
      v[j] = row[j] < p.N ? sc[row[j]] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < GB; ++j)
      if (row[j] < p.N) {
        const u64 x = composite(v[j], (unsigned)row[j]);
        if (x >= T) cand[atomicAdd(&n_cand, 1u)] = x;
      }
  }
  __syncthreads();
  const int C = (int)n_cand;              // >= k: the k group maxima are among them
  if (C <= GSEL_RANK_MAX) {
    // a candidate's rank = the number of larger candidates (keys are unique): ranks below k are the answer, already in order
    if (tid < C) {
      const u64 x = cand[tid];
      int rank = 0;
      for (int j = 0; j < C; ++j) rank += cand[j] > x;
      if (rank < k) {
        const long long o = (long long)q * k + rank;
        p.out_d[o] = okey_inv((unsigned)(x >> 32));
        p.out_i[o] = (long long)(~(unsigned)(x & 0xffffffffull));
      }
    }
    return;
  }
  // many candidates (the answer's groups are full of high scorers): a second radix select, then the rank sort over k keys
  u64 cor = 0ull, cand_and = ~0ull;
  for (int i = tid; i < C; i += GSEL_NT) { cor |= cand[i]; cand_and &= cand[i]; }
  const u64 T2 = kth_largest<GSEL_NT>([&](auto f) {
    for (int i = tid; i < C; i += GSEL_NT) f(cand[i]);
  }, k, ks, cor, cand_and);
  for (int i = tid; i < C; i += GSEL_NT) {
    const u64 x = cand[i];
    if (x >= T2) srt[atomicAdd(&n_sel, 1u)] = x;
  }
  __syncthreads();
  for (int i = tid; i < k; i += GSEL_NT) {
    const u64 x = srt[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += srt[j] > x;
    const long long o = (long long)q * k + rank;
    p.out_d[o] = okey_inv((unsigned)(x >> 32));
    p.out_i[o] = (long long)(~(unsigned)(x & 0xffffffffull));
  }
}

struct L2Args { float* x; long long rows; int d; };
__global__ __launch_bounds__(256) void l2norm_kernel(L2Args p) {
  const int w = wave_id(), l = lane_id();
  const long long row = (long long)blockIdx.x * 4 + w;
  if (row >= p.rows) return;
  float* xr = p.x + row * p.d;
  // x / x.norm(dim=-1): sequential-in-lane then butterfly; fp32
  float ss = 0.f;
  for (int c = l; c < p.d; c += 64) ss += xr[c] * xr[c];
  ss = wave_sum(ss);
  const float nrm = sqrtf(ss);
  for (int c = l; c < p.d; c += 64) xr[c] = xr[c] / nrm;
}

// launch geometry of the scan: a multiple of 8 * ntile workgroups (the tiles of a row range share an XCD)
inline int scan_grid(long long niter, int ntile) {
  const long long unit = 8 * ntile;
  long long want = (niter + 3) / 4 * ntile;                 // one wave per group
  want = (want + unit - 1) / unit * unit;
  // workgroups at most (speed only; 0 = the measured default: two resident workgroups per CU, each wave walks many groups with
  // the next group's first chunk prefetched — scan at Q = 16, N = 118 287: 40.2 us with 512, 41.8 with 1024, 46.9 with 1856)
  const int opt = drag_opt(DRAG_OPT_TOPK_GRID);
  long long cap = (long long)(min(opt > 0 ? opt : 512, 2048) / unit) * unit;
  if (cap < unit) cap = unit;                               // a "topk_grid" below one unit (a zero grid, and a division by zero downstream)
  return (int)(want < unit ? unit : (want > cap ? cap : want));
}
template <int NBUF, int QT>
int launch_scan_n(ScanArgs& sa, hipStream_t st) {
  const int lds = QT * (sa.d / 64) * 4096 + 4 * NBUF * 4096;
  return drag_launch<ip_scan_kernel<NBUF, QT>>(dim3(scan_grid(sa.niter, sa.ntile)), 256, lds, st, sa);      // (d >= 768: more than 64 KiB)
}
// Query tiles per workgroup ("topk_qt"; 0 = the default, 1): 1 — every tile of 16 queries gets its own workgroup and the tiles of a
// row range share the corpus through their XCD's L2 (two workgroups per CU); 2 / 4 — a workgroup keeps that many tiles in LDS and
// feeds each corpus fragment to all of them (one workgroup per CU: the form the round-2 verdict suggested).  Measured, scan only,
// same box: N = 118 287: Q = 64 85.8 us (1) vs 106.4 (2) vs 110.8 (4), Q = 32 50.3 vs 64.2; N = 1 000 000: Q = 64 754 vs 790 vs 701,
// Q = 32 442 vs 461 vs 468 — with one workgroup (4 waves) per CU nothing hides a wave's LDS-DMA latency, which costs more than
// the L2 re-reads of the sibling form; only the longest, matrix-core-bound launch gains (7 %).  The default stays 1.
// scan_qt(Q, d) is what the launcher and the candidate-region sizing both use.
inline int scan_qt(int Q, int d) {
  const int opt = DRAG_EXP ? drag_opt(DRAG_OPT_TOPK_QT) : 0;
  int qt = opt > 0 ? opt : 1;
  if (qt != 1 && qt != 2 && qt != 4) qt = 1;
  while (qt > 1 && (qt * (d / 64) * 4096 + 4 * 2 * 4096 > 160 * 1024 || 16 * (qt / 2) >= Q)) qt >>= 1;    // LDS; no empty tiles
  return qt;
}
// Ring depth 2 (one chunk ahead) is the measured default: 8 waves per CU hide each other's latency, a third buffer per wave
// (80 KiB per workgroup, still two per CU) measured -3...-7 % at Q <= 16 and +2 % at Q = 64; putting a whole group in flight
// (8 buffers, 160 KiB, one workgroup per CU) for the launches that give a wave a single group (the 512-group sample) made
// that launch slower (7.2-8.4 -> 9.6-11.2 us): it is bound by the workgroup's start-up (32 KiB query image), not by the stream.
int launch_scan(ScanArgs& sa, hipStream_t st) {
  const int qt = scan_qt(sa.Q, sa.d);
  sa.ntile = ((sa.Q + 15) / 16 + qt - 1) / qt;
#if DRAG_EXP
  if (qt == 4) return launch_scan_n<2, 4>(sa, st);
  if (qt == 2) return launch_scan_n<2, 2>(sa, st);
#endif
  if (drag_opt(DRAG_OPT_TOPK_DEPTH) == 3) return launch_scan_n<3, 1>(sa, st);
  if (sa.d == 512 && drag_opt(DRAG_OPT_TOPK_QREG) != 1) {      // CLIP's width: the query tile in registers (ip_scan_q512_kernel)
    hipLaunchKernelGGL(ip_scan_q512_kernel, dim3(scan_grid(sa.niter, sa.ntile)), dim3(256), 0, st, sa);
    DRAG_LAUNCH_CHECK();
    return 0;
  }
  return launch_scan_n<2, 1>(sa, st);
}

// workspace layout: thresholds [64] u64 | region counters [64][MAXREG] u32 | sample keys [64][8192] u64 |
//                   candidates [min(Q,64)][ceil16(N) + 16 * MAXREG] u64 (one region per scanning wave, MAXREG = 2048 workgroups x 4)
inline long long ceil16(long long n) { return (n + 15) / 16 * 16; }
constexpr long long MAXREG = 8192;
inline long long cand_stride(long long N) { return ceil16(N) + 16 * MAXREG; }
// queries per corpus pass: 64, fewer when their candidate regions (room for ALL rows, 8 bytes each) would pass 1 GiB
inline int pass_queries(long long N) {
  int qp = 64;
  while (qp > 16 && (long long)qp * cand_stride(N) * 8 > (1ll << 30)) qp >>= 1;
  return qp;
}

}  // namespace

extern "C" int64_t drag_cosine_topk_workspace_bytes(int64_t N, int32_t Q) {
  if (N <= 0 || Q <= 0) return 0;
  const long long qp = Q < pass_queries(N) ? Q : pass_queries(N);
  return 64 * 8 + 64 * MAXREG * 4 + 64ll * SAMPLE_GROUPS * 16 * 8 + qp * cand_stride(N) * 8 + 256;
}

// scan only: scores[q, n] = <corpus[n], queries[q]> for Q <= 64 queries in ONE pass over the corpus, row stride
// npad = ceil64(N) floats.  The same kernel, launch geometry and summation order as the scan inside drag_cosine_topk_f32
// (bench.py times the HBM-bound pass alone through this entry; tests compare it bit for bit with the oracle's score order).
extern "C" int drag_cosine_scores_f32(const float* corpus, const float* queries, int64_t N, int32_t d, int32_t Q,
                                      float* scores, void* stream) {
  DRAG_CHECK(corpus && queries && scores, "drag_cosine_scores_f32: null pointer");
  DRAG_CHECK(N > 0 && Q > 0 && Q <= 64, "drag_cosine_scores_f32: N > 0 and 1 <= Q <= 64 (one scan pass)");
  DRAG_CHECK(d > 0 && d % 64 == 0 && d <= 1024, "drag_cosine_scores_f32: d must be a multiple of 64, <= 1024");
  DRAG_CHECK(N < (1ll << 32) - 1, "drag_cosine_scores_f32: N must fit 32 bits");
  ScanArgs sa{};
  sa.corpus = corpus; sa.queries = queries; sa.N = N; sa.d = d; sa.Q = Q; sa.ntile = (Q + 15) / 16;
  sa.mode = SCAN_SCORES; sa.gstride = 1; sa.niter = (N + 15) / 16;
  sa.scores = scores; sa.npad = (N + 63) / 64 * 64;
  return launch_scan(sa, (hipStream_t)stream);
}

extern "C" int drag_cosine_topk_f32(const float* corpus, const float* queries, int64_t N, int32_t d, int32_t Q,
                                    int32_t k, float* out_d, int64_t* out_i, void* workspace, void* stream) {
  DRAG_CHECK(corpus && queries && out_d && out_i && workspace, "drag_cosine_topk_f32: null pointer");
  DRAG_CHECK(N > 0 && Q > 0, "drag_cosine_topk_f32: N and Q must be positive");
  DRAG_CHECK(d > 0 && d % 64 == 0 && d <= 1024, "drag_cosine_topk_f32: d must be a multiple of 64, <= 1024");
  DRAG_CHECK(k > 0 && k <= KMAX, "drag_cosine_topk_f32: 1 <= k <= 2048");
  DRAG_CHECK(N < (1ll << 32) - 1, "drag_cosine_topk_f32: N must fit 32 bits");
  hipStream_t st = (hipStream_t)stream;
  u64* thresh = (u64*)workspace;
  unsigned* counts = (unsigned*)(thresh + 64);
  u64* sample = (u64*)(counts + 64 * MAXREG);
  u64* cand = sample + 64ll * SAMPLE_GROUPS * 16;
  const long long ngroups = (N + 15) / 16;
  const long long cstride = cand_stride(N);
  int kpad = 1;
  while (kpad < k) kpad <<= 1;

  const int qpass = pass_queries(N);
  for (int q0 = 0; q0 < Q; q0 += qpass) {
    const int qn = min(qpass, Q - q0);
    ScanArgs sa{};
    sa.corpus = corpus; sa.queries = queries + (long long)q0 * d; sa.N = N; sa.d = d; sa.Q = qn; sa.ntile = (qn + 15) / 16;
    SelArgs se{};
    se.k = k; se.kpad = kpad;
    // two launches through the group maxima (select_groups_kernel): every group maximum fits one workgroup's LDS and k groups
    // of 16 rows bound the candidates; "topk_path" = 1 forces the sampled-threshold form below (A/B, tests)
    // Beyond 131 072 rows (more than one row group per key) the [Q, N] scores the scan has to write start to cost what the saved launches
    // gave: measured (profiles/r04_topk_two_launch_ab.log) N = 300 000: Q = 1 -9 %, Q = 4 -5 %, Q = 16 -1 %, Q = 32 +1 %; N = 1 000 000:
    // Q = 1 -0.5 %, Q = 4 +2 %, Q = 16 +6 % — so by policy only up to 524 288 rows and 4 queries per pass; "topk_path" = 2 takes
    // it wherever it applies (tests, measurements)
    const int path_opt = drag_opt(DRAG_OPT_TOPK_PATH);
    const bool group_ok = ngroups > SAMPLE_GROUPS && ngroups <= 8 * LMAX && k <= GSEL_KMAX;
    const bool group_path = group_ok && path_opt != 1 && (path_opt == 2 || ngroups <= LMAX || (ngroups <= 4 * LMAX && qn <= 4));
    if (group_path) {
      // workspace reuse: a query's candidate region (8 bytes per row + 1 MiB) holds its scores (4 bytes per row) and, behind them, its
      // group maxima (half a byte per row)
      u64* gm = (u64*)((char*)cand + 4 * ceil16(N));
      sa.mode = SCAN_SCORES_GMAX; sa.gstride = 1; sa.niter = ngroups; sa.keys = gm; sa.kstride = cstride;
      sa.scores = (float*)cand; sa.npad = 2 * cstride;
      if (int rc = launch_scan(sa, st)) return rc;
      GroupSelArgs ga{};
      ga.gmax = gm; ga.gstride = cstride; ga.ngroups = (int)ngroups; ga.scores = sa.scores; ga.npad = sa.npad; ga.N = N; ga.k = k;
      ga.out_d = out_d + (long long)q0 * k; ga.out_i = (long long*)out_i + (long long)q0 * k;
      const long long per_key = (ngroups + LMAX - 1) / LMAX;             // row groups per key: 1 up to 131 072 rows, 8 up to 1 048 576
      if (per_key <= 1) hipLaunchKernelGGL(select_groups_kernel<1>, dim3(qn), dim3(GSEL_NT), 0, st, ga);
      else if (per_key <= 2) hipLaunchKernelGGL(select_groups_kernel<2>, dim3(qn), dim3(GSEL_NT), 0, st, ga);
      else if (per_key <= 4) hipLaunchKernelGGL(select_groups_kernel<4>, dim3(qn), dim3(GSEL_NT), 0, st, ga);
      else hipLaunchKernelGGL(select_groups_kernel<8>, dim3(qn), dim3(GSEL_NT), 0, st, ga);
      DRAG_LAUNCH_CHECK();
      continue;
    }
    if (ngroups <= SAMPLE_GROUPS) {
      // small corpus: every composite goes to the candidate list at its own slot (no sample, no atomics)
      sa.mode = SCAN_KEYS_DENSE; sa.gstride = 1; sa.niter = ngroups; sa.keys = cand; sa.kstride = cstride;
      if (int rc = launch_scan(sa, st)) return rc;
      se.keys = cand; se.kstride = cstride; se.counts = nullptr; se.fixed_count = ngroups * 16;
    } else {
      // 1) the strided sample -> 2) a lower bound of the answer's k-th best composite per query = the filter threshold.
      //    k <= 128: the BEST composite of each of the 512 sampled groups is kept (512 keys per query) and the k-th best of those
      //    group maxima is the bound — k different rows reach it, and it sits where the k-th best of all 8192 sampled rows does
      //    to within ~10 % more candidates (a row beats the bound with probability p, a group of 16 with 16 p), at 1/16 of the
      //    selection's input.  Larger k: every sampled row's composite, and their exact k-th best.
      const bool gmax = k <= 128 && !drag_opt(DRAG_OPT_TOPK_DENSE_SAMPLE);
      sa.mode = gmax ? SCAN_GROUP_MAX : SCAN_KEYS_DENSE; sa.gstride = ngroups / SAMPLE_GROUPS; sa.niter = SAMPLE_GROUPS; sa.keys = sample;
      sa.kstride = gmax ? SAMPLE_GROUPS : SAMPLE_GROUPS * 16;
      if (int rc = launch_scan(sa, st)) return rc;
      SelArgs sth = se;
      sth.keys = sample; sth.kstride = sa.kstride; sth.counts = nullptr; sth.fixed_count = sa.kstride;
      sth.thresh = thresh;
      if (gmax) hipLaunchKernelGGL(select_kernel<256>, dim3(qn), dim3(256), 0, st, sth);
      else hipLaunchKernelGGL(select_kernel<1024>, dim3(qn), dim3(1024), 0, st, sth);
      DRAG_LAUNCH_CHECK();
      // 3) the one pass over the corpus, keeping what can still make the top k: one candidate region per scanning wave,
      //    sized for every row the wave visits
      const int qt_ = scan_qt(sa.Q, sa.d);
      sa.ntile = ((sa.Q + 15) / 16 + qt_ - 1) / qt_;                       // (launch_scan sets the same value)
      const int grid = scan_grid(ngroups, sa.ntile);
      const long long nwaves = (long long)(grid / (8 * sa.ntile)) * 8 * 4;
      sa.mode = SCAN_KEYS_FILTER; sa.gstride = 1; sa.niter = ngroups; sa.keys = cand; sa.kstride = cstride;
      sa.thresh = thresh; sa.counts = counts; sa.nregions = (int)nwaves; sa.region_cap = 16 * ((ngroups + nwaves - 1) / nwaves);
      if (int rc = launch_scan(sa, st)) return rc;
      se.keys = cand; se.kstride = cstride; se.counts = counts; se.fixed_count = 0; se.nregions = sa.nregions; se.region_cap = sa.region_cap;
    }
    // 4) select + sort + decode on the candidates
    se.thresh = nullptr;
    se.out_d = out_d + (long long)q0 * k; se.out_i = (long long*)out_i + (long long)q0 * k;
    // 1024 threads also for ~1 500 candidates: measured 67.1 vs 73.2 us per Q = 16 call with 256 (the rank sort and the region walk
    // are per-thread loops); "topk_select" = 256 forces the small workgroup (measurements)
    const bool small = drag_opt(DRAG_OPT_TOPK_SELECT) == 256;
    if (small) hipLaunchKernelGGL(select_kernel<256>, dim3(qn), dim3(256), 0, st, se);
    else hipLaunchKernelGGL(select_kernel<1024>, dim3(qn), dim3(1024), 0, st, se);
    DRAG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int drag_l2_normalize_f32(float* x, int64_t rows, int32_t d, void* stream) {
  DRAG_CHECK(x && rows > 0 && d > 0, "drag_l2_normalize_f32: bad args");
  L2Args p{x, rows, d};
  hipLaunchKernelGGL(l2norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}
