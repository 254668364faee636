// jpeg_par.hip — the PARALLEL entropy route for sequential-Huffman JPEG files on gfx950: one file spread over many lanes and, above
// 32 KiB of entropy data, over several workgroups (arithmetic, states, fallback conditions: jpeg_par_core.h).  Opt-in
// (drag_jpeg_decode_rgb_par); everything behind the entropy stage — jpeg_idct_kernel, jpeg_color_kernel — and the lane kernels
// for progressive files and for files that fall back are jpeg.hip's, unchanged.
//
// Launches per batch, all on one stream, no host read-back between them:
//   jpeg_par_round_kernel  round 0                 grid (spans, files) x 256 lanes.  Lane t of workgroup w owns subsequence w * 256 + t of its
//                                                  file: speculative decode from the guess, then Jacobi iterations over the workgroup's own
//                                                  span behind barriers (exit states in LDS) until an iteration changes no exit.
//   jpeg_par_round_kernel  rounds 1..ROUND_CAP     the first lane of every span takes the exit the previous span had after the previous
//                                                  launch (two copies, alternating: no workgroup reads what another writes in the same
//                                                  launch) and the span iterates again.  A launch in which no exit changed anywhere in the
//                                                  file clears nothing in flags[round]: the file is settled and the later rounds return at once.
//   jpeg_par_scan_kernel                           one workgroup per file: settled? exclusive scan of the block-start and RSTn counts, the
//                                                  placement and end checks, route 1 (parallel) or 2 (fallback) + the lane kernel's mask + stats.
//   jpeg_par_write_kernel                          route-1 files: every lane decodes its subsequence once more from its settled entry and
//                                                  stores AC values and DC differences at the addresses the scan gave it.
//   jpeg_par_dc_kernel                             route-1 files, one workgroup per component: segmented inclusive sum of the DC differences.
//   jpeg_huffman_kernel (masked), jpeg_progressive_kernel, jpeg_idct_kernel, jpeg_color_kernel   (jpeg.hip)
// A file that falls back has written nothing (every fallback condition is known to the scan kernel), so its coefficients are still
// the zeros of the initial memset, which is what the lane kernel requires.
//
// Geometry (jpeg_par_core.h; exposed by drag_jpeg_par_geometry):
//   S = 128 bytes per subsequence.  A quality-75 file spends ~5 bits per symbol: ~200 symbols per lane and pass, enough to amortise the
//     entry / exit bookkeeping, while a 52-KiB 504x376 file still spreads over 400 lanes and a 1.5-MiB 2096x2800 frame over 12 000.  On
//     the host build the quality <= 95 files of the test matrix settle their spans in 2-12 local iterations at S = 128; S = 64 doubles
//     the iterations for the same bytes (synchronisation takes a number of BYTES, not of subsequences) and S = 256 halves the lanes.
//   SPAN = 256 subsequences (32 KiB) per workgroup = one per lane of a 256-lane workgroup: four waves share one copy of the code tables,
//     and a long-synchronising file (quality 100 holds ~170 bytes per MCU and was seen to need 100 subsequences) still settles inside
//     its span.  The local iteration cap is SPAN: a span of n subsequences is settled after at most n iterations whatever the data is.
//   ROUND_CAP = 4 cross-span launches.  Once every span is settled locally, round 1 hands every span its true entry unless a
//     synchronisation is still under way at a span's end, and the next round confirms: every file of the test matrix and the 2096x2800
//     frames use 2.  A file that needs more than 4 takes the fallback (correct, slow).
//   Tables: all lanes of a workgroup decode the same file, so the four code tables exist once per workgroup in LDS (11 KiB with 10-bit
//     direct tables: a quality-75 AC code is <= 10 bits for all but the rarest symbols), not once per lane as in jpeg_huffman_kernel.
//     The stream itself is read from global memory, one dependent load per symbol: staging the span's 32 KiB in LDS is the obvious next step
//     (a first attempt that read it back through generic pointers faulted on the device and is not part of this file).
//     No dynamically indexed private arrays: component constants are packed into scalars (JpegParFile).
#include "drag_common.h"
#include "jpeg_internal.h"
#include "jpeg_par_core.h"

namespace {

constexpr int S = JPEG_PAR_S, SPAN = JPEG_PAR_SPAN, ROUND_CAP = JPEG_PAR_ROUND_CAP, LB = JPEG_PAR_LB;
constexpr int HDR_WORDS = 16;            // per file: [0 .. ROUND_CAP] "an exit changed in this round", [8] route
constexpr int HDR_ROUTE = 8;
static_assert(ROUND_CAP + 1 <= HDR_ROUTE, "round flags overlap the route word");

struct ParArgs {
  JpegArgs j;
  const int64_t* par_plan;               // [n, 2]: first subsequence, first span of the file in the workspace arrays; -1 = not eligible
  int64_t tot_subs, tot_spans;
  int32_t* hdr;                          // [n, HDR_WORDS]
  int32_t* mask;                         // [n]: 1 = jpeg_huffman_kernel's file
  JpegParState* span_exit;               // [2, tot_spans]
  JpegParState* entry;                   // [tot_subs] ...
  JpegParState* exit;
  int32_t *nblocks, *nrst, *first_rst, *reason, *gbase;
  int32_t* stats;                        // [n, 4]
};

struct FileView {
  JpegParFile f;
  const uint8_t* d;
  int64_t sub0, span0, nsubs, nspans;
};

// false: not this route's file (status, progressive, too long, not planned, or planned outside the workspace)
__device__ __forceinline__ bool file_view(const ParArgs& a, int i, FileView* v) {
  const JpegInfo& o = a.j.info[i];
  const int64_t len = a.j.off[i + 1] - a.j.off[i];
  if (!jpeg_par_eligible(&o, len)) return false;
  v->sub0 = a.par_plan[2 * (int64_t)i]; v->span0 = a.par_plan[2 * (int64_t)i + 1];
  v->nsubs = jpeg_par_subseqs(o.scan_off, len, S); v->nspans = (v->nsubs + SPAN - 1) / SPAN;
  if (v->sub0 < 0 || v->span0 < 0 || v->sub0 + v->nsubs > a.tot_subs || v->span0 + v->nspans > a.tot_spans) return false;
  jpeg_par_file_init(&o, len, &v->f);
  v->d = a.j.data + a.j.off[i];
  return true;
}

template <int LB_, int NV_>
struct SharedTable {                     // one copy per workgroup, plain layout
  enum { LB = LB_, NV = NV_ };
  DRAG_LDS uint16_t* l;
  DRAG_LDS uint32_t* k;
  DRAG_LDS uint8_t* v;
  __device__ __forceinline__ DRAG_LDS uint16_t& lut(int i) const { return l[i]; }
  __device__ __forceinline__ DRAG_LDS uint32_t& limk(int i) const { return k[i]; }
  __device__ __forceinline__ DRAG_LDS uint8_t& val(int i) const { return v[i]; }
};
struct SharedTabs {                      // DC 0, DC 1, AC 0, AC 1
  DRAG_LDS uint16_t* L;
  DRAG_LDS uint32_t* K;
  DRAG_LDS uint8_t* V;
  __device__ __forceinline__ SharedTable<LB, 16> dc(int id) const { return {L + (id << LB), K + id * 17, V + id * 16}; }
  __device__ __forceinline__ SharedTable<LB, 256> ac(int id) const { return {L + ((2 + id) << LB), K + (2 + id) * 17, V + 32 + id * 256}; }
};
struct SharedNat {
  DRAG_LDS uint8_t* t;
  __device__ __forceinline__ uint8_t operator[](int k) const { return t[k]; }
};

struct TableLds {
  uint16_t lut[4 << LB];
  uint32_t limk[4 * 17];
  uint8_t val[32 + 512];
  uint8_t nat[80];
};

// lanes 0-3 build one table each; everybody waits
__device__ __forceinline__ SharedTabs build_tables(TableLds& m, const uint8_t* d, const JpegInfo& o) {
  const SharedTabs tab{(DRAG_LDS uint16_t*)m.lut, (DRAG_LDS uint32_t*)m.limk, (DRAG_LDS uint8_t*)m.val};
  const int t = threadIdx.x;
  if (t < 2) { if (o.dht_off[t] >= 0) jpeg_build_huff(d + o.dht_off[t], tab.dc(t)); }
  else if (t < 4) { if (o.dht_off[4 + t - 2] >= 0) jpeg_build_huff(d + o.dht_off[4 + t - 2], tab.ac(t - 2)); }
  else if (t >= 64 && t < 64 + 80) m.nat[t - 64] = (uint8_t)jpeg_natural_order(t - 64);
  __syncthreads();
  return tab;
}

__device__ __forceinline__ int64_t sub_end(const JpegParFile& f, int64_t s) {
  const int64_t e = f.scan_off + (s + 1) * (int64_t)S;
  return e < f.len ? e : f.len;
}

__global__ __launch_bounds__(SPAN) void jpeg_par_round_kernel(ParArgs a, int round) {
  __shared__ TableLds m;
  __shared__ JpegParState lds_exit[SPAN];
  const int i = blockIdx.y, w = blockIdx.x, t = threadIdx.x;
  FileView v;
  if (!file_view(a, i, &v) || w >= v.nspans) return;
  int32_t* hdr = a.hdr + (int64_t)i * HDR_WORDS;
  if (round > 0 && hdr[round - 1] == 0) return;                  // settled: no exit changed in the previous launch
  const JpegInfo& o = a.j.info[i];
  if (round == 0 && w == 0 && t < 64 * o.ncomp) {                // quantisation tables, natural order, for the IDCT kernel (as jpeg_huffman_kernel writes them)
    const int c = t >> 6, k = t & 63;
    const uint8_t* qt = v.d + o.dqt_off[o.tq[c]];
    a.j.qtab[((int64_t)i * 3 + c) * 64 + jpeg_natural_order(k)] = o.dqt_16[o.tq[c]] ? (uint16_t)jpeg_u16(qt + 2 * k) : (uint16_t)qt[k];
  }
  const uint8_t* d = v.d;
  const SharedTabs tab = build_tables(m, v.d, o);
  const SharedNat nat{(DRAG_LDS uint8_t*)m.nat};
  const int64_t s = (int64_t)w * SPAN + t;
  const bool valid = s < v.nsubs;
  const int64_t gs = v.sub0 + s;
  const int64_t end = sub_end(v.f, s);
  JpegParState entry = {0, JPAR_DEAD};
  JpegParResult r;
  r.exit = entry; r.nblocks = r.nrst = 0; r.first_rst = -1; r.reason = 0;
  bool dirty = false;
  if (valid) {
    if (round == 0) {
      entry = s == 0 ? jpeg_par_start(&v.f) : jpeg_par_guess(d, &v.f, s, S);
      jpeg_par_decode_subseq(d, &v.f, tab, nat, entry, end, JpegParNoSink(), &r);
      dirty = true;
    } else {
      entry = a.entry[gs]; r.exit = a.exit[gs];
    }
  }
  lds_exit[t] = r.exit;
  __syncthreads();
  bool changed = false, converged = false;
  for (int it = 0; it < JPEG_PAR_LOCAL_CAP; ++it) {
    JpegParState cand = entry;
    if (valid) {
      if (t > 0) cand = lds_exit[t - 1];
      else if (round > 0 && w > 0) cand = a.span_exit[(int64_t)((round - 1) & 1) * a.tot_spans + v.span0 + w - 1];
    }
    const bool need = valid && !jpeg_par_same(cand, entry);
    __syncthreads();                                             // everybody has read the previous iteration's exits
    int ch = 0;
    if (need) {
      const JpegParState old = r.exit;
      entry = cand;
      jpeg_par_decode_subseq(d, &v.f, tab, nat, entry, end, JpegParNoSink(), &r);
      lds_exit[t] = r.exit;
      ch = !jpeg_par_same(old, r.exit);
      dirty = true;
    }
    if (!__syncthreads_or(ch)) { converged = true; break; }
    changed = true;
  }
  if (valid && dirty) {
    a.entry[gs] = entry; a.exit[gs] = r.exit;
    a.nblocks[gs] = r.nblocks; a.nrst[gs] = r.nrst; a.first_rst[gs] = r.first_rst; a.reason[gs] = r.reason;
  }
  const int64_t left = v.nsubs - (int64_t)w * SPAN;
  if (t == (left < SPAN ? (int)left : SPAN) - 1) a.span_exit[(int64_t)(round & 1) * a.tot_spans + v.span0 + w] = r.exit;
  if (t == 0) {
    if (round == 0) changed = v.nspans > 1 || !converged;
    if (changed) hdr[round] = 1;
  }
}

__global__ __launch_bounds__(256) void jpeg_par_scan_kernel(ParArgs a) {
  __shared__ long long sb[256], sr[256];
  __shared__ long long tot[2];
  __shared__ int why;
  const int i = blockIdx.x, t = threadIdx.x;
  FileView v;
  if (!file_view(a, i, &v)) {
    if (t == 0) {
      a.mask[i] = 1;                                             // the lane kernels treat the file as drag_jpeg_decode_rgb does
      for (int k = 0; k < 4; ++k) a.stats[(int64_t)i * 4 + k] = 0;
    }
    return;
  }
  int32_t* hdr = a.hdr + (int64_t)i * HDR_WORDS;
  int rounds = -1;
  for (int r = ROUND_CAP; r >= 0; --r) if (hdr[r] == 0) rounds = r;
  const int64_t chunk = (v.nsubs + 255) / 256;
  const int64_t s0 = t * chunk < v.nsubs ? t * chunk : v.nsubs, s1 = s0 + chunk < v.nsubs ? s0 + chunk : v.nsubs;
  long long nb = 0, nr = 0;
  for (int64_t s = s0; s < s1; ++s) { nb += a.nblocks[v.sub0 + s]; nr += a.nrst[v.sub0 + s]; }
  sb[t] = nb; sr[t] = nr;
  if (t == 0) why = 0;
  __syncthreads();
  if (t == 0) {
    long long g = 0, r = 0;
    for (int k = 0; k < 256; ++k) { const long long b = sb[k], q = sr[k]; sb[k] = g; sr[k] = r; g += b; r += q; }
    tot[0] = g; tot[1] = r;
  }
  __syncthreads();
  long long g = sb[t], rs = sr[t];
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t gsub = v.sub0 + s;
    JpegParResult r;
    r.nblocks = a.nblocks[gsub]; r.nrst = a.nrst[gsub]; r.first_rst = a.first_rst[gsub]; r.reason = a.reason[gsub];
    a.gbase[gsub] = (int32_t)(g < v.f.total_blocks ? g : v.f.total_blocks);     // (the sink stores nothing at or past total_blocks)
    const int bad = jpeg_par_check_place(&v.f, &r, g, rs);
    if (bad) atomicMax(&why, bad);
    g += r.nblocks; rs += r.nrst;
  }
  __syncthreads();
  if (t == 0) {
    int reason = rounds < 0 ? JPAR_ROUND_CAP : why;
    if (!reason) reason = jpeg_par_check_end(v.d, &v.f, a.exit[v.sub0 + v.nsubs - 1], tot[0], tot[1]);
    const int route = reason ? 2 : 1;
    hdr[HDR_ROUTE] = route;
    a.mask[i] = reason ? 1 : 0;
    if (!reason) a.j.scan_status[i] = 0;                         // < 8 padding bits, then EOI inside the file
    int32_t* st = a.stats + (int64_t)i * 4;
    st[0] = route; st[1] = rounds < 0 ? ROUND_CAP : rounds; st[2] = (int32_t)v.nsubs; st[3] = reason;
  }
}

struct CoefSink {                        // g = gbase + ordinal -> the block's address, looked up once per block; nothing outside the file's planned blocks
  const JpegParFile* f;
  int16_t* coef;
  int64_t gbase;
  int cur;
  int16_t* blk;
  __device__ __forceinline__ void operator()(int ord, int nat, int val) {
    if (ord != cur) {
      cur = ord;
      const int64_t g = gbase + ord;
      blk = (g >= 0 && g < f->total_blocks) ? coef + jpeg_par_block_offset(f, g) : nullptr;
    }
    if (blk) blk[nat] = (int16_t)val;
  }
};

__global__ __launch_bounds__(SPAN) void jpeg_par_write_kernel(ParArgs a) {
  __shared__ TableLds m;
  const int i = blockIdx.y, w = blockIdx.x, t = threadIdx.x;
  FileView v;
  if (!file_view(a, i, &v) || w >= v.nspans) return;
  if (a.hdr[(int64_t)i * HDR_WORDS + HDR_ROUTE] != 1) return;
  const uint8_t* d = v.d;
  const SharedTabs tab = build_tables(m, v.d, a.j.info[i]);
  const SharedNat nat{(DRAG_LDS uint8_t*)m.nat};
  const int64_t s = (int64_t)w * SPAN + t;
  if (s >= v.nsubs) return;
  JpegParResult r;
  jpeg_par_decode_subseq(d, &v.f, tab, nat, a.entry[v.sub0 + s], sub_end(v.f, s),
                         CoefSink{&v.f, a.j.coef + a.j.plan[(int64_t)i * 3], a.gbase[v.sub0 + s], -2, nullptr}, &r);
}

__global__ __launch_bounds__(1024) void jpeg_par_dc_kernel(ParArgs a) {
  __shared__ uint32_t sum[1024];
  __shared__ uint8_t rst[1024];
  const int i = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  FileView v;
  if (!file_view(a, i, &v) || c >= v.f.ncomp) return;
  if (a.hdr[(int64_t)i * HDR_WORDS + HDR_ROUTE] != 1) return;
  int16_t* coef = a.j.coef + a.j.plan[(int64_t)i * 3];
  const int64_t nb = jpeg_par_comp_blocks(&v.f, c), chunk = (nb + 1023) / 1024;
  const int64_t j0 = t * chunk < nb ? t * chunk : nb, j1 = j0 + chunk < nb ? j0 + chunk : nb;
  bool reset;
  sum[t] = jpeg_par_dc_chunk(&v.f, coef, c, j0, j1, 0, false, &reset);
  rst[t] = reset;
  __syncthreads();
  if (t == 0) {                                                  // running sum entering every chunk
    uint32_t carry = 0;
    for (int k = 0; k < 1024; ++k) { const uint32_t sk = sum[k]; sum[k] = carry; carry = rst[k] ? sk : carry + sk; }
  }
  __syncthreads();
  jpeg_par_dc_chunk(&v.f, coef, c, j0, j1, sum[t], true, &reset);
}

struct Layout { int64_t hdr, mask, span_exit, entry, exit, nblocks, nrst, first_rst, reason, gbase, bytes; };
Layout layout(int64_t n, int64_t subs, int64_t spans) {
  Layout l;
  int64_t p = 0;
  auto take = [&p](int64_t bytes) { const int64_t at = p; p += (bytes + 255) / 256 * 256; return at; };
  l.hdr = take(n * HDR_WORDS * 4); l.mask = take(n * 4); l.span_exit = take(2 * spans * 8);
  l.entry = take(subs * 8); l.exit = take(subs * 8);
  l.nblocks = take(subs * 4); l.nrst = take(subs * 4); l.first_rst = take(subs * 4); l.reason = take(subs * 4); l.gbase = take(subs * 4);
  l.bytes = p;
  return l;
}

}  // namespace

extern "C" int drag_jpeg_par_geometry(int32_t* subseq_bytes, int32_t* subseqs_per_workgroup, int32_t* round_cap) {
  DRAG_CHECK(subseq_bytes && subseqs_per_workgroup && round_cap, "drag_jpeg_par_geometry: null pointer");
  *subseq_bytes = S; *subseqs_per_workgroup = SPAN; *round_cap = ROUND_CAP;
  return 0;
}

extern "C" int drag_jpeg_par_plan(const int64_t* scan_bytes, const int64_t* blocks, int32_t n, int64_t* par_plan, int64_t* totals,
                                  int64_t* workspace_bytes) {
  DRAG_CHECK(scan_bytes && blocks && par_plan && totals && workspace_bytes, "drag_jpeg_par_plan: null pointer");
  DRAG_CHECK(n > 0 && n <= 65535, "drag_jpeg_par_plan: n must be 1..65535");
  int64_t subs = 0, spans = 0, max_spans = 0;
  for (int i = 0; i < n; ++i) {
    DRAG_CHECK(scan_bytes[i] >= 0 && scan_bytes[i] < (1ll << 28) && blocks[i] >= 0, "drag_jpeg_par_plan: bad sizes");
    if (scan_bytes[i] == 0 || blocks[i] == 0) { par_plan[2 * i] = par_plan[2 * i + 1] = -1; continue; }
    const int64_t ns = (scan_bytes[i] + S - 1) / S, nw = (ns + SPAN - 1) / SPAN;
    par_plan[2 * i] = subs; par_plan[2 * i + 1] = spans;
    subs += ns; spans += nw;
    if (nw > max_spans) max_spans = nw;
  }
  totals[0] = subs; totals[1] = spans; totals[2] = max_spans;
  *workspace_bytes = layout(n, subs, spans).bytes;
  return 0;
}

extern "C" int drag_jpeg_decode_rgb_par(const void* data, const int64_t* offsets, const drag_jpeg_info* info, const int64_t* plan,
                                        int32_t n, int64_t max_blocks, int64_t max_pixels, void* coef_ws, int64_t coef_bytes,
                                        void* plane_ws, void* qtab_ws, void* out_rgb, int32_t* scan_status, const int64_t* par_plan,
                                        const int64_t* totals, void* workspace, int64_t workspace_bytes, int32_t* stats, void* stream) {
  DRAG_CHECK(data && offsets && info && plan && coef_ws && plane_ws && qtab_ws && out_rgb && scan_status && par_plan && totals &&
                 workspace && stats,
             "drag_jpeg_decode_rgb_par: null pointer");
  DRAG_CHECK(n > 0 && max_blocks > 0 && max_pixels > 0 && coef_bytes > 0, "drag_jpeg_decode_rgb_par: bad sizes");
  DRAG_CHECK(max_blocks < (1ll << 31) * 256 && max_pixels < (1ll << 31) * 256 && n <= 65535, "drag_jpeg_decode_rgb_par: batch too large");
  const int64_t subs = totals[0], spans = totals[1], max_spans = totals[2];
  DRAG_CHECK(subs >= 0 && spans >= 0 && max_spans >= 0 && max_spans <= spans && spans <= subs && subs < (1ll << 40),
             "drag_jpeg_decode_rgb_par: bad totals (drag_jpeg_par_plan writes them)");
  const Layout l = layout(n, subs, spans);
  DRAG_CHECK(workspace_bytes >= l.bytes, "drag_jpeg_decode_rgb_par: workspace too small (drag_jpeg_par_plan says how large)");
  DRAG_CHECK(((uintptr_t)workspace & 255) == 0, "drag_jpeg_decode_rgb_par: workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  ParArgs a;
  a.j.data = (const uint8_t*)data; a.j.off = offsets; a.j.info = (const JpegInfo*)info; a.j.plan = plan;
  a.j.coef = (int16_t*)coef_ws; a.j.planes = (uint8_t*)plane_ws; a.j.qtab = (uint16_t*)qtab_ws; a.j.out = (uint8_t*)out_rgb;
  a.j.scan_status = scan_status; a.j.n = n;
  a.par_plan = par_plan; a.tot_subs = subs; a.tot_spans = spans;
  a.hdr = (int32_t*)(ws + l.hdr); a.mask = (int32_t*)(ws + l.mask); a.span_exit = (JpegParState*)(ws + l.span_exit);
  a.entry = (JpegParState*)(ws + l.entry); a.exit = (JpegParState*)(ws + l.exit);
  a.nblocks = (int32_t*)(ws + l.nblocks); a.nrst = (int32_t*)(ws + l.nrst); a.first_rst = (int32_t*)(ws + l.first_rst);
  a.reason = (int32_t*)(ws + l.reason); a.gbase = (int32_t*)(ws + l.gbase);
  a.stats = stats;
  a.j.mask = a.mask;
  hipError_t e = hipMemsetAsync(coef_ws, 0, (size_t)coef_bytes, st);      // as drag_jpeg_decode_rgb: only non-zero coefficients are stored
  DRAG_CHECK(e == hipSuccess, "drag_jpeg_decode_rgb_par: memset failed");
  e = hipMemsetAsync(a.hdr, 0, (size_t)n * HDR_WORDS * 4, st);            // round flags
  DRAG_CHECK(e == hipSuccess, "drag_jpeg_decode_rgb_par: memset failed");
  if (max_spans > 0) {
    DRAG_CHECK(max_spans < (1ll << 31), "drag_jpeg_decode_rgb_par: batch too large");
    const dim3 grid((unsigned)max_spans, n);
    for (int round = 0; round <= ROUND_CAP; ++round) {
      hipLaunchKernelGGL(jpeg_par_round_kernel, grid, dim3(SPAN), 0, st, a, round);
      DRAG_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(jpeg_par_scan_kernel, dim3(n), dim3(256), 0, st, a);
  DRAG_LAUNCH_CHECK();
  if (max_spans > 0) {
    hipLaunchKernelGGL(jpeg_par_write_kernel, dim3((unsigned)max_spans, n), dim3(SPAN), 0, st, a);
    DRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_par_dc_kernel, dim3(3, n), dim3(1024), 0, st, a);
    DRAG_LAUNCH_CHECK();
  }
  return jpeg_lane_and_pixels(a.j, max_blocks, max_pixels, st);
}
