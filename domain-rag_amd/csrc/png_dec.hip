// png_dec.hip — PNG files in HBM -> uint8 pixels in HBM (gfx950): the functions of png_dec_core.h run in parallel.  The class of files
// is the one csrc/png.hip writes (8-bit grey / RGB, ONE final dynamic-Huffman block of literals); everything else gets a status and
// is left to the caller (png.py: Pillow).  A batch travels as one byte blob + offsets, like the JPEG decoder's; sizes differ per file.
//
//   1 pngd_parse_kernel     one workgroup per file: chunk walk by lane 0, the CRC-32 of every chunk by 256 lanes (pieces + GF(2)
//                           combine), IDAT payloads gathered into one contiguous zlib stream, zlib + block header (general RFC 1951
//                           form) and canonical codes by lane 0, the 2^15-entry direct table filled by all lanes
//   --- the caller reads the descriptors back (the one synchronisation) and plans workspace and output (drag_png_decode_plan) ---
//   2 pngd_round_kernel     x PNGD_ROUND_CAP: one lane per subsequence of PNGD_S bytes, PNGD_SPAN subsequences per workgroup, a file
//                           spans as many workgroups as it needs.  A workgroup settles its own span by Jacobi steps through LDS; the
//                           first lane of a span reads the exit the span before it had after the previous launch (two buffers).
//   3 pngd_verify_kernel    one workgroup per file: fixed-point check, first reason, end-of-block place, exclusive scan of the counts,
//                           the verdict of pngd_decide
//   4 pngd_write_kernel     as 2, from the settled entries, literals stored at the scanned offsets (filtered bytes, in the workspace)
//   5 pngd_adler_kernel     one lane per 64 filtered bytes: Adler-32 partial sums; the filter bytes are checked to be <= 4
//   6 pngd_unfilter_kernel  one wave per file: final status; un-filter by bands of PNGD_BAND rows, one row per lane, row y running one
//                           pixel behind row y - 1 (the anti-diagonal), b and c taken from the lane above with a lane shift
// All of it is stream-ordered.  Every loop's bound is geometry (bits of a subsequence, chunks that fit the file, rows and columns of
// the validated IHDR, the round cap), every read is checked against the file / stream length, every write against the planned
// region; nothing is written to the caller's output unless the file's status is 0.
#include "drag_common.h"
#include "png_dec_core.h"

namespace {

constexpr int ACHUNK = 64;         // filtered bytes per lane in the Adler kernel

struct PngdArgs {
  const uint8_t* data; const int64_t* offsets; int64_t total_bytes; int n;
  uint8_t* streams;                // file i's gathered zlib stream at streams + offsets[i] (capacity: the file's size)
  uint16_t* tables;                // [n, 2^15]
  int32_t* info;                   // [n, PNGD_INFO_WORDS]
  const int64_t* plan;             // [n, 4]: first subsequence slot, filtered-byte offset, output offset, output bytes
  int64_t total_subs, filt_total, out_total;
  int32_t *exit0, *exit1, *used, *count, *reason, *eob;      // [total_subs]
  int64_t* offs;                   // [total_subs]
  int32_t* res;                    // [n, 4]: verdict (fallback reason), rounds that decoded something, decided flag, last subsequence of the verdict
  unsigned long long* sums;        // [n, 4]: Adler A sum, B sum, bad-filter flag
  uint8_t* filt; uint8_t* out; int32_t* stats;
  int want_rgb, round;
};

__global__ __launch_bounds__(256) void pngd_parse_kernel(PngdArgs p) {
  __shared__ uint32_t tab[256], crc_s[256], len_s[256], next[16];
  __shared__ PngdWalk w;
  __shared__ int go_s, status_s;
  __shared__ uint8_t lens[320], work[160];
  __shared__ uint16_t rcode[260];
  const int i = blockIdx.x, t = threadIdx.x;
  tab[t] = png_crc_table_entry((uint32_t)t);
  const int64_t o0 = p.offsets[i], o1 = p.offsets[i + 1];
  const bool range_ok = o0 >= 0 && o1 >= o0 && o1 <= p.total_bytes;
  const int64_t size = range_ok ? o1 - o0 : 0;
  const uint8_t* f = p.data + (range_ok ? o0 : 0);
  uint8_t* stream = p.streams + (range_ok ? o0 : 0);
  if (t == 0) pngd_walk_init(&w, f, size);
  __syncthreads();
  const int64_t max_steps = size / 12 + 1;
  for (int64_t it = 0; it < max_steps; ++it) {
    if (t == 0) go_s = pngd_walk_next(&w, f, size);
    __syncthreads();
    if (!go_s) break;
    const int64_t pos = w.pos, base = w.idat_bytes;
    const uint32_t len = w.len;
    const bool gather = w.nchunks > 0 && w.type == PNGD_TYPE('I', 'D', 'A', 'T');
    const int64_t cn = (int64_t)len + 4;                        // the CRC's domain: type + data, inside the file (pngd_walk_next)
    const int64_t piece = max((int64_t)64, (cn + 255) / 256);
    const int64_t q0 = (int64_t)t * piece;
    const int64_t m = min(piece, max((int64_t)0, cn - q0));
    const uint8_t* cs = f + pos + 4;
    uint32_t crc = 0xffffffffu;
    for (int64_t k = 0; k < m; ++k) {
      const uint8_t b = cs[q0 + k];
      crc = tab[(crc ^ b) & 0xff] ^ (crc >> 8);
      const int64_t so = base + q0 + k - 4;
      if (gather && q0 + k >= 4 && so < size) stream[so] = b;
    }
    crc_s[t] = crc ^ 0xffffffffu; len_s[t] = (uint32_t)m;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      if ((t & (2 * s - 1)) == 0) {
        const uint32_t lb = len_s[t + s];
        if (lb) { crc_s[t] = len_s[t] ? png_crc_combine(crc_s[t], crc_s[t + s], lb) : crc_s[t + s]; len_s[t] += lb; }
      }
      __syncthreads();
    }
    if (t == 0) pngd_walk_commit(&w, f, crc_s[0] == pngd_be32(cs + 4 + len));
    __syncthreads();
  }
  __syncthreads();
  if (t == 0) {
    int st = w.status;
    if (st == 0 && !w.done) st = PNGD_TRUNCATED;
    if (!range_ok) st = PNGD_NOT_PNG;
    int32_t data_bit = 0, end_bit = 0;
    const int64_t zn = w.idat_bytes;
    if (st == 0) st = pngd_parse_stream_header(stream, zn, lens, work, &data_bit, &end_bit);
    if (st == 0) pngd_assign_codes(lens, rcode, next);
    int32_t* o = p.info + (int64_t)i * PNGD_INFO_WORDS;
    for (int k = 0; k < PNGD_INFO_WORDS; ++k) o[k] = 0;
    o[PNGD_I_STATUS] = st; o[PNGD_I_WIDTH] = w.width; o[PNGD_I_HEIGHT] = w.height; o[PNGD_I_CHANNELS] = w.channels;
    o[PNGD_I_IDAT_BYTES] = (int32_t)zn; o[PNGD_I_NIDAT] = w.nidat;
    if (st == 0) {
      o[PNGD_I_DATA_BIT] = data_bit; o[PNGD_I_END_BIT] = end_bit; o[PNGD_I_NSUB] = pngd_nsub(data_bit, end_bit, PNGD_S);
      o[PNGD_I_ADLER] = (int32_t)pngd_be32(stream + zn - 4);
    }
    status_s = st;
  }
  __syncthreads();
  if (status_s != 0) return;
  uint16_t* table = p.tables + (int64_t)i * PNGD_TABLE_SIZE;
  for (int s = 0; s < 257; ++s) pngd_fill_symbol(table, s, lens[s], rcode[s], (uint32_t)t, 256u);   // a complete code fills every entry
}

struct SubGeom { int32_t entry_guess, sub_end, data_bit, end_bit; int64_t g, zn; const uint8_t* z; const uint16_t* table; };

// the geometry of subsequence s of file i; false: nothing to do (declined file, s past the file's subsequences, a slot outside the plan)
__device__ __forceinline__ bool sub_geometry(const PngdArgs& p, int i, int64_t s, SubGeom& q) {
  const int32_t* info = p.info + (int64_t)i * PNGD_INFO_WORDS;
  if (info[PNGD_I_STATUS] != 0 || s >= info[PNGD_I_NSUB]) return false;
  q.g = p.plan[(int64_t)i * 4 + 0] + s;
  if (q.g < 0 || q.g >= p.total_subs) return false;
  q.data_bit = info[PNGD_I_DATA_BIT]; q.end_bit = info[PNGD_I_END_BIT]; q.zn = info[PNGD_I_IDAT_BYTES];
  const int64_t start = (int64_t)q.data_bit + 8ll * PNGD_S * s;
  if (start >= q.end_bit && s > 0) return false;
  q.entry_guess = (int32_t)start;
  q.sub_end = (int32_t)min(start + 8ll * PNGD_S, (int64_t)q.end_bit);
  q.z = p.streams + p.offsets[i];
  q.table = p.tables + (int64_t)i * PNGD_TABLE_SIZE;
  return true;
}

// One launch = one CROSS-SPAN round.  Inside it a workgroup iterates over its own span (Jacobi steps through LDS) until no entry of the
// span changes; PNGD_SPAN steps settle a span whatever the data, so the loop's bound is geometry.  Only the first lane of a span depends
// on another workgroup: it reads its predecessor's exit of the launch before (two buffers by the round's parity, so a launch does not
// depend on the order of its workgroups).
__global__ __launch_bounds__(PNGD_SPAN) void pngd_round_kernel(PngdArgs p) {
  __shared__ int32_t ex_s[PNGD_SPAN];
  const int i = blockIdx.y, t = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * PNGD_SPAN + t;
  if (p.info[(int64_t)i * PNGD_INFO_WORDS + PNGD_I_STATUS] != 0) return;          // the whole workgroup
  SubGeom q;
  const bool valid = sub_geometry(p, i, s, q);
  const int r = p.round;
  int32_t* ex_cur = (r & 1) ? p.exit1 : p.exit0;
  const int32_t* ex_prev = (r & 1) ? p.exit0 : p.exit1;
  PngdSub d = {PNGD_DEAD, 0, 0, -1};
  int32_t entry = PNGD_DEAD, used = PNGD_DEAD;
  bool have = false, decoded = false;
  if (valid) {
    entry = s == 0 ? q.data_bit : (r == 0 ? q.entry_guess : ex_prev[q.g - 1]);
    if (r > 0) {
      have = true; used = p.used[q.g]; d.exit = ex_prev[q.g]; d.count = p.count[q.g]; d.reason = p.reason[q.g]; d.eob_end = p.eob[q.g];
      if (pngd_terminal(entry)) entry = used;                       // terminal states do not travel (png_dec_core.h)
    }
  }
  for (int it = 0; it < PNGD_SPAN; ++it) {
    if (valid && (!have || entry != used)) {
      pngd_decode_subseq(q.z, q.zn, q.end_bit, q.table, entry, q.sub_end, PNGD_S, nullptr, 0, 0, &d);
      used = entry; have = true; decoded = true;
    }
    ex_s[t] = d.exit;
    __syncthreads();
    int changed = 0;
    if (valid && t > 0) {
      const int32_t e = ex_s[t - 1];
      if (!pngd_terminal(e)) entry = e;
      changed = entry != used;
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (!valid) return;
  ex_cur[q.g] = d.exit;
  if (decoded) {
    p.used[q.g] = used; p.count[q.g] = d.count; p.reason[q.g] = d.reason; p.eob[q.g] = d.eob_end;
    const unsigned long long act = __ballot(1);
    if (lane_id() == __ffsll((long long)act) - 1) atomicMax(&p.res[(int64_t)i * 4 + 1], r + 1);
  }
}

__global__ __launch_bounds__(1024) void pngd_verify_kernel(PngdArgs p) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t carry_s;
  __shared__ int conv_s;
  __shared__ unsigned int reason_key, eob_key, term_key;
  const int i = blockIdx.x, t = threadIdx.x;
  const int32_t* info = p.info + (int64_t)i * PNGD_INFO_WORDS;
  if (info[PNGD_I_STATUS] != 0) return;
  const int64_t nsub = info[PNGD_I_NSUB], g0 = p.plan[(int64_t)i * 4 + 0];
  if (g0 < 0 || g0 + nsub > p.total_subs) return;                // (res stays 0 only for planned files: the plan and the info agree)
  const int32_t* ex = ((PNGD_ROUND_CAP - 1) & 1) ? p.exit1 : p.exit0;
  if (t == 0) { carry_s = 0; conv_s = 1; reason_key = 0xffffffffu; eob_key = 0xffffffffu; term_key = (unsigned int)(nsub - 1); }
  __syncthreads();
  for (int64_t c = t; c < nsub; c += 1024)                         // f: the first subsequence whose exit is terminal; the verdict is over 0..f
    if (pngd_terminal(ex[g0 + c])) atomicMin(&term_key, (unsigned int)c);
  __syncthreads();
  const int64_t f = term_key;
  for (int64_t base = 0; base < nsub; base += 1024) {
    const int64_t c = base + t;
    int64_t v = 0;
    if (c <= f) {
      const int64_t g = g0 + c;
      v = p.count[g];
      if (c > 0 && p.used[g] != ex[g - 1]) conv_s = 0;
      const int rs = p.reason[g];
      if (rs) atomicMin(&reason_key, ((unsigned int)c << 3) | (unsigned int)rs);
      if (p.eob[g] >= 0) atomicMin(&eob_key, (unsigned int)c);
    }
    int64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t y = __shfl_up(x, d, 64);
      if (lane_id() >= d) x += y;
    }
    if (lane_id() == 63) wsum[wave_id()] = x;
    __syncthreads();
    int64_t off = carry_s;
    for (int k = 0; k < wave_id(); ++k) off += wsum[k];
    if (c < nsub) p.offs[g0 + c] = off + x - v;
    __syncthreads();
    if (t == 1023) carry_s = off + x;
    __syncthreads();
  }
  if (t == 0) {
    const int64_t nf = (int64_t)info[PNGD_I_HEIGHT] * (1 + (int64_t)info[PNGD_I_WIDTH] * info[PNGD_I_CHANNELS]);
    const int32_t eob_end = eob_key == 0xffffffffu ? -1 : p.eob[g0 + eob_key];
    const int first_reason = reason_key == 0xffffffffu ? 0 : (int)(reason_key & 7);
    int verdict = pngd_decide(conv_s, first_reason, eob_end, carry_s, nf, info[PNGD_I_END_BIT]);
    const int64_t fo = p.plan[(int64_t)i * 4 + 1];
    if (verdict == 0 && (fo < 0 || fo + nf > p.filt_total)) verdict = PNGD_FB_COUNT;     // cannot happen with drag_png_decode_plan's plan
    p.res[(int64_t)i * 4 + 0] = verdict;
    p.res[(int64_t)i * 4 + 2] = 1;                                // decided
    p.res[(int64_t)i * 4 + 3] = (int32_t)f;
  }
}

__device__ __forceinline__ bool file_settled(const PngdArgs& p, int i) {
  return p.info[(int64_t)i * PNGD_INFO_WORDS + PNGD_I_STATUS] == 0 && p.res[(int64_t)i * 4 + 2] == 1 && p.res[(int64_t)i * 4 + 0] == 0;
}

__global__ __launch_bounds__(PNGD_SPAN) void pngd_write_kernel(PngdArgs p) {
  const int i = blockIdx.y;
  const int64_t s = (int64_t)blockIdx.x * PNGD_SPAN + threadIdx.x;
  SubGeom q;
  if (!sub_geometry(p, i, s, q) || !file_settled(p, i) || s > p.res[(int64_t)i * 4 + 3]) return;
  const int32_t* info = p.info + (int64_t)i * PNGD_INFO_WORDS;
  const int64_t nf = (int64_t)info[PNGD_I_HEIGHT] * (1 + (int64_t)info[PNGD_I_WIDTH] * info[PNGD_I_CHANNELS]);
  PngdSub d;
  pngd_decode_subseq(q.z, q.zn, q.end_bit, q.table, p.used[q.g], q.sub_end, PNGD_S, p.filt + p.plan[(int64_t)i * 4 + 1], nf, p.offs[q.g], &d);
}

__global__ __launch_bounds__(256) void pngd_adler_kernel(PngdArgs p) {
  __shared__ unsigned long long red[4][2];
  const int i = blockIdx.y, t = threadIdx.x;
  if (!file_settled(p, i)) return;
  const int32_t* info = p.info + (int64_t)i * PNGD_INFO_WORDS;
  const int64_t H = info[PNGD_I_HEIGHT], rb = (int64_t)info[PNGD_I_WIDTH] * info[PNGD_I_CHANNELS], nf = H * (1 + rb);
  const uint8_t* filt = p.filt + p.plan[(int64_t)i * 4 + 1];
  const int64_t c = (int64_t)blockIdx.x * 256 + t;
  const int64_t j0 = c * ACHUNK;
  uint64_t sa = 0, sb = 0;
  if (j0 < nf) pngd_adler_chunk(filt + j0, (int)min((int64_t)ACHUNK, nf - j0), j0, nf, &sa, &sb);
  bool bad = false;
  for (int64_t r = c; r < H; r += (int64_t)gridDim.x * 256) bad = bad || filt[r * (1 + rb)] > 4;
  unsigned long long a = sa, b = sb;
#pragma unroll
  for (int m2 = 32; m2 >= 1; m2 >>= 1) { a += __shfl_xor(a, m2, 64); b += __shfl_xor(b, m2, 64); }
  if (lane_id() == 0) { red[wave_id()][0] = a; red[wave_id()][1] = b; }
  if (bad) atomicOr(&p.sums[(int64_t)i * 4 + 2], 1ull);
  __syncthreads();
  if (t == 0) {
    atomicAdd(&p.sums[(int64_t)i * 4 + 0], red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    atomicAdd(&p.sums[(int64_t)i * 4 + 1], red[0][1] + red[1][1] + red[2][1] + red[3][1]);
  }
}

// One wave per file.  Lane l of a band holds row band + l and at step t reconstructs pixel x = t - l: the lane above reconstructed the
// same x one step earlier (that is b) and x - 1 two steps earlier (c = the b of this lane's previous step); a is the lane's own previous
// result.  Lane 0 reads b from the output row above, which the previous band wrote (fence + barrier between bands).  Eight steps'
// loads are issued together so that their latency is paid once per eight steps.
__global__ __launch_bounds__(64) void pngd_unfilter_kernel(PngdArgs p) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int32_t* info = p.info + (int64_t)i * PNGD_INFO_WORDS;
  int st = info[PNGD_I_STATUS], reason = 0;
  const int H = info[PNGD_I_HEIGHT], W = info[PNGD_I_WIDTH], C = info[PNGD_I_CHANNELS];
  const int64_t rb = (int64_t)W * C, nf = (int64_t)H * (1 + rb);
  const int Co = (C == 1 && p.want_rgb) ? 3 : C;
  const int64_t out_off = p.plan[(int64_t)i * 4 + 2], out_bytes = p.plan[(int64_t)i * 4 + 3];
  if (st == 0) {
    if (p.res[(int64_t)i * 4 + 2] != 1) { st = PNGD_FALLBACK; reason = PNGD_FB_COUNT; }       // not planned: never with drag_png_decode_plan's plan
    else if ((reason = p.res[(int64_t)i * 4 + 0]) != 0) st = PNGD_FALLBACK;
    else if (pngd_adler_finish(p.sums[(int64_t)i * 4 + 0], p.sums[(int64_t)i * 4 + 1], nf) != (uint32_t)info[PNGD_I_ADLER]) st = PNGD_ADLER;
    else if (p.sums[(int64_t)i * 4 + 2] != 0) st = PNGD_FILTER;
    else if (out_off < 0 || out_bytes != (int64_t)H * W * Co || out_off + out_bytes > p.out_total) { st = PNGD_FALLBACK; reason = PNGD_FB_COUNT; }
  }
  if (lane == 0) {
    int32_t* o = p.stats + (int64_t)i * 4;
    o[0] = st; o[1] = reason; o[2] = info[PNGD_I_STATUS] == 0 ? p.res[(int64_t)i * 4 + 1] : 0; o[3] = info[PNGD_I_STATUS] == 0 ? info[PNGD_I_NSUB] : 0;
  }
  if (st != 0) return;
  const uint8_t* filt = p.filt + p.plan[(int64_t)i * 4 + 1];
  uint8_t* out = p.out + out_off;
  const int nsteps = W + PNGD_BAND - 1;
  for (int band = 0; band < H; band += PNGD_BAND) {
    const int y = band + lane;
    const bool active = y < H;
    const uint8_t* row = filt + (int64_t)(active ? y : 0) * (1 + rb);
    const int f = active ? row[0] : 0;
    const uint8_t* up_row = out + (int64_t)(y > 0 ? y - 1 : 0) * W * Co;
    const bool take_up = lane == 0 && y > 0;
    uint32_t last = 0, cprev = 0;
    for (int t0 = 0; t0 < nsteps; t0 += 8) {
      uint32_t raw[8], up[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int x = t0 + k - lane;
        raw[k] = 0; up[k] = 0;
        if (active && x >= 0 && x < W) {
          const uint8_t* px = row + 1 + (int64_t)x * C;
          raw[k] = px[0];
          if (C == 3) raw[k] |= ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
          if (take_up) {
            const uint8_t* ux = up_row + (int64_t)x * Co;
            up[k] = ux[0];
            if (C == 3) up[k] |= ((uint32_t)ux[1] << 8) | ((uint32_t)ux[2] << 16);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int x = t0 + k - lane;
        uint32_t bpk = __shfl_up(last, 1, 64);
        if (lane == 0) bpk = up[k];
        if (active && x >= 0 && x < W) {
          uint32_t v = 0;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch)
            if (ch < C)
              v |= (uint32_t)pngd_unfilter_byte(f, (raw[k] >> (8 * ch)) & 255, (last >> (8 * ch)) & 255, (bpk >> (8 * ch)) & 255,
                                                (cprev >> (8 * ch)) & 255) << (8 * ch);
          const int64_t idx = ((int64_t)y * W + x) * Co;
          if (idx + Co <= out_bytes) {
            if (C == 3) { out[idx] = (uint8_t)v; out[idx + 1] = (uint8_t)(v >> 8); out[idx + 2] = (uint8_t)(v >> 16); }
            else { for (int k2 = 0; k2 < Co; ++k2) out[idx + k2] = (uint8_t)v; }
          }
          last = v; cprev = bpk;
        }
      }
    }
    __threadfence();
    __syncthreads();
  }
}

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct ParseLayout { int64_t off_tables, total; };
bool parse_layout(int n, int64_t total_bytes, ParseLayout& q) {
  if (n <= 0 || n > 65535 || total_bytes < 0 || total_bytes >= ((int64_t)1 << 40)) return false;
  q.off_tables = align_up(total_bytes + 64, 256);
  q.total = q.off_tables + (int64_t)n * PNGD_TABLE_SIZE * 2;
  return true;
}

struct DecLayout { int64_t off_exit0, off_exit1, off_used, off_count, off_reason, off_eob, off_offs, off_res, off_sums, off_filt, total; };
bool dec_layout(int n, int64_t total_subs, int64_t filt_total, DecLayout& q) {
  if (n <= 0 || n > 65535 || total_subs < 0 || filt_total < 0 || total_subs >= ((int64_t)1 << 40) || filt_total >= ((int64_t)1 << 44)) return false;
  int64_t o = 0;
  const int64_t sub4 = align_up(total_subs * 4 + 4, 256);
  q.off_exit0 = o; o += sub4;
  q.off_exit1 = o; o += sub4;
  q.off_used = o; o += sub4;
  q.off_count = o; o += sub4;
  q.off_reason = o; o += sub4;
  q.off_eob = o; o += sub4;
  q.off_offs = o; o += align_up(total_subs * 8 + 8, 256);
  q.off_res = o; o += align_up((int64_t)n * 16, 256);
  q.off_sums = o; o += align_up((int64_t)n * 32, 256);
  q.off_filt = o; o += align_up(filt_total + 64, 256);
  q.total = o;
  return true;
}

}  // namespace

extern "C" int drag_png_decode_geometry(int32_t* subsequence_bytes, int32_t* span, int32_t* round_cap, int32_t* band_rows) {
  if (subsequence_bytes) *subsequence_bytes = PNGD_S;
  if (span) *span = PNGD_SPAN;
  if (round_cap) *round_cap = PNGD_ROUND_CAP;
  if (band_rows) *band_rows = PNGD_BAND;
  return 0;
}

extern "C" int drag_png_parse_workspace(int32_t n, int64_t total_bytes, int64_t* workspace_bytes) {
  ParseLayout q;
  DRAG_CHECK(workspace_bytes, "drag_png_parse_workspace: null pointer");
  DRAG_CHECK(parse_layout(n, total_bytes, q), "drag_png_parse_workspace: 1 <= n <= 65535 files and 0 <= total_bytes < 2^40 expected");
  *workspace_bytes = q.total;
  return 0;
}

extern "C" int drag_png_parse(const void* data, const int64_t* offsets, int32_t n, int64_t total_bytes, void* parse_ws, int64_t parse_ws_bytes,
                              int32_t* info, void* stream) {
  DRAG_CHECK(data && offsets && parse_ws && info, "drag_png_parse: null pointer");
  ParseLayout q;
  DRAG_CHECK(parse_layout(n, total_bytes, q), "drag_png_parse: 1 <= n <= 65535 files and 0 <= total_bytes < 2^40 expected");
  DRAG_CHECK(parse_ws_bytes >= q.total, "drag_png_parse: workspace smaller than drag_png_parse_workspace's");
  DRAG_CHECK(((uintptr_t)parse_ws & 255) == 0, "drag_png_parse: workspace must be 256-byte aligned");
  PngdArgs p = {};
  p.data = (const uint8_t*)data; p.offsets = offsets; p.total_bytes = total_bytes; p.n = n;
  p.streams = (uint8_t*)parse_ws; p.tables = (uint16_t*)((char*)parse_ws + q.off_tables); p.info = info;
  hipLaunchKernelGGL(pngd_parse_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}

// host only: info = the descriptors read back from drag_png_parse.  plan[i] = {first subsequence slot, filtered-byte offset, output offset,
// output bytes} (zeros for a declined file), totals = {subsequences, filtered bytes, output bytes, most subsequences in a file, most
// filtered bytes in a file}
extern "C" int drag_png_decode_plan(const int32_t* info, int32_t n, int32_t want_rgb, int64_t* plan, int64_t* totals, int64_t* workspace_bytes) {
  DRAG_CHECK(info && plan && totals && workspace_bytes, "drag_png_decode_plan: null pointer");
  DRAG_CHECK(n > 0 && n <= 65535, "drag_png_decode_plan: 1 <= n <= 65535 files expected");
  int64_t subs = 0, filt = 0, outb = 0, max_sub = 0, max_nf = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t* o = info + (int64_t)i * PNGD_INFO_WORDS;
    int64_t* q = plan + (int64_t)i * 4;
    q[0] = q[1] = q[2] = q[3] = 0;
    if (o[PNGD_I_STATUS] != 0) continue;
    const int64_t H = o[PNGD_I_HEIGHT], W = o[PNGD_I_WIDTH], C = o[PNGD_I_CHANNELS], nsub = o[PNGD_I_NSUB];
    const int64_t nf = H * (1 + W * C);
    DRAG_CHECK(H > 0 && W > 0 && (C == 1 || C == 3) && nf < ((int64_t)1 << 26) && nsub > 0 && nsub <= ((int64_t)1 << 28) / PNGD_S + 1,
               "drag_png_decode_plan: a descriptor with status 0 that drag_png_parse cannot have written");
    const int64_t ob = H * W * ((C == 1 && want_rgb) ? 3 : C);
    q[0] = subs; q[1] = filt; q[2] = outb; q[3] = ob;
    subs += nsub; filt += align_up(nf, 64); outb += align_up(ob, 64);
    max_sub = nsub > max_sub ? nsub : max_sub; max_nf = nf > max_nf ? nf : max_nf;
  }
  DecLayout L;
  DRAG_CHECK(dec_layout(n, subs, filt, L), "drag_png_decode_plan: batch too large");
  totals[0] = subs; totals[1] = filt; totals[2] = outb; totals[3] = max_sub; totals[4] = max_nf;
  *workspace_bytes = L.total;
  return 0;
}

extern "C" int drag_png_decode(const void* parse_ws, const int64_t* offsets, int32_t n, int64_t total_bytes, const int32_t* info, const int64_t* plan,
                               const int64_t* totals, int32_t want_rgb, void* workspace, int64_t workspace_bytes, void* out, int64_t out_bytes,
                               int32_t* stats, void* stream) {
  DRAG_CHECK(parse_ws && offsets && info && plan && totals && workspace && out && stats, "drag_png_decode: null pointer");
  ParseLayout q;
  DRAG_CHECK(parse_layout(n, total_bytes, q), "drag_png_decode: 1 <= n <= 65535 files and 0 <= total_bytes < 2^40 expected");
  DecLayout L;
  DRAG_CHECK(totals[3] >= 0 && totals[3] <= totals[0] && totals[4] >= 0 && totals[4] <= totals[1] && totals[2] >= 0 && dec_layout(n, totals[0], totals[1], L),
             "drag_png_decode: totals are not drag_png_decode_plan's");
  DRAG_CHECK(workspace_bytes >= L.total, "drag_png_decode: workspace smaller than drag_png_decode_plan's");
  DRAG_CHECK(out_bytes >= totals[2], "drag_png_decode: output buffer smaller than drag_png_decode_plan's");
  DRAG_CHECK(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)parse_ws & 255) == 0, "drag_png_decode: workspaces must be 256-byte aligned");
  char* ws = (char*)workspace;
  PngdArgs p = {};
  p.offsets = offsets; p.total_bytes = total_bytes; p.n = n;
  p.streams = (uint8_t*)parse_ws; p.tables = (uint16_t*)((char*)parse_ws + q.off_tables); p.info = (int32_t*)info;
  p.plan = plan; p.total_subs = totals[0]; p.filt_total = totals[1]; p.out_total = totals[2];
  p.exit0 = (int32_t*)(ws + L.off_exit0); p.exit1 = (int32_t*)(ws + L.off_exit1); p.used = (int32_t*)(ws + L.off_used);
  p.count = (int32_t*)(ws + L.off_count); p.reason = (int32_t*)(ws + L.off_reason); p.eob = (int32_t*)(ws + L.off_eob);
  p.offs = (int64_t*)(ws + L.off_offs); p.res = (int32_t*)(ws + L.off_res); p.sums = (unsigned long long*)(ws + L.off_sums);
  p.filt = (uint8_t*)(ws + L.off_filt); p.out = (uint8_t*)out; p.stats = stats; p.want_rgb = want_rgb ? 1 : 0;
  const hipStream_t st = (hipStream_t)stream;
  DRAG_CHECK(hipMemsetAsync(ws + L.off_res, 0, (size_t)(L.off_filt - L.off_res), st) == hipSuccess, "drag_png_decode: memset failed");
  if (totals[0] > 0) {
    const dim3 gsub((unsigned)((totals[3] + PNGD_SPAN - 1) / PNGD_SPAN), (unsigned)n);
    for (int r = 0; r < PNGD_ROUND_CAP; ++r) {
      p.round = r;
      hipLaunchKernelGGL(pngd_round_kernel, gsub, dim3(PNGD_SPAN), 0, st, p);
    }
    hipLaunchKernelGGL(pngd_verify_kernel, dim3((unsigned)n), dim3(1024), 0, st, p);
    hipLaunchKernelGGL(pngd_write_kernel, gsub, dim3(PNGD_SPAN), 0, st, p);
    const int64_t nchunks = (totals[4] + ACHUNK - 1) / ACHUNK;
    hipLaunchKernelGGL(pngd_adler_kernel, dim3((unsigned)((nchunks + 255) / 256), (unsigned)n), dim3(256), 0, st, p);
  }
  hipLaunchKernelGGL(pngd_unfilter_kernel, dim3((unsigned)n), dim3(64), 0, st, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}
