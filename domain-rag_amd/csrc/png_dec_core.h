// png_dec_core.h — the arithmetic of a PNG reader for the files csrc/png.hip writes (and any other file of the same class): container
// walk with CRC-32, zlib / DEFLATE dynamic block header in the general RFC 1951 form, canonical code and direct lookup table, Huffman
// decoding of ONE literal-only block from many starting points at once, Adler-32 from partial sums, the five PNG un-filters.
// Host/device neutral (PHD convention of png_core.h): csrc/png_dec.hip runs these functions in gfx950 kernels, tests/helpers/
// png_dec_host.cpp compiles the same header with g++ and runs the rounds serially.  The yardstick is Pillow: a file the device route
// accepts decodes to exactly Image.open(f).convert(mode); everything else is DECLINED with a number and decoded by Pillow itself.
//
// STATUS (why a file is not decoded on the device; 0 = it was)
//    1 PNGD_NOT_PNG      signature / first chunk is not a 13-byte IHDR / zero size / compression or filter method not 0
//    2 PNGD_TRUNCATED    a chunk does not fit the file, no IEND, no IDAT, or a zlib stream shorter than its header + Adler-32
//    3 PNGD_CRC          the CRC-32 of a chunk (IHDR, every IDAT, and every other chunk walked over) does not match
//    4 PNGD_BIT_DEPTH    bit depth other than 8
//    5 PNGD_COLOUR       colour type other than 0 / 2 (palette, alpha), or a PLTE / tRNS chunk
//    6 PNGD_INTERLACED   Adam7
//    7 PNGD_BLOCK_KIND   the first DEFLATE block is stored, fixed, reserved, or not the final one (multi-block)
//    8 PNGD_HLIT         HLIT > 257: length symbols (LZ77 matches) are possible
//    9 PNGD_BAD_TABLE    code-length code or literal code incomplete / over-subscribed, a repeat without a predecessor or past the
//                        end, no end-of-block code, a distance code zlib refuses
//   10 PNGD_EXIF         an eXIf chunk, a text chunk "Raw profile type exif" or an XMP packet ("XML:com.adobe.xmp"): everything Pillow's
//                        getexif() takes an orientation from; the caller applies it
//   11 PNGD_TOO_LARGE    2^26 or more filtered bytes (the encoder's limit), or 2^28 or more IDAT bytes
//   12 PNGD_OTHER        bad CMF/FLG, preset dictionary, unknown critical chunk, APNG chunks, IDAT chunks that are not consecutive,
//                        more than PNGD_MAX_CHUNKS chunks
//   13 PNGD_ADLER        the Adler-32 of the decoded bytes is not the stream's
//   14 PNGD_FILTER       a filter byte > 4
//   15 PNGD_FALLBACK     the parallel Huffman decode declined; the FALLBACK REASON says why:
//    1 PNGD_FB_NO_CODE   a 15-bit window is no code of the table
//    2 PNGD_FB_PAST_END  a symbol needs bits past the stream (this is also how a missing end-of-block symbol shows)
//    3 PNGD_FB_EARLY_EOB end-of-block after fewer than H * (1 + W * C) literals
//    4 PNGD_FB_TRAILING  bytes between the end-of-block's byte boundary and the Adler-32
//    5 PNGD_FB_COUNT     end-of-block after more than H * (1 + W * C) literals
//    6 PNGD_FB_ROUND_CAP the rounds did not reach the fixed point within PNGD_ROUND_CAP
//   16 (never written by this code or the kernels) png.py's decode_files sets it in its copy of the descriptors when mode "L" is
//                        asked of an RGB file: Pillow's luma transform is not a device path
// Every one of these is known BEFORE a pixel is written: the filtered bytes go to a workspace, the caller's output only sees the
// un-filter, which runs when the status is 0.
//
// PARALLEL HUFFMAN DECODE.  The DEFLATE data [data_bit, end_bit) (bit positions LSB-first inside the zlib stream; end_bit is where
// the Adler-32 starts) is cut into SUBSEQUENCES of S bytes counted from data_bit.  The decoder state at a symbol boundary is the bit
// position alone (no byte stuffing, no block index), plus two terminal states: PNGD_END (the end-of-block symbol has been decoded)
// and PNGD_DEAD (the decode ran into reason 1 or 2).  Subsequence 0 enters at data_bit, every other one at its own first bit as a
// guess; a subsequence decodes every symbol that STARTS before its end and hands its exit state on.  Jacobi rounds: in round r a
// subsequence whose predecessor's exit of round r - 1 differs from the entry it last decoded from decodes again from that exit.
//   Induction (that of jpeg_par_core.h): the result of a subsequence is a function of its entry alone.  Subsequence 0's entry is the
//   true one in every round.  If after a round every entry used by s >= 1 equals the exit of s - 1 (the check pngd_decide gets as
//   `converged`), then s = 1 decoded from the true exit of 0, hence has the sequential decoder's exit, hence s = 2 ..., so all counts,
//   exits and reasons are the sequential decoder's.  After round r subsequences 0..r are right whatever the data, so nsub rounds always
//   suffice; self-synchronisation of Huffman codes only makes the rounds few.  Correctness never rests on it having happened: a file
//   whose rounds exceed the cap falls back (reason 6).
// The rounds are run in two levels, as the JPEG route's: a SPAN of PNGD_SPAN consecutive subsequences belongs to one workgroup, which
// repeats Jacobi steps over its span until none of its entries changes (at most PNGD_SPAN steps: step k settles the span's k-th
// subsequence, given the span's first entry).  One launch does that for every span at once; the first subsequence of a span enters
// at the exit its predecessor had at the end of the launch before.  PNGD_ROUND_CAP counts these launches.  The fixed-point check is
// the same one over ALL subsequences, so the argument above is untouched by how the steps were scheduled; a file whose code does
// not self-synchronise settles one span per launch and needs as many launches as it has spans.
// TERMINAL STATES DO NOT TRAVEL.  A decode from a wrong guess can meet the end-of-block code anywhere (or die near the end of the
// stream).  If its successors took PNGD_END / PNGD_DEAD as their entry they would drop the (usually already right) state they reached from
// their own guess, and the loss would run ahead of the repair, one span per launch.  So a subsequence IGNORES a terminal exit of its
// predecessor and keeps what it has, and the verdict is taken over the prefix 0..f, f = the first subsequence whose exit is terminal
// (or the last one): the fixed-point check, the reasons, the end-of-block place and the counts of 0..f only.  That is sound: the
// induction above covers 0..f, and the sequential decoder stops in f — behind it there is nothing to decode, which pngd_decide checks
// (the end-of-block must end in the last byte before the Adler-32, with exactly H * (1 + W * C) literals before it).
// An exclusive scan of the per-subsequence literal counts gives each subsequence its output offset; the writing pass decodes once
// more from the settled entries (subsequences 0..f).
#pragma once
#include "png_core.h"

// product geometry (reasons: DESIGN.md (f)); the host helper takes S and the cap at run time
#define PNGD_S 128             // compressed bytes per subsequence
#define PNGD_SPAN 256          // subsequences per workgroup
#define PNGD_ROUND_CAP 8       // cross-span rounds (launches); inside a launch a workgroup iterates over its own span until it is settled
#define PNGD_BAND 64           // rows per un-filter band: one row per lane of a wave
#define PNGD_MAX_CHUNKS 8192   // chunks walked per file (a walk step costs a workgroup a few barriers: a hostile file of empty chunks stays short)
#define PNGD_TABLE_BITS 15
#define PNGD_TABLE_SIZE (1 << PNGD_TABLE_BITS)
#define PNGD_INFO_WORDS 16

enum {
  PNGD_OK = 0, PNGD_NOT_PNG = 1, PNGD_TRUNCATED = 2, PNGD_CRC = 3, PNGD_BIT_DEPTH = 4, PNGD_COLOUR = 5, PNGD_INTERLACED = 6,
  PNGD_BLOCK_KIND = 7, PNGD_HLIT = 8, PNGD_BAD_TABLE = 9, PNGD_EXIF = 10, PNGD_TOO_LARGE = 11, PNGD_OTHER = 12, PNGD_ADLER = 13,
  PNGD_FILTER = 14, PNGD_FALLBACK = 15,
};
enum {
  PNGD_FB_NONE = 0, PNGD_FB_NO_CODE = 1, PNGD_FB_PAST_END = 2, PNGD_FB_EARLY_EOB = 3, PNGD_FB_TRAILING = 4, PNGD_FB_COUNT = 5,
  PNGD_FB_ROUND_CAP = 6,
};
enum { PNGD_END = 0x7fffffff, PNGD_DEAD = 0x7ffffffe };

// info words (int32) per file
enum { PNGD_I_STATUS = 0, PNGD_I_WIDTH, PNGD_I_HEIGHT, PNGD_I_CHANNELS, PNGD_I_IDAT_BYTES, PNGD_I_DATA_BIT, PNGD_I_END_BIT, PNGD_I_NSUB,
       PNGD_I_ADLER, PNGD_I_NIDAT };

PHD uint32_t pngd_be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
#define PNGD_TYPE(a, b, c, d) (((uint32_t)(a) << 24) | ((uint32_t)(b) << 16) | ((uint32_t)(c) << 8) | (uint32_t)(d))

// ---- container ------------------------------------------------------------------------------------------------------
// The walk is cut into steps so that the caller can checksum (and gather) a chunk between them with as many lanes as it has:
//   pngd_walk_init; while (pngd_walk_next) { crc over f[pos + 4, pos + 8 + len) ; if IDAT: copy f[pos + 8, +len) to stream + idat_bytes ;
//   pngd_walk_commit(crc_ok) }.  Every step moves pos by at least 12 bytes: at most size / 12 steps.
struct PngdWalk {
  int64_t pos, idat_bytes;
  uint32_t len, type;
  int32_t status, done, nchunks, idat_state /* 0 none yet, 1 inside the run of IDATs, 2 behind it */, nidat;
  int32_t width, height, channels;
};
PHD void pngd_walk_init(PngdWalk* w, const uint8_t* f, int64_t size) {
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  w->pos = 8; w->idat_bytes = 0; w->len = 0; w->type = 0; w->status = 0; w->done = 0; w->nchunks = 0; w->idat_state = 0; w->nidat = 0;
  w->width = w->height = w->channels = 0;
  bool prefix = true;
  for (int k = 0; k < 8; ++k)
    if (k < size && f[k] != sig[k]) prefix = false;
  if (!prefix || size == 0) w->status = PNGD_NOT_PNG;
  else if (size < 8) w->status = PNGD_TRUNCATED;
}
// 1: there is a chunk (w->len, w->type) at w->pos that fits the file; 0: the walk is over (w->status says how)
PHD int pngd_walk_next(PngdWalk* w, const uint8_t* f, int64_t size) {
  if (w->status != 0 || w->done) return 0;
  if (w->pos + 12 > size) { w->status = PNGD_TRUNCATED; return 0; }
  if (w->nchunks >= PNGD_MAX_CHUNKS) { w->status = PNGD_OTHER; return 0; }
  const uint32_t len = pngd_be32(f + w->pos);
  if (len > 0x7fffffffu || (int64_t)len > size - w->pos - 12) { w->status = PNGD_TRUNCATED; return 0; }
  w->len = len; w->type = pngd_be32(f + w->pos + 4);
  return 1;
}
// a text chunk Pillow's getexif() reads an orientation from: keyword "Raw profile type exif", or (iTXt) the XMP packet "XML:com.adobe.xmp"
PHD bool pngd_is_exif_text(const uint8_t* d, uint32_t len) {
  const char key[] = "Raw profile type exif";
  const char xmp[] = "XML:com.adobe.xmp";
  bool is_key = len >= sizeof(key) - 1, is_xmp = len >= sizeof(xmp) - 1;
  for (uint32_t k = 0; k < sizeof(key) - 1 && is_key; ++k)
    if (d[k] != (uint8_t)key[k]) is_key = false;
  for (uint32_t k = 0; k < sizeof(xmp) - 1 && is_xmp; ++k)
    if (d[k] != (uint8_t)xmp[k]) is_xmp = false;
  return is_key || is_xmp;
}
PHD void pngd_walk_commit(PngdWalk* w, const uint8_t* f, int crc_ok) {
  const uint8_t* d = f + w->pos + 8;
  const uint32_t t = w->type, len = w->len;
  if (!crc_ok) { w->status = w->nchunks == 0 && (t != PNGD_TYPE('I', 'H', 'D', 'R') || len != 13) ? PNGD_NOT_PNG : PNGD_CRC; return; }
  if (w->nchunks == 0) {
    if (t != PNGD_TYPE('I', 'H', 'D', 'R') || len != 13) { w->status = PNGD_NOT_PNG; return; }
    const uint32_t W = pngd_be32(d), H = pngd_be32(d + 4);
    const int depth = d[8], ctype = d[9];
    if (W == 0 || H == 0 || W > 0x7fffffffu || H > 0x7fffffffu || d[10] != 0 || d[11] != 0 || d[12] > 1) { w->status = PNGD_NOT_PNG; return; }
    if (depth != 8) { w->status = PNGD_BIT_DEPTH; return; }
    if (ctype != 0 && ctype != 2) { w->status = PNGD_COLOUR; return; }
    if (d[12] != 0) { w->status = PNGD_INTERLACED; return; }
    const int C = ctype == 0 ? 1 : 3;
    const int64_t rb = (int64_t)W * C;
    if (rb >= ((int64_t)1 << 26) || (int64_t)H * (1 + rb) >= ((int64_t)1 << 26)) { w->status = PNGD_TOO_LARGE; return; }
    w->width = (int32_t)W; w->height = (int32_t)H; w->channels = C;
  } else if (t == PNGD_TYPE('I', 'D', 'A', 'T')) {
    if (w->idat_state == 2) { w->status = PNGD_OTHER; return; }
    w->idat_state = 1; w->nidat++;
    w->idat_bytes += len;
    if (w->idat_bytes >= ((int64_t)1 << 28)) { w->status = PNGD_TOO_LARGE; return; }
  } else {
    if (w->idat_state == 1) w->idat_state = 2;
    if (t == PNGD_TYPE('I', 'E', 'N', 'D')) {
      w->done = 1;
      if (w->idat_state == 0) w->status = PNGD_TRUNCATED;
      return;
    }
    if (t == PNGD_TYPE('P', 'L', 'T', 'E') || t == PNGD_TYPE('t', 'R', 'N', 'S')) { w->status = PNGD_COLOUR; return; }
    if (t == PNGD_TYPE('e', 'X', 'I', 'f')) { w->status = PNGD_EXIF; return; }
    if ((t == PNGD_TYPE('t', 'E', 'X', 't') || t == PNGD_TYPE('z', 'T', 'X', 't') || t == PNGD_TYPE('i', 'T', 'X', 't')) && pngd_is_exif_text(d, len)) {
      w->status = PNGD_EXIF; return;
    }
    if (t == PNGD_TYPE('a', 'c', 'T', 'L') || t == PNGD_TYPE('f', 'c', 'T', 'L') || t == PNGD_TYPE('f', 'd', 'A', 'T') || !((t >> 24) & 0x20)) {
      w->status = PNGD_OTHER; return;               // APNG, or a critical chunk this reader does not know
    }
  }
  w->pos += 12 + (int64_t)len;
  w->nchunks++;
}

// ---- bits of the zlib stream (LSB first) ------------------------------------------------------------------------------
// 24 bits starting at bit position pos; bytes at or behind nbytes read as zero (the caller compares positions with end_bit)
PHD uint32_t pngd_window(const uint8_t* z, int64_t nbytes, int64_t pos) {
  const int64_t i = pos >> 3;
  uint32_t w;
  if (i + 4 <= nbytes) {
    __builtin_memcpy(&w, z + i, 4);                  // little-endian on both builds
  } else {
    w = 0;
    for (int k = 0; k < 4; ++k)
      if (i + k < nbytes && i + k >= 0) w |= (uint32_t)z[i + k] << (8 * k);
  }
  return w >> (pos & 7);
}
// n <= 16 header bits; *bad is set when they reach past limit_bit
PHD uint32_t pngd_take(const uint8_t* z, int64_t nbytes, int64_t limit_bit, int64_t* pos, int n, int* bad) {
  if (*pos + n > limit_bit) { *bad = 1; return 0; }
  const uint32_t v = pngd_window(z, nbytes, *pos) & ((1u << n) - 1);
  *pos += n;
  return v;
}

// Kraft sum of n code lengths in units of 2^-15 (complete: exactly 1 << 15)
PHD uint32_t pngd_kraft(const uint8_t* len, int n) {
  uint32_t k = 0;
  for (int s = 0; s < n; ++s)
    if (len[s]) k += 1u << (15 - len[s]);
  return k;
}

// zlib header + the dynamic block's header.  lens: >= 320 bytes, receives the 257 literal lengths (then the distance lengths);
// work: >= 160 bytes (the code-length code's 19 lengths and its 7-bit lookup table: no dynamically indexed local arrays, so a kernel
// keeps them in LDS).  Returns the status; on 0 *data_bit is the first bit of the data and *end_bit where the Adler-32 starts.
PHD int pngd_parse_stream_header(const uint8_t* z, int64_t zn, uint8_t* lens, uint8_t* work, int32_t* data_bit, int32_t* end_bit) {
  if (zn < 2 + 4) return PNGD_TRUNCATED;
  const int cmf = z[0], flg = z[1];
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return PNGD_OTHER;
  const int64_t limit = 8 * (zn - 4);
  int64_t pos = 16;
  int bad = 0;
  const uint32_t bfinal = pngd_take(z, zn, limit, &pos, 1, &bad), btype = pngd_take(z, zn, limit, &pos, 2, &bad);
  if (bad) return PNGD_TRUNCATED;
  if (btype != 2 || bfinal != 1) return PNGD_BLOCK_KIND;
  const int hlit = 257 + (int)pngd_take(z, zn, limit, &pos, 5, &bad), hdist = 1 + (int)pngd_take(z, zn, limit, &pos, 5, &bad);
  const int hclen = 4 + (int)pngd_take(z, zn, limit, &pos, 4, &bad);
  if (bad) return PNGD_TRUNCATED;
  if (hlit > 257) return PNGD_HLIT;
  if (hdist > 30) return PNGD_BAD_TABLE;
  uint8_t* cl = work;                               // [19]
  uint8_t* cltab = work + 32;                       // [128]: (length << 5) | symbol, 0 = no code
  for (int i = 0; i < 19; ++i) cl[i] = 0;
  for (int i = 0; i < hclen; ++i) {
    // the permuted order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 as arithmetic
    const int o = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;
    cl[o] = (uint8_t)pngd_take(z, zn, limit, &pos, 3, &bad);
  }
  if (bad) return PNGD_TRUNCATED;
  uint32_t k = 0;
  for (int s = 0; s < 19; ++s)
    if (cl[s]) k += 1u << (7 - cl[s]);
  if (k != 128) return PNGD_BAD_TABLE;
  for (int i = 0; i < 128; ++i) cltab[i] = 0;
  uint32_t code = 0;
  for (int l = 1; l <= 7; ++l) {                    // canonical order: by length, then by symbol
    for (int s = 0; s < 19; ++s)
      if (cl[s] == l) {
        const uint32_t r = png_reverse_bits(code++, l);
        for (uint32_t e = r; e < 128; e += 1u << l) cltab[e] = (uint8_t)((l << 5) | s);
      }
    code <<= 1;
  }
  const int total = hlit + hdist;
  int n = 0, prev = -1;
  for (int it = 0; it < 320 && n < total; ++it) {
    if (pos >= limit) return PNGD_TRUNCATED;
    const uint32_t e = cltab[pngd_window(z, zn, pos) & 127];
    const int l = e >> 5, s = e & 31;
    if (l == 0) return PNGD_BAD_TABLE;
    if (pos + l > limit) return PNGD_TRUNCATED;
    pos += l;
    if (s < 16) { lens[n++] = (uint8_t)s; prev = s; continue; }
    int rep, val;
    if (s == 16) { if (prev < 0) return PNGD_BAD_TABLE; val = prev; rep = 3 + (int)pngd_take(z, zn, limit, &pos, 2, &bad); }
    else if (s == 17) { val = 0; rep = 3 + (int)pngd_take(z, zn, limit, &pos, 3, &bad); prev = 0; }
    else { val = 0; rep = 11 + (int)pngd_take(z, zn, limit, &pos, 7, &bad); prev = 0; }
    if (bad) return PNGD_TRUNCATED;
    if (n + rep > total) return PNGD_BAD_TABLE;
    for (int q = 0; q < rep; ++q) lens[n++] = (uint8_t)val;
  }
  if (n != total) return PNGD_BAD_TABLE;
  if (lens[256] == 0) return PNGD_BAD_TABLE;
  if (pngd_kraft(lens, 257) != (1u << 15)) return PNGD_BAD_TABLE;
  // the distance code is never used, but zlib checks it: no code at all, a complete code, or a single 1-bit code
  int nd = 0, l1 = 0;
  for (int s = 0; s < hdist; ++s) { nd += lens[257 + s] != 0; l1 += lens[257 + s] == 1; }
  const uint32_t kd = pngd_kraft(lens + 257, hdist);
  if (!(nd == 0 || kd == (1u << 15) || (nd == 1 && l1 == 1))) return PNGD_BAD_TABLE;
  *data_bit = (int32_t)pos; *end_bit = (int32_t)limit;
  return PNGD_OK;
}

// canonical codes of the 257 literal lengths, bit-reversed (LSB-first): rcode[s]; next: >= 16 uint32 of work
PHD void pngd_assign_codes(const uint8_t* lens, uint16_t* rcode, uint32_t* next) {
  for (int b = 0; b <= 15; ++b) next[b] = 0;
  for (int s = 0; s < 257; ++s) next[lens[s]]++;
  next[0] = 0;
  uint32_t c = 0, cnt_prev = 0;
  for (int b = 1; b <= 15; ++b) { c = (c + cnt_prev) << 1; cnt_prev = next[b]; next[b] = c; }
  for (int s = 0; s < 257; ++s) {
    const int l = lens[s];
    rcode[s] = l ? (uint16_t)png_reverse_bits(next[l]++, l) : 0;
  }
}
// direct table over 15 bits: entry = (length << 9) | symbol, 0 = no code.  Entries k0, k0 + kstep, ... of symbol s (a kernel splits them over lanes)
PHD void pngd_fill_symbol(uint16_t* table, int s, int l, uint32_t rcode, uint32_t k0, uint32_t kstep) {
  if (l == 0) return;
  const uint32_t reps = 1u << (PNGD_TABLE_BITS - l);
  for (uint32_t k = k0; k < reps; k += kstep) table[rcode + (k << l)] = (uint16_t)((l << 9) | s);
}

PHD bool pngd_terminal(int32_t state) { return state == PNGD_END || state == PNGD_DEAD; }

PHD int32_t pngd_nsub(int32_t data_bit, int32_t end_bit, int S) {
  const int64_t bits = (int64_t)end_bit - data_bit;
  const int64_t n = bits <= 0 ? 1 : (bits + 8 * (int64_t)S - 1) / (8 * (int64_t)S);
  return (int32_t)n;
}

struct PngdSub {
  int32_t exit;        // bit position of the first symbol at or behind the subsequence's end, or PNGD_END / PNGD_DEAD
  int32_t count;       // literals decoded
  int32_t reason;      // 0, PNGD_FB_NO_CODE, PNGD_FB_PAST_END
  int32_t eob_end;     // bit position behind the end-of-block symbol, -1 = not met here
};
// Decode the symbols that start in [entry, sub_end).  out == nullptr: count only; else literal k goes to out[out_off + k] when that is
// below out_cap.  The loop runs at most 8 * S + 16 times whatever the data says (every symbol is at least one bit long).
PHD void pngd_decode_subseq(const uint8_t* z, int64_t zn, int32_t end_bit, const uint16_t* table, int32_t entry, int32_t sub_end, int S,
                            uint8_t* out, int64_t out_cap, int64_t out_off, PngdSub* r) {
  r->exit = entry; r->count = 0; r->reason = 0; r->eob_end = -1;
  if (entry == PNGD_END || entry == PNGD_DEAD) return;
  int32_t pos = entry, count = 0;
  for (int it = 0; it < 8 * S + 16 && pos < sub_end; ++it) {
    const uint32_t e = table[pngd_window(z, zn, pos) & (PNGD_TABLE_SIZE - 1)];
    const int l = e >> 9, s = e & 511;
    if (l == 0) { r->reason = PNGD_FB_NO_CODE; r->exit = PNGD_DEAD; r->count = count; return; }
    if (pos > end_bit - l) { r->reason = PNGD_FB_PAST_END; r->exit = PNGD_DEAD; r->count = count; return; }
    pos += l;
    if (s == 256) { r->eob_end = pos; r->exit = PNGD_END; r->count = count; return; }
    if (out && out_off + count < out_cap && out_off + count >= 0) out[out_off + count] = (uint8_t)s;
    ++count;
  }
  r->exit = pos; r->count = count;
}

// the verdict from the settled states: converged = every entry used equals the predecessor's exit; first_reason = the reason of the
// first subsequence that has one; eob_end = where the end-of-block symbol ended (-1: never met); total = sum of the counts
PHD int pngd_decide(int converged, int first_reason, int32_t eob_end, int64_t total, int64_t nf, int32_t end_bit) {
  if (!converged) return PNGD_FB_ROUND_CAP;
  if (first_reason) return first_reason;
  if (eob_end < 0) return PNGD_FB_PAST_END;
  if (total < nf) return PNGD_FB_EARLY_EOB;
  if (total > nf) return PNGD_FB_COUNT;
  if (((eob_end + 7) & ~7) != end_bit) return PNGD_FB_TRAILING;
  return PNGD_FB_NONE;
}

// ---- Adler-32 from partial sums (as the encoder): A = 1 + sum d_j, B = nf + sum (nf - j) d_j  (mod 65521); exact in 64 bits for nf < 2^26
PHD void pngd_adler_chunk(const uint8_t* d, int m, int64_t j0, int64_t nf, uint64_t* sa, uint64_t* sb) {
  uint64_t a = 0, ks = 0;
  for (int k = 0; k < m; ++k) { a += d[k]; ks += (uint64_t)k * d[k]; }
  *sa = a; *sb = (uint64_t)(nf - j0) * a - ks;
}
PHD uint32_t pngd_adler_finish(uint64_t sa, uint64_t sb, int64_t nf) {
  const uint64_t A = (1 + sa) % 65521ull, B = ((uint64_t)nf + sb) % 65521ull;
  return (uint32_t)((B << 16) | A);
}

// ---- un-filter: x = filtered byte, a = left, b = up, c = up-left (reconstructed bytes, 0 outside the image) ------------------
PHD uint8_t pngd_unfilter_byte(int f, int x, int a, int b, int c) {
  const int p = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
  return (uint8_t)(x + p);
}
