// jpeg_par_core.h — entropy decoding of ONE sequential-Huffman JPEG scan from many starting points at once (host/device neutral,
// same JHD convention as jpeg_core.h; csrc/jpeg_par.hip wraps it in gfx950 kernels, tests/helpers/jpeg_par_host.cpp compiles the
// same functions with g++ and runs the rounds serially).
//
// The scheme is the published one for GPU JPEG decoding (Klein & Wiseman's self-synchronisation of Huffman streams; Weissenberger &
// Schmidt's subsequence / overflow formulation):
//   * the entropy segment [scan_off, len) is cut into SUBSEQUENCES of S raw bytes;
//   * the decoder state at a symbol boundary is (raw bit position, block index inside the MCU, zigzag index z; z = 0: a DC symbol is due);
//   * subsequence 0 enters with the true start state, every other one with the guess (its first bit, block 0, z = 0); a subsequence decodes
//     every symbol that STARTS before its end and hands its exit state on;
//   * Jacobi rounds: a subsequence whose predecessor's exit differs from the entry it last decoded from decodes again from that exit.
//     When a round changes nothing, every entry equals its predecessor's exit and subsequence 0's entry is the true one: by induction the
//     states are the sequential decoder's.  Correctness never rests on self-synchronisation having happened; it only makes the rounds few.
//   * an exclusive scan of the per-subsequence block-start counts gives every subsequence the scan-order index g of its first block; the
//     writing pass decodes once more and stores AC values and the DC DIFFERENCE at g's address; a last pass turns the differences of each
//     component into DC values (inclusive wrapping 32-bit sum truncated to int16, segmented at restart intervals: what
//     jpeg_decode_block computes).
//
// Bit position: raw byte index * 8 + bit (0 = the byte's MSB).  It is canonical under byte stuffing: consuming the last bit of a data
// 0xFF steps over its stuffed 0x00 at once, so a position never names a stuffed byte and two decoders that have consumed the same
// bits hold the same number.  (JpegBits keeps an unstuffed count and a 64-bit buffer: it cannot say where in the file it is.)
//
// EQUIVALENCE with the one-lane decoder (jpeg_huffman_kernel / jpeg_decode_block) holds by construction for clean files and by
// FALLBACK for everything else: a file is handed to the lane decoder, and decoded by it as if this route did not exist, when
//   1  JPAR_BAD_CODE        a 16-bit window is no code of its table (the lane decoder skips 16 bits and goes on)
//   2  JPAR_PAST_63         a run/size pair or a ZRL moves k past 63 (the lane decoder aliases such writes to coefficient 63)
//   3  JPAR_PAST_DATA       a symbol needs bits behind a marker or behind the end of the file (the lane decoder feeds zero bits there);
//                           this covers every marker met anywhere but on an MCU boundary with fewer than 8 padding bits before it
//   4  JPAR_RST_NO_INTERVAL an RSTn while the restart interval is 0
//   5  JPAR_RST_PLACE       the k-th RSTn is not exactly at block k * interval * blocks_per_mcu, or the number of RSTn is not the
//                           number of interval boundaries inside the image
//   6  JPAR_BLOCK_COUNT     the data ends after a number of blocks other than mcus_x * mcus_y * blocks_per_mcu
//   7  JPAR_BAD_END         the data does not end with fewer than 8 padding bits followed by an EOI that lies inside the file (any
//                           other marker, 0xFF 0xFF fill bytes, a file cut short)
//   8  JPAR_ROUND_CAP       the rounds did not reach the fixed point within the cap (hostile input; never seen on an encoder's file)
// Reasons 1-4 are found by jpeg_par_decode_subseq, 5-7 by jpeg_par_check_place / jpeg_par_check_end from the settled states, 8 by the
// driver.  All of them are known BEFORE the writing pass, so a file that falls back has written nothing: its coefficients are still zero,
// as the lane decoder requires.
#pragma once
#include "jpeg_core.h"

// The product geometry (reasoning next to the kernels, csrc/jpeg_par.hip); the host helper takes all of them at run time.
#define JPEG_PAR_S 128            // raw bytes per subsequence
#define JPEG_PAR_SPAN 256         // subsequences per workgroup span (one per lane)
#define JPEG_PAR_ROUND_CAP 4      // cross-span rounds (launches) after the speculative one
#define JPEG_PAR_LOCAL_CAP JPEG_PAR_SPAN   // Jacobi iterations a workgroup runs over its own span per launch: enough to settle it whatever the data
#define JPEG_PAR_LB 10            // lookahead bits of the shared direct tables

enum {
  JPAR_OK = 0, JPAR_BAD_CODE = 1, JPAR_PAST_63 = 2, JPAR_PAST_DATA = 3, JPAR_RST_NO_INTERVAL = 4, JPAR_RST_PLACE = 5,
  JPAR_BLOCK_COUNT = 6, JPAR_BAD_END = 7, JPAR_ROUND_CAP = 8,
};
enum { JPAR_END = 1 << 16,       // the data ended here (marker other than RSTn, or end of file, met on an MCU boundary): pos = that byte * 8
       JPAR_DEAD = 1 << 17 };    // a decode that ran out of data: its successors decode nothing

struct JpegParState {            // 8 bytes: moved as one word
  int32_t pos;                   // raw bit position (files of 2^28 bytes and more are not eligible)
  int32_t bz;                    // block in MCU * 64 + z, or JPAR_END / JPAR_DEAD
};
JHD bool jpeg_par_same(JpegParState a, JpegParState b) { return a.pos == b.pos && a.bz == b.bz; }

struct JpegParResult {
  JpegParState exit;
  int32_t nblocks;               // block starts (DC symbols) met
  int32_t nrst;                  // RSTn met
  int32_t first_rst;             // nblocks when the first RSTn was met, -1 = none
  int32_t reason;                // JPAR_OK or 1-4
};

struct JpegParFile {             // what the passes need of a JpegInfo, without dynamically indexed arrays
  int64_t len;
  int32_t scan_off, ncomp, bpm /* blocks per MCU */, nb0 /* of which component 0's */, hs0, vs0, mcus_x, mcus_y, interval;
  int32_t tsel;                  // bit c: DC table id of component c; bit 4 + c: its AC table id
  int32_t total_blocks;
};

JHD void jpeg_par_file_init(const JpegInfo* o, int64_t len, JpegParFile* f) {
  f->len = len; f->scan_off = o->scan_off; f->ncomp = o->ncomp;
  f->hs0 = o->hs[0]; f->vs0 = o->vs[0]; f->nb0 = o->hs[0] * o->vs[0];
  f->bpm = f->nb0 + (o->ncomp == 3 ? 2 : 0);
  f->mcus_x = o->mcus_x; f->mcus_y = o->mcus_y; f->interval = o->restart_interval;
  f->tsel = (o->td[0] & 1) | ((o->ta[0] & 1) << 4);
  if (o->ncomp == 3) f->tsel |= ((o->td[1] & 1) << 1) | ((o->td[2] & 1) << 2) | ((o->ta[1] & 1) << 5) | ((o->ta[2] & 1) << 6);
  f->total_blocks = o->mcus_x * o->mcus_y * f->bpm;      // <= 2^24 pixels / 64 * 3
}

// sequential, single scan, and small enough for 32-bit bit positions
JHD bool jpeg_par_eligible(const JpegInfo* o, int64_t len) {
  return o->status == 0 && !o->progressive && len < ((int64_t)1 << 28) && o->scan_off > 0 && o->scan_off < len;
}
JHD int64_t jpeg_par_subseqs(int64_t scan_off, int64_t len, int S) { return (len - scan_off + S - 1) / S; }

// ---------------------------------------------------------------------------------------------- bits
// 32 bits from (bp, bo), MSB first, stuffing removed; *avail = how many bits from (bp, bo) on are DATA (the rest are the zero bits the
// lane decoder would feed behind a marker / the end of the file).  Reads d[bp .. bp + 10) at most, with bp < len.
// *stop: where the data stops when avail < 33 (the byte index of a marker's 0xFF, or len).
JHD uint32_t jpeg_par_peek(const uint8_t* d, int64_t len, int64_t bp, int bo, int* avail, int64_t* stop) {
  if (bp + 8 <= len) {
    uint64_t w;
    __builtin_memcpy(&w, d + bp, 8);                                   // first stream byte in bits 0-7
    const uint64_t v = ~w | 0xFFFFFF0000000000ull;                     // a zero byte of v = an 0xFF among the first five stream bytes
    if (((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) == 0) {
      *avail = 40 - bo;
      return (uint32_t)((__builtin_bswap64(w) << bo) >> 32);
    }
  }
  uint64_t acc = 0;
  int nb = 0;
  int64_t p = bp;
  while (nb < 40 && p < len) {
    const unsigned byte = d[p];
    if (byte == 0xFF) {
      if (p + 1 < len && d[p + 1] == 0) p += 2;                        // stuffed zero
      else break;                                                      // marker (an 0xFF that ends the file counts as one)
    } else {
      p += 1;
    }
    acc |= (uint64_t)byte << (56 - nb);
    nb += 8;
  }
  *avail = nb - bo;
  *stop = p;
  return (uint32_t)((acc << bo) >> 32);
}
// n <= avail bits on: every byte stepped over is data
JHD void jpeg_par_advance(const uint8_t* d, int64_t* bp, int* bo, int n) {
  int t = *bo + n;
  int64_t p = *bp;
  while (t >= 8) { p += d[p] == 0xFF ? 2 : 1; t -= 8; }
  *bp = p; *bo = t;
}

// A symbol ran into a marker: if it is an RSTn, a decode can go on behind it with (block 0, z = 0) — the file is damaged if its TRUE decode
// gets here (reason 3 stays on the subsequence), but a speculative decode from a wrong entry gets here at every marker of a file with
// restart intervals, and behind the marker it holds the true state.
JHD bool jpeg_par_resync(const uint8_t* d, int64_t len, int64_t stop) {
  return stop + 1 < len && d[stop] == 0xFF && d[stop + 1] >= 0xD0 && d[stop + 1] <= 0xD7;
}

// one code of table t out of a 16-bit window; *len = 0: the window is no code
template <typename T>
JHD int jpeg_par_symbol(uint32_t w16, T t, int* len) {
  const unsigned e = t.lut((int)(w16 >> (16 - T::LB)));
  if (e) { *len = (int)(e >> 8); return (int)(e & 255); }
  uint32_t first = t.limk(T::LB) & 0xFFFFu;
  for (int l = T::LB + 1; l <= 16; ++l) {
    const uint32_t lk = t.limk(l);
    if (w16 < (lk & 0xFFFFu)) {
      *len = l;
      return t.val((int)(((lk >> 16) + ((w16 - first) >> (16 - l))) & (T::NV - 1)));
    }
    first = lk & 0xFFFFu;
  }
  *len = 0;
  return 0;
}

// ---------------------------------------------------------------------------------------------- states
JHD JpegParState jpeg_par_start(const JpegParFile* f) { JpegParState s; s.pos = f->scan_off * 8; s.bz = 0; return s; }

// the guess for subsequence s > 0: its first bit, block 0, z = 0 — moved off a stuffed zero (no position names one) and off the second
// byte of an RSTn (behind the marker the guess IS the true state: files with restart intervals synchronise at once)
JHD JpegParState jpeg_par_guess(const uint8_t* d, const JpegParFile* f, int64_t s, int S) {
  int64_t b = f->scan_off + s * S;
  if (d[b - 1] == 0xFF && (d[b] == 0 || (d[b] >= 0xD0 && d[b] <= 0xD7))) b += 1;
  JpegParState st; st.pos = (int32_t)(b * 8); st.bz = 0;
  return st;
}

struct JpegParNoSink {
  JHD void operator()(int, int, int) const {}
};

// Decodes every symbol that starts before byte `end` (<= len) from the entry state `in`.  tab.dc(id) / tab.ac(id), id 0 | 1: table views
// as in jpeg_core.h; nat: zigzag -> natural order.  sink(block ordinal within the subsequence, natural index, value): the ordinal of
// the first block STARTED here is 0, the block an entry with z > 0 continues has ordinal -1; index 0 carries the DC difference.
// Never reads outside [0, len + JPEG_TAIL_PAD).
template <typename TAB, typename NAT, typename SINK>
JHD void jpeg_par_decode_subseq(const uint8_t* d, const JpegParFile* f, TAB tab, NAT nat, JpegParState in, int64_t end, SINK sink,
                                JpegParResult* out) {
  out->exit = in; out->nblocks = 0; out->nrst = 0; out->first_rst = -1; out->reason = JPAR_OK;
  if (in.bz & (JPAR_END | JPAR_DEAD)) return;
  const int64_t len = f->len;
  int64_t bp = in.pos >> 3;
  int bo = in.pos & 7;
  int blk = (in.bz >> 6) & 15, z = in.bz & 63;
  int nblocks = 0, nrst = 0, last_rst = 0;
  int reason = JPAR_OK;        // a decode that cannot go on (no data left before a marker other than RSTn / the end): the exit is JPAR_DEAD
  int soft = JPAR_OK;          // every other reason: the decode goes on (a code of 16 bits with symbol 0; the block ends; behind an RSTn), so
                               // that a SPECULATIVE decode from a wrong entry, which meets these all the time, can still synchronise
  if (bp < f->scan_off || blk >= f->bpm) reason = JPAR_PAST_DATA;            // (no state this code hands on; a caller's garbage)
  while (!reason && bp < end) {
    if (z == 0 && blk == 0) {
      // MCU boundary: the bits left in this byte are padding if a marker follows
      const int64_t q = bo ? bp + (d[bp] == 0xFF ? 2 : 1) : bp;
      if (q >= len || (d[q] == 0xFF && !(q + 1 < len && d[q + 1] == 0))) {
        const int m = q + 1 < len ? d[q + 1] : 0;
        if (q < len && m >= 0xD0 && m <= 0xD7) {
          if (f->interval == 0) soft = JPAR_RST_NO_INTERVAL;
          if (nrst == 0) out->first_rst = nblocks;
          else if (nblocks - last_rst != f->interval * f->bpm) soft = JPAR_RST_PLACE;
          last_rst = nblocks;
          ++nrst;
          bp = q + 2; bo = 0;
          continue;
        }
        out->exit.pos = (int32_t)(q * 8); out->exit.bz = JPAR_END;
        out->nblocks = nblocks; out->nrst = nrst; out->reason = soft;
        return;
      }
    }
    int avail;
    int64_t stop = 0;
    const uint32_t w = jpeg_par_peek(d, len, bp, bo, &avail, &stop);
    const int c = blk < f->nb0 ? 0 : blk - f->nb0 + 1;
    int l, n;
    if (z == 0) {
      const int s = jpeg_par_symbol(w >> 16, tab.dc((f->tsel >> c) & 1), &l) & 15;
      if (l == 0) { soft = JPAR_BAD_CODE; l = 16; }
      n = l + s;
      if (n > avail) {
        if (jpeg_par_resync(d, len, stop)) { soft = JPAR_PAST_DATA; ++nrst; bp = stop + 2; bo = 0; blk = 0; z = 0; continue; }
        reason = JPAR_PAST_DATA; break;
      }
      ++nblocks;
      if (s) {
        const int r = (int)((w << l) >> (32 - s));
        sink(nblocks - 1, 0, r < (1 << (s - 1)) ? r - (1 << s) + 1 : r);
      }
      z = 1;
    } else {
      const int rs = jpeg_par_symbol(w >> 16, tab.ac((f->tsel >> (4 + c)) & 1), &l);
      if (l == 0) { soft = JPAR_BAD_CODE; l = 16; }
      const int run = rs >> 4, s = rs & 15;
      n = l + s;
      if (n > avail) {
        if (jpeg_par_resync(d, len, stop)) { soft = JPAR_PAST_DATA; ++nrst; bp = stop + 2; bo = 0; blk = 0; z = 0; continue; }
        reason = JPAR_PAST_DATA; break;
      }
      if (s) {
        const int k = z + run;
        if (k > 63) {
          soft = JPAR_PAST_63;
        } else {
          const int r = (int)((w << l) >> (32 - s));
          sink(nblocks - 1, (int)nat[k], r < (1 << (s - 1)) ? r - (1 << s) + 1 : r);
        }
        z = k + 1;
      } else if (run == 15) {
        if (z + 15 > 63) soft = JPAR_PAST_63;
        z += 16;
      } else {
        z = 64;                                                               // end of block
      }
    }
    if (z >= 64) { z = 0; if (++blk == f->bpm) blk = 0; }
    jpeg_par_advance(d, &bp, &bo, n);
  }
  out->nblocks = nblocks; out->nrst = nrst; out->reason = reason ? reason : soft;
  if (reason) { out->exit.pos = 0; out->exit.bz = JPAR_DEAD; }
  else { out->exit.pos = (int32_t)(bp * 8 + bo); out->exit.bz = blk * 64 + z; }
}

// ---------------------------------------------------------------------------------------------- checks on the settled states
// a subsequence whose first block has scan-order index gbase and which `rbase` RSTn precede: its first RSTn must be the (rbase + 1)-th
// interval boundary (the later ones of the same subsequence are interval * bpm blocks apart: jpeg_par_decode_subseq saw to it)
JHD int jpeg_par_check_place(const JpegParFile* f, const JpegParResult* r, int64_t gbase, int64_t rbase) {
  if (r->reason) return r->reason;
  if (r->nrst && gbase + r->first_rst != (rbase + 1) * (int64_t)f->interval * f->bpm) return JPAR_RST_PLACE;
  return JPAR_OK;
}
// the last subsequence's exit, the block and RSTn totals
JHD int jpeg_par_check_end(const uint8_t* d, const JpegParFile* f, JpegParState last, int64_t blocks, int64_t rsts) {
  if (last.bz & JPAR_DEAD) return JPAR_PAST_DATA;
  if (blocks != f->total_blocks) return JPAR_BLOCK_COUNT;
  const int64_t mcus = (int64_t)f->mcus_x * f->mcus_y;
  if (rsts != (f->interval ? (mcus - 1) / f->interval : 0)) return JPAR_RST_PLACE;
  if (!(last.bz & JPAR_END)) return JPAR_BAD_END;
  const int64_t p = last.pos >> 3;
  if (p + 2 > f->len || d[p] != 0xFF || d[p + 1] != 0xD9) return JPAR_BAD_END;
  return JPAR_OK;
}

// ---------------------------------------------------------------------------------------------- placement
// scan-order block index g (0 <= g < total_blocks) -> offset of the block in the file's coefficient planes (int16 elements; the planes
// of components 0, 1, 2 follow each other, row stride mcus_x * hs blocks: jpeg_huffman_kernel's layout)
JHD int64_t jpeg_par_block_offset(const JpegParFile* f, int64_t g) {
  const int64_t m = g / f->bpm;
  const int b = (int)(g - m * f->bpm);
  const int my = (int)(m / f->mcus_x), mx = (int)(m - (int64_t)my * f->mcus_x);
  if (b < f->nb0) {
    const int v = b / f->hs0, h = b - v * f->hs0;
    return ((int64_t)(my * f->vs0 + v) * (f->mcus_x * f->hs0) + mx * f->hs0 + h) * 64;
  }
  const int64_t n0 = (int64_t)f->mcus_x * f->hs0 * f->mcus_y * f->vs0, n1 = (int64_t)f->mcus_x * f->mcus_y;
  return (n0 + (b - f->nb0) * n1 + (int64_t)my * f->mcus_x + mx) * 64;
}
// blocks of component c in the scan, and the j-th of them: its offset, and whether a restart segment (DC prediction 0) begins with it
JHD int64_t jpeg_par_comp_blocks(const JpegParFile* f, int c) { return (int64_t)f->mcus_x * f->mcus_y * (c == 0 ? f->nb0 : 1); }
JHD int64_t jpeg_par_comp_block(const JpegParFile* f, int c, int64_t j, bool* seg_start) {
  const int per = c == 0 ? f->nb0 : 1;
  const int64_t m = j / per;
  const int b = (int)(j - m * per);
  *seg_start = b == 0 && (f->interval ? m % f->interval == 0 : m == 0);
  return jpeg_par_block_offset(f, m * f->bpm + (c == 0 ? b : f->nb0 + c - 1));
}

// The DC pass over one chunk [j0, j1) of a component's blocks: `carry` = the running sum entering the chunk.  With store = false it only
// returns the chunk's own sum since its last segment start (*reset says whether it had one), so that chunks can be combined.
JHD uint32_t jpeg_par_dc_chunk(const JpegParFile* f, int16_t* coef, int c, int64_t j0, int64_t j1, uint32_t carry, bool store, bool* reset) {
  uint32_t sum = carry;
  bool rs = false;
  for (int64_t j = j0; j < j1; ++j) {
    bool seg;
    int16_t* blk = coef + jpeg_par_comp_block(f, c, j, &seg);
    if (seg) { sum = 0; rs = true; }
    sum += (uint32_t)(int32_t)blk[0];
    if (store) blk[0] = (int16_t)sum;
  }
  *reset = rs;
  return sum;
}
