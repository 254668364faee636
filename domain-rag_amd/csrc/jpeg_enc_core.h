// jpeg_enc_core.h — baseline JPEG ENCODING arithmetic, byte-identical to what Pillow writes for `Image.save(path)` of an RGB
// or L image (libjpeg's default compression path: fixed-point RGB -> YCbCr, box downsampling without smoothing, the "ISLOW"
// integer forward DCT, quantisation by the quality-scaled Annex K tables, the Annex K Huffman tables, one interleaved scan).
// The reference writes its stage-0 results that way (lama_inpaint/lama_inpaint.py:211, `result.save(output_filename)`), and
// those .jpg files are the inputs of stages 1 and 2: an encoder that replaces Pillow there has to write Pillow's bytes.
// The algorithms restated here are libjpeg's published ones (jccolor, jcsample, jfdctint, jcdctmgr, jcparam, jchuff, jcmarker).
//
// Host/device neutral like jpeg_core.h: csrc/jpeg_enc.hip runs these functions in gfx950 kernels (one thread per plane
// sample / per 8x8 block / per chunk of stream bytes), tests/helpers/jpeg_enc_host.cpp composes the very same functions serially
// under g++ so that the arithmetic is checked against Pillow where there is no GPU.
//
// Offered: 8-bit RGB (3 components, 4:4:4 / 4:2:2 / 4:2:0) and grey (1 component), quality 1..100, the standard tables.
// Not offered: optimised Huffman tables, progressive scans, restart markers.
#pragma once
#include <stdint.h>

#if !defined(JHD)
#if defined(__HIPCC__)
#define JHD __host__ __device__ __forceinline__
#else
#define JHD inline
#endif
#endif

enum {
  JPEG_ENC_BLOCK_BYTES = 256,     // unstuffed stream bytes reserved per 8x8 block.  What the Annex K tables can code at all: a DC
                                  // difference of category 11 at most (9-bit code) and 63 AC coefficients of category 10 at most behind
                                  // 16-bit codes = 20 + 63 * 26 = 1658 bits (208 bytes); 8-bit samples with q >= 1 cannot exceed these
                                  // categories (libjpeg raises an error there; here a larger magnitude would find no symbol and be
                                  // dropped from the stream, never written past the block's reserve: at most 28 + 63 * 27 bits)
  JPEG_ENC_HEADER_MAX = 640,      // SOI .. SOS of a colour file is 623 bytes, of a grey file 333
  JPEG_ENC_TAB = 272,             // one Huffman pair as (length << 16) | code: [0, 16) DC by category, [16, 272) AC by run/size symbol
};

JHD int jpeg_enc_zigzag(int k) {   // zigzag position -> natural (row-major) position
  const uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}

// ---------------------------------------------------------------------------------------------- geometry
// One interleaved scan: an MCU holds hs x vs luminance blocks (row-major) and, for colour, one Cb and one Cr block.
// A component's padded plane covers every block position of every MCU, dummy ones included.
struct JpegEncGeom {
  int32_t W, H, ncomp;
  int32_t hs, vs;                 // luminance sampling factors (chroma is 1 x 1)
  int32_t mcus_x, mcus_y;
  int32_t bpm;                    // blocks per MCU
  int32_t pw[3], ph[3];           // padded plane size per component (samples)
  int32_t wb[3], hb[3];           // REAL blocks per component: ceil(component width / 8), ceil(component height / 8)
  int64_t plane_off[3];           // byte offset of a component's plane inside the image's plane region
  int64_t plane_bytes;            // all planes of one image
  int64_t nblocks;                // blocks per image in scan order = mcus_x * mcus_y * bpm
};

// subsampling: Pillow's numbers, 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (ignored for grey)
JHD void jpeg_enc_geometry(int W, int H, int C, int subsampling, JpegEncGeom* g) {
  g->W = W; g->H = H; g->ncomp = C == 1 ? 1 : 3;
  g->hs = (C == 1 || subsampling == 0) ? 1 : 2;
  g->vs = (C != 1 && subsampling == 2) ? 2 : 1;
  g->mcus_x = (W + 8 * g->hs - 1) / (8 * g->hs);
  g->mcus_y = (H + 8 * g->vs - 1) / (8 * g->vs);
  g->bpm = g->hs * g->vs + (g->ncomp == 3 ? 2 : 0);
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    const int h = c == 0 ? g->hs : 1, v = c == 0 ? g->vs : 1;
    const bool used = c < g->ncomp;
    const int cw = (W * h + g->hs - 1) / g->hs, ch = (H * v + g->vs - 1) / g->vs;       // component size in samples
    g->pw[c] = used ? g->mcus_x * 8 * h : 0;
    g->ph[c] = used ? g->mcus_y * 8 * v : 0;
    g->wb[c] = used ? (cw + 7) / 8 : 0;
    g->hb[c] = used ? (ch + 7) / 8 : 0;
    g->plane_off[c] = off;
    off += (int64_t)g->pw[c] * g->ph[c];
  }
  g->plane_bytes = off;
  g->nblocks = (int64_t)g->mcus_x * g->mcus_y * g->bpm;
}

// ---------------------------------------------------------------------------------------------- colour, edges, downsampling
// jccolor.c's tables as their closed form (16-bit fixed point; the chroma rounding constant is ONE_HALF - 1)
JHD int jpeg_enc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
JHD int jpeg_enc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
JHD int jpeg_enc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// component c of the pixel at (x, y), x < W, y < H; img is [H, W, C] dense
JHD int jpeg_enc_pixel(const uint8_t* img, const JpegEncGeom& g, int c, int x, int y) {
  if (g.ncomp == 1) return img[(int64_t)y * g.W + x];
  const uint8_t* p = img + ((int64_t)y * g.W + x) * 3;
  return c == 0 ? jpeg_enc_y(p[0], p[1], p[2]) : c == 1 ? jpeg_enc_cb(p[0], p[1], p[2]) : jpeg_enc_cr(p[0], p[1], p[2]);
}

// sample (x, y) of component c's padded plane.  The edges as libjpeg makes them: columns are replicated on the full-resolution
// converted plane and then downsampled; rows are replicated up to a whole row group (an even height at 4:2:0), downsampled, and
// the LAST DOWNSAMPLED ROW is replicated down to the MCU height.
JHD uint8_t jpeg_enc_sample(const uint8_t* img, const JpegEncGeom& g, int c, int x, int y) {
  const int W = g.W, H = g.H;
  if (c == 0 || (g.hs == 1 && g.vs == 1)) {
    return (uint8_t)jpeg_enc_pixel(img, g, c, x < W ? x : W - 1, y < H ? y : H - 1);
  }
  const int x0 = 2 * x < W ? 2 * x : W - 1, x1 = 2 * x + 1 < W ? 2 * x + 1 : W - 1;
  if (g.vs == 1) {                                                        // h2v1: bias 0, 1, 0, 1, ...
    const int yy = y < H ? y : H - 1;
    return (uint8_t)((jpeg_enc_pixel(img, g, c, x0, yy) + jpeg_enc_pixel(img, g, c, x1, yy) + (x & 1)) >> 1);
  }
  const int rows = (H + 1) / 2;                                           // downsampled rows that exist
  const int yo = y < rows ? y : rows - 1;
  const int y0 = 2 * yo < H ? 2 * yo : H - 1, y1 = 2 * yo + 1 < H ? 2 * yo + 1 : H - 1;
  return (uint8_t)((jpeg_enc_pixel(img, g, c, x0, y0) + jpeg_enc_pixel(img, g, c, x1, y0) + jpeg_enc_pixel(img, g, c, x0, y1) +
                    jpeg_enc_pixel(img, g, c, x1, y1) + 1 + (x & 1)) >> 2);             // h2v2: bias 1, 2, 1, 2, ...
}

// ---------------------------------------------------------------------------------------------- block order, dummy blocks
struct JpegEncBlock {
  int32_t comp;                   // component
  int32_t bx, by;                 // position of the block whose SAMPLES are transformed (for a dummy block: its DC source)
  int32_t dummy;                  // 1 = beyond the component's real blocks: AC zero, DC copied from the source block
  int64_t pred;                   // scan index of the previous block of the same component (the DC predictor), -1 = none
};

// block b (scan order) of an image.  A dummy block at the right edge takes the DC of the block to its left; a dummy block ROW at the
// bottom takes the DC of the last block of the row above it in the same MCU (which may itself be a right-edge dummy).
JHD void jpeg_enc_block(const JpegEncGeom& g, int64_t b, JpegEncBlock* o) {
  const int64_t mcu = b / g.bpm;
  const int k = (int)(b - mcu * g.bpm);
  const int mx = (int)(mcu % g.mcus_x), my = (int)(mcu / g.mcus_x);
  const int nl = g.hs * g.vs;
  if (k < nl) {
    int kx = k % g.hs, ky = k / g.hs;
    o->comp = 0;
    o->pred = k > 0 ? b - 1 : (mcu > 0 ? b - g.bpm + nl - 1 : -1);
    o->dummy = 0;
    if (my * g.vs + ky >= g.hb[0]) { o->dummy = 1; ky -= 1; kx = g.hs - 1; }       // (vs == 2, ky == 1: the last block of row 0)
    if (mx * g.hs + kx >= g.wb[0]) { o->dummy = 1; kx -= 1; }                      // (hs == 2, kx == 1)
    o->bx = mx * g.hs + kx; o->by = my * g.vs + ky;
  } else {
    o->comp = 1 + (k - nl);
    o->pred = mcu > 0 ? b - g.bpm : -1;
    o->dummy = 0;
    o->bx = mx; o->by = my;
  }
}

// ---------------------------------------------------------------------------------------------- forward DCT + quantisation
#define JPEG_ENC_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
// jfdctint.c (ISLOW): CONST_BITS 13, PASS1_BITS 2; d: 64 samples minus 128, row-major, transformed in place; outputs 8x scaled
JHD void jpeg_enc_fdct(int32_t* d) {
  const int32_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int st = pass == 0 ? 1 : 8, step = pass == 0 ? 8 : 1;          // element stride inside a line, stride between lines
    const int n = pass == 0 ? 11 : 15;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      int32_t* p = d + l * step;
      const int32_t t0 = p[0] + p[7 * st], t7 = p[0] - p[7 * st], t1 = p[st] + p[6 * st], t6 = p[st] - p[6 * st];
      const int32_t t2 = p[2 * st] + p[5 * st], t5 = p[2 * st] - p[5 * st], t3 = p[3 * st] + p[4 * st], t4 = p[3 * st] - p[4 * st];
      const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
      if (pass == 0) {
        p[0] = (t10 + t11) * 4;                                 // (<< PASS1_BITS)
        p[4 * st] = (t10 - t11) * 4;
      } else {
        p[0] = JPEG_ENC_DESCALE(t10 + t11, 2);
        p[4 * st] = JPEG_ENC_DESCALE(t10 - t11, 2);
      }
      int32_t z1 = (t12 + t13) * F0_541;
      p[2 * st] = JPEG_ENC_DESCALE(z1 + t13 * F0_765, n);
      p[6 * st] = JPEG_ENC_DESCALE(z1 + t12 * (-F1_847), n);
      z1 = t4 + t7;
      int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
      const int32_t z5 = (z3 + z4) * F1_175;
      const int32_t u4 = t4 * F0_298, u5 = t5 * F2_053, u6 = t6 * F3_072, u7 = t7 * F1_501;
      z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
      z3 += z5; z4 += z5;
      p[7 * st] = JPEG_ENC_DESCALE(u4 + z1 + z3, n);
      p[5 * st] = JPEG_ENC_DESCALE(u5 + z2 + z4, n);
      p[3 * st] = JPEG_ENC_DESCALE(u6 + z2 + z3, n);
      p[st] = JPEG_ENC_DESCALE(u7 + z1 + z4, n);
    }
  }
}

// jcdctmgr.c: the DCT output is 8x scaled, so the divisor is 8 * q; round half away from zero
JHD int jpeg_enc_quantise(int32_t c, int q) {
  const int32_t d = 8 * q;
  return c >= 0 ? (c + (d >> 1)) / d : -((-c + (d >> 1)) / d);
}

// entry k (natural order) of quantisation table `which` (0 luminance, 1 chrominance) at `quality` 1..100: Annex K.1 / K.2 scaled
// as jcparam.c does it (jpeg_quality_scaling, force_baseline)
JHD int jpeg_enc_quant(int which, int quality, int k) {
  const uint8_t lum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                           69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                           81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  const uint8_t chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = ((which == 0 ? lum[k] : chr[k]) * scale + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// block (bx, by) of a padded plane (row stride pw) -> 64 quantised coefficients in ZIGZAG order; qt: the table in natural order
JHD void jpeg_enc_block_coefs(const uint8_t* plane, int pw, int bx, int by, const uint16_t* qt, int dummy, int16_t* out) {
  int32_t d[64];
  const uint8_t* s = plane + (int64_t)by * 8 * pw + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint64_t v = *(const uint64_t*)(s + (int64_t)r * pw);          // planes and their rows are 8-byte aligned (pw % 8 == 0)
#pragma unroll
    for (int c = 0; c < 8; ++c) d[r * 8 + c] = (int32_t)((v >> (8 * c)) & 0xff) - 128;
  }
  jpeg_enc_fdct(d);
  out[0] = (int16_t)jpeg_enc_quantise(d[0], qt[0]);
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int nat = jpeg_enc_zigzag(k);
    out[k] = dummy ? (int16_t)0 : (int16_t)jpeg_enc_quantise(d[nat], qt[nat]);
  }
}

// ---------------------------------------------------------------------------------------------- Huffman tables (Annex K.3 - K.6)
// table t: 0 = DC luminance, 1 = AC luminance, 2 = DC chrominance, 3 = AC chrominance (the order the DHT segments are written in)
JHD int jpeg_enc_huff_bits(int t, int l) {   // number of codes of length l = 1..16
  const uint8_t b[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                            {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                            {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                            {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
  return b[t][l - 1];
}
JHD int jpeg_enc_huff_count(int t) { return (t & 1) ? 162 : 12; }
JHD int jpeg_enc_huff_val(int t, int k) {    // k-th symbol in code order
  const uint8_t acl[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  const uint8_t acc[162] = {
      0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  if (!(t & 1)) return k;                    // both DC tables list the categories 0..11 in order
  return t == 1 ? acl[k] : acc[k];
}

// the canonical code of the k-th symbol of table t as (length << 16) | code: every symbol finds its own code in 16 steps, so a
// workgroup derives a whole table with one symbol per thread
JHD uint32_t jpeg_enc_huff_code(int t, int k) {
  uint32_t code = 0;
  int cum = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = jpeg_enc_huff_bits(t, l);
    if (k < cum + n) return ((uint32_t)l << 16) | (code + (uint32_t)(k - cum));
    code = (code + (uint32_t)n) << 1;
    cum += n;
  }
  return 0;
}

// slot of table t's k-th symbol in a JPEG_ENC_TAB-entry pair table (pair 0 = luminance tables 0 / 1, pair 1 = chrominance 2 / 3)
JHD int jpeg_enc_tab_slot(int t, int k) { return (t & 1) ? 16 + jpeg_enc_huff_val(t, k) : jpeg_enc_huff_val(t, k); }

// ---------------------------------------------------------------------------------------------- entropy coding of one block
JHD int jpeg_enc_bitlen(int v) {             // bits needed for a magnitude v >= 0
  return v ? 32 - __builtin_clz((unsigned)v) : 0;
}

// jchuff.c encode_one_block: zz = the block's coefficients in zigzag order, last_dc = the DC of the previous block of the component,
// tab = the component's pair table.  Every code goes to put(bits, length) together with the value bits behind it (at most 27 bits):
// a counting `put` gives the block's coded length, a writing one the stream.
template <typename Put>
JHD void jpeg_enc_block_codes(const int16_t* zz, int last_dc, const uint32_t* tab, Put& put) {
  int t = (int)zz[0] - last_dc, t2 = t;
  if (t < 0) { t = -t; --t2; }
  int nb = jpeg_enc_bitlen(t);
  uint32_t e = tab[nb & 15];
  put(((e & 0xffffu) << nb) | ((uint32_t)t2 & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
  int r = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {                                         // (unrolled: zz stays in registers on the device)
    t = zz[k];
    if (t == 0) { ++r; continue; }
    while (r > 15) { e = tab[16 + 0xF0]; put(e & 0xffffu, (int)(e >> 16)); r -= 16; }
    t2 = t;
    if (t < 0) { t = -t; --t2; }
    nb = jpeg_enc_bitlen(t);
    e = tab[16 + (((r << 4) + nb) & 255)];
    put(((e & 0xffffu) << nb) | ((uint32_t)t2 & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
    r = 0;
  }
  if (r > 0) { e = tab[16]; put(e & 0xffffu, (int)(e >> 16)); }
}

struct JpegEncCountBits {
  uint32_t bits = 0;
  JHD void operator()(uint32_t, int len) { bits += (uint32_t)len; }
};

// ---------------------------------------------------------------------------------------------- header
// SOI, APP0 (JFIF 1.01, no density), DQT 0 (and 1), SOF0, DHT DC0 AC0 (DC1 AC1), SOS: the segments jcmarker.c writes for Pillow's
// default save, in its order.  out: JPEG_ENC_HEADER_MAX bytes.  Returns the header's length.
JHD int jpeg_enc_header(const JpegEncGeom& g, int quality, uint8_t* out) {
  int n = 0;
  const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 20; ++i) out[n++] = app0[i];
  const int ntab = g.ncomp == 3 ? 2 : 1;
  for (int t = 0; t < ntab; ++t) {
    out[n++] = 0xFF; out[n++] = 0xDB; out[n++] = 0; out[n++] = 67; out[n++] = (uint8_t)t;
    for (int k = 0; k < 64; ++k) out[n++] = (uint8_t)jpeg_enc_quant(t, quality, jpeg_enc_zigzag(k));
  }
  out[n++] = 0xFF; out[n++] = 0xC0; out[n++] = 0; out[n++] = (uint8_t)(8 + 3 * g.ncomp); out[n++] = 8;
  out[n++] = (uint8_t)(g.H >> 8); out[n++] = (uint8_t)g.H; out[n++] = (uint8_t)(g.W >> 8); out[n++] = (uint8_t)g.W;
  out[n++] = (uint8_t)g.ncomp;
  for (int c = 0; c < g.ncomp; ++c) {
    out[n++] = (uint8_t)(c + 1);
    out[n++] = c == 0 ? (uint8_t)((g.hs << 4) | g.vs) : (uint8_t)0x11;
    out[n++] = c == 0 ? 0 : 1;
  }
  for (int t = 0; t < 2 * ntab; ++t) {
    const int cnt = jpeg_enc_huff_count(t);
    out[n++] = 0xFF; out[n++] = 0xC4; out[n++] = 0; out[n++] = (uint8_t)(2 + 1 + 16 + cnt);
    out[n++] = (uint8_t)(((t & 1) << 4) | (t >> 1));
    for (int l = 1; l <= 16; ++l) out[n++] = (uint8_t)jpeg_enc_huff_bits(t, l);
    for (int k = 0; k < cnt; ++k) out[n++] = (uint8_t)jpeg_enc_huff_val(t, k);
  }
  out[n++] = 0xFF; out[n++] = 0xDA; out[n++] = 0; out[n++] = (uint8_t)(6 + 2 * g.ncomp); out[n++] = (uint8_t)g.ncomp;
  for (int c = 0; c < g.ncomp; ++c) { out[n++] = (uint8_t)(c + 1); out[n++] = c == 0 ? 0x00 : 0x11; }
  out[n++] = 0; out[n++] = 63; out[n++] = 0;
  return n;
}
