// jpeg_enc.hip — uint8 images in HBM -> complete baseline JPEG files in HBM (gfx950), byte-identical to Pillow's `Image.save`:
// the functions of jpeg_enc_core.h run in parallel.  Replaces the reference's host-side `result.save(output_filename)` of its
// stage-0 frames (lama_inpaint/lama_inpaint.py:211).  A batch of n same-size images is encoded by eight stream-ordered launches,
// no host round trip in between; the caller reads the n file sizes and copies the bytes out.
//
//   1 jpeg_enc_planes_kernel  one thread per sample of the padded component planes: RGB -> YCbCr, edge replication, downsampling
//   2 jpeg_enc_dct_kernel     one thread per 8x8 block in scan order, dummy blocks included: FDCT + quantisation -> int16, zigzag order
//   3 jpeg_enc_bits_kernel    one thread per block: its coded length in bits (DC difference against its predecessor in scan order)
//   4 jpeg_enc_scan_kernel    exclusive scan of the block lengths (one workgroup per image)
//   5 jpeg_enc_pack_kernel    one thread per block: codes shifted into a 64-bit window MSB first, whole words stored, the two
//                             boundary words atomicOr-ed (the buffer is zeroed first: deterministic)
//   6 jpeg_enc_ff_kernel      one thread per 64-byte chunk of the stream: the 0xFF bytes in it (each gets a 0x00 behind it)
//   7 jpeg_enc_scan_kernel    exclusive scan of those counts
//   8 jpeg_enc_write_kernel   header, stuffed stream bytes at their final positions, the 1-bit padding, EOI, the file size
// All of it is integer work on a few bytes per pixel: nothing for the matrix cores, no floating point.
#include "drag_common.h"
#include "jpeg_enc_core.h"

namespace {

constexpr int CHUNK = 64;          // stream bytes per thread in the stuffing kernels

struct JpegEncArgs {
  const uint8_t* img;              // [n, H, W, C]
  JpegEncGeom g;
  long long img_stride;            // bytes per image
  uint8_t* planes; long long planes_stride;
  int16_t* coef; long long coef_stride;          // [n, nblocks * 64]
  uint32_t* bbits; long long bb_stride;          // [n, nblocks]: bits per block, then (after the scan) exclusive offsets
  uint32_t* words; long long words_stride;       // [n, ...] the entropy-coded stream, MSB first in big-endian words, unstuffed
  uint32_t* ffc; long long ffc_stride;           // [n, nchunks_max]: 0xFF bytes per chunk, then exclusive offsets
  unsigned long long* sums;        // [n, 4]: total bits, total 0xFF bytes, unused, unused
  uint8_t* out; long long out_stride;
  long long* sizes;
  int hdr_len;
  uint16_t qt[2][64];              // natural order
  uint8_t hdr[JPEG_ENC_HEADER_MAX];
};

__global__ __launch_bounds__(256) void jpeg_enc_planes_kernel(JpegEncArgs p) {
  const int i = blockIdx.y;
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= p.g.plane_bytes) return;
  const int c = s >= p.g.plane_off[2] && p.g.ncomp == 3 ? 2 : (s >= p.g.plane_off[1] && p.g.ncomp == 3 ? 1 : 0);
  const long long r = s - p.g.plane_off[c];
  const int y = (int)(r / p.g.pw[c]), x = (int)(r - (long long)y * p.g.pw[c]);
  p.planes[(long long)i * p.planes_stride + s] = jpeg_enc_sample(p.img + (long long)i * p.img_stride, p.g, c, x, y);
}

__global__ __launch_bounds__(256) void jpeg_enc_dct_kernel(JpegEncArgs p) {
  const int i = blockIdx.y;
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= p.g.nblocks) return;
  JpegEncBlock k;
  jpeg_enc_block(p.g, b, &k);
  int16_t zz[64];
  jpeg_enc_block_coefs(p.planes + (long long)i * p.planes_stride + p.g.plane_off[k.comp], p.g.pw[k.comp], k.bx, k.by,
                       p.qt[k.comp ? 1 : 0], k.dummy, zz);
  u32x4_t* o = (u32x4_t*)(p.coef + (long long)i * p.coef_stride + b * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    u32x4_t v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (uint32_t)(uint16_t)zz[8 * q + 2 * e] | ((uint32_t)(uint16_t)zz[8 * q + 2 * e + 1] << 16);
    o[q] = v;
  }
}

// both Huffman pairs into LDS, one symbol per thread
__device__ __forceinline__ void load_tables(uint32_t* tab) {
  for (int s = threadIdx.x; s < 2 * JPEG_ENC_TAB; s += blockDim.x) tab[s] = 0;
  __syncthreads();
  for (int s = threadIdx.x; s < 2 * (12 + 162); s += blockDim.x) {
    const int pair = s / (12 + 162), r = s - pair * (12 + 162);
    const int t = 2 * pair + (r >= 12), k = r >= 12 ? r - 12 : r;
    tab[pair * JPEG_ENC_TAB + jpeg_enc_tab_slot(t, k)] = jpeg_enc_huff_code(t, k);
  }
  __syncthreads();
}

// block b's coefficients into registers, its component and the DC it is predicted from
__device__ __forceinline__ void load_block(const JpegEncArgs& p, int i, long long b, int16_t* zz, int& comp, int& last_dc) {
  const int16_t* coef = p.coef + (long long)i * p.coef_stride;
  const u32x4_t* s = (const u32x4_t*)(coef + b * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const u32x4_t v = s[q];
#pragma unroll
    for (int e = 0; e < 4; ++e) { zz[8 * q + 2 * e] = (int16_t)(v[e] & 0xffffu); zz[8 * q + 2 * e + 1] = (int16_t)(v[e] >> 16); }
  }
  JpegEncBlock k;
  jpeg_enc_block(p.g, b, &k);
  comp = k.comp;
  last_dc = k.pred >= 0 ? (int)coef[k.pred * 64] : 0;
}

__global__ __launch_bounds__(256) void jpeg_enc_bits_kernel(JpegEncArgs p) {
  __shared__ uint32_t tab[2 * JPEG_ENC_TAB];
  load_tables(tab);
  const int i = blockIdx.y;
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= p.g.nblocks) return;
  int16_t zz[64];
  int comp, last_dc;
  load_block(p, i, b, zz, comp, last_dc);
  JpegEncCountBits cnt;
  jpeg_enc_block_codes(zz, last_dc, tab + (comp ? JPEG_ENC_TAB : 0), cnt);
  p.bbits[(long long)i * p.bb_stride + b] = cnt.bits;
}

// phase 0: the block lengths (count = nblocks, total -> sums[0]); phase 1: the 0xFF counts (count from sums[0], total -> sums[1])
__global__ __launch_bounds__(1024) void jpeg_enc_scan_kernel(JpegEncArgs p, int phase) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry_s;
  const int i = blockIdx.x, t = threadIdx.x;
  uint32_t* a = phase == 0 ? p.bbits + (long long)i * p.bb_stride : p.ffc + (long long)i * p.ffc_stride;
  const long long count = phase == 0 ? (long long)p.g.nblocks
                                     : (long long)((((p.sums[(long long)i * 4 + 0] + 7) >> 3) + CHUNK - 1) / CHUNK);
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (long long base = 0; base < count; base += 1024) {
    const long long c = base + t;
    const uint32_t v = c < count ? a[c] : 0u;
    uint32_t x = v;                                            // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane_id() >= d) x += y;
    }
    if (lane_id() == 63) wsum[wave_id()] = x;
    __syncthreads();
    uint32_t off = carry_s;
    for (int w = 0; w < wave_id(); ++w) off += wsum[w];
    if (c < count) a[c] = off + x - v;                         // exclusive
    __syncthreads();
    if (t == 1023) carry_s = off + x;
    __syncthreads();
  }
  if (t == 0) p.sums[(long long)i * 4 + phase] = carry_s;
}

struct PackBits {
  uint32_t* words;
  uint32_t w;
  int nb;
  unsigned long long acc;
  bool first;
  __device__ __forceinline__ void operator()(uint32_t bits, int len) {
    acc = (acc << len) | bits;
    nb += len;
    if (nb >= 32) {
      const uint32_t v = (uint32_t)(acc >> (nb - 32));
      // the first word is shared with the previous block's last bits; later whole words belong to this block alone
      if (first) { atomicOr(&words[w], v); first = false; } else words[w] = v;
      ++w; nb -= 32;
    }
  }
};

__global__ __launch_bounds__(256) void jpeg_enc_pack_kernel(JpegEncArgs p) {
  __shared__ uint32_t tab[2 * JPEG_ENC_TAB];
  load_tables(tab);
  const int i = blockIdx.y;
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= p.g.nblocks) return;
  int16_t zz[64];
  int comp, last_dc;
  load_block(p, i, b, zz, comp, last_dc);
  const uint32_t off = p.bbits[(long long)i * p.bb_stride + b];
  PackBits put{p.words + (long long)i * p.words_stride, off >> 5, (int)(off & 31), 0ull, true};
  jpeg_enc_block_codes(zz, last_dc, tab + (comp ? JPEG_ENC_TAB : 0), put);
  if (put.nb > 0) atomicOr(&put.words[put.w], (uint32_t)(put.acc << (32 - put.nb)));
}

// byte q of image i's unstuffed stream of `bits` bits; the last byte is padded with 1-bits
__device__ __forceinline__ uint32_t stream_byte(const uint32_t* words, long long q, unsigned long long bits) {
  uint32_t v = (words[q >> 2] >> (24 - 8 * (int)(q & 3))) & 0xffu;
  const long long tail = 8 * (q + 1) - (long long)bits;
  if (tail > 0) v |= (1u << tail) - 1u;
  return v;
}

__global__ __launch_bounds__(256) void jpeg_enc_ff_kernel(JpegEncArgs p) {
  const int i = blockIdx.y;
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long bits = p.sums[(long long)i * 4 + 0];
  const long long nbytes = (long long)((bits + 7) >> 3);
  const long long q0 = c * CHUNK;
  if (q0 >= nbytes) return;
  const uint32_t* words = p.words + (long long)i * p.words_stride;
  const int m = (int)min((long long)CHUNK, nbytes - q0);
  uint32_t n = 0;
  for (int k = 0; k < m; ++k) n += stream_byte(words, q0 + k, bits) == 0xffu;
  p.ffc[(long long)i * p.ffc_stride + c] = n;
}

__global__ __launch_bounds__(256) void jpeg_enc_write_kernel(JpegEncArgs p) {
  const int i = blockIdx.y;
  uint8_t* out = p.out + (long long)i * p.out_stride;
  if (blockIdx.x == 0)
    for (int k = threadIdx.x; k < p.hdr_len; k += 256) out[k] = p.hdr[k];
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long bits = p.sums[(long long)i * 4 + 0];
  const long long nbytes = (long long)((bits + 7) >> 3);
  const long long q0 = c * CHUNK;
  if (q0 >= nbytes) return;
  const uint32_t* words = p.words + (long long)i * p.words_stride;
  const int m = (int)min((long long)CHUNK, nbytes - q0);
  uint8_t* o = out + p.hdr_len + q0 + p.ffc[(long long)i * p.ffc_stride + c];
  for (int k = 0; k < m; ++k) {
    const uint32_t v = stream_byte(words, q0 + k, bits);
    *o++ = (uint8_t)v;
    if (v == 0xffu) *o++ = 0;
  }
  if (q0 + m == nbytes) {                                      // the last chunk: o is the end of the stuffed stream
    o[0] = 0xFF; o[1] = 0xD9;
    p.sizes[i] = (long long)(o + 2 - out);
  }
}

inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

struct JpegEncPlan {
  JpegEncGeom g;
  long long max_d, nchunks_max;
  long long planes_stride, coef_stride, bb_stride, words_stride, ffc_stride;
  long long off_planes, off_coef, off_bb, off_ffc, off_sums, off_words, total;
  long long out_stride;
};

bool make_plan(int n, int H, int W, int C, int subsampling, JpegEncPlan& q) {
  if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return false;
  if ((long long)H * W > (1ll << 24)) return false;
  if (C == 3 && (subsampling < 0 || subsampling > 2)) return false;
  jpeg_enc_geometry(W, H, C, subsampling, &q.g);
  q.max_d = q.g.nblocks * JPEG_ENC_BLOCK_BYTES;                 // < 2^32 bits: at most ~810 k blocks below 2^24 pixels
  if (q.max_d * 8 >= (1ll << 32)) return false;
  q.nchunks_max = (q.max_d + CHUNK - 1) / CHUNK;
  q.planes_stride = align_up(q.g.plane_bytes, 64);
  q.coef_stride = q.g.nblocks * 64;
  q.bb_stride = align_up(q.g.nblocks, 64);
  q.words_stride = align_up(q.max_d / 4 + 4, 64);
  q.ffc_stride = align_up(q.nchunks_max, 64);
  long long o = 0;
  q.off_planes = o; o = align_up(o + n * q.planes_stride, 256);
  q.off_coef = o; o = align_up(o + n * q.coef_stride * 2, 256);
  q.off_bb = o; o = align_up(o + n * q.bb_stride * 4, 256);
  q.off_ffc = o; o = align_up(o + n * q.ffc_stride * 4, 256);
  q.off_sums = o; o = align_up(o + (long long)n * 4 * 8, 256);
  q.off_words = o; o = align_up(o + n * q.words_stride * 4, 256);
  q.total = o;
  q.out_stride = align_up(JPEG_ENC_HEADER_MAX + 2 * q.max_d + 2, 256);     // every stream byte 0xFF: stuffing doubles it
  return true;
}

#define JPEG_ENC_PLAN_MSG "n, H, W must be positive, H and W at most 65535 with at most 2^24 pixels, channels 1 or 3, subsampling 0, 1 or 2"

}  // namespace

// workspace / output sizing for a batch of n images [H, W, C]: *workspace_bytes for the scratch buffer, *out_stride bytes per
// image in the output buffer (the worst case: JPEG_ENC_BLOCK_BYTES of stream per block, every byte of it stuffed)
extern "C" int drag_jpeg_encode_plan(int32_t n, int32_t H, int32_t W, int32_t C, int32_t subsampling, int64_t* workspace_bytes,
                                     int64_t* out_stride) {
  JpegEncPlan q;
  DRAG_CHECK(make_plan(n, H, W, C, subsampling, q), "drag_jpeg_encode_plan: " JPEG_ENC_PLAN_MSG);
  if (workspace_bytes) *workspace_bytes = q.total;
  if (out_stride) *out_stride = q.out_stride;
  return 0;
}

// images uint8 [n, H, W, C] (C = 3 RGB, 1 grey; dense) -> n JPEG files at out + i * out_stride, their byte counts in sizes[i]
// (device int64).  workspace: drag_jpeg_encode_plan's size, 256-byte aligned.  Everything is enqueued on `stream`.
extern "C" int drag_jpeg_encode(const void* images, int32_t n, int32_t H, int32_t W, int32_t C, int32_t quality, int32_t subsampling,
                                void* workspace, int64_t workspace_bytes, void* out, int64_t out_stride, int64_t* sizes, void* stream) {
  DRAG_CHECK(images && workspace && out && sizes, "drag_jpeg_encode: null pointer");
  DRAG_CHECK(quality >= 1 && quality <= 100, "drag_jpeg_encode: quality must be 1..100");
  JpegEncPlan q;
  DRAG_CHECK(make_plan(n, H, W, C, subsampling, q), "drag_jpeg_encode: " JPEG_ENC_PLAN_MSG);
  DRAG_CHECK(workspace_bytes >= q.total && out_stride >= q.out_stride, "drag_jpeg_encode: workspace or out_stride smaller than drag_jpeg_encode_plan's");
  DRAG_CHECK(((uintptr_t)workspace & 255) == 0, "drag_jpeg_encode: workspace must be 256-byte aligned");
  char* ws = (char*)workspace;
  JpegEncArgs p;
  p.img = (const uint8_t*)images; p.g = q.g; p.img_stride = (long long)H * W * C;
  p.planes = (uint8_t*)(ws + q.off_planes); p.planes_stride = q.planes_stride;
  p.coef = (int16_t*)(ws + q.off_coef); p.coef_stride = q.coef_stride;
  p.bbits = (uint32_t*)(ws + q.off_bb); p.bb_stride = q.bb_stride;
  p.ffc = (uint32_t*)(ws + q.off_ffc); p.ffc_stride = q.ffc_stride;
  p.sums = (unsigned long long*)(ws + q.off_sums);
  p.words = (uint32_t*)(ws + q.off_words); p.words_stride = q.words_stride;
  p.out = (uint8_t*)out; p.out_stride = out_stride; p.sizes = (long long*)sizes;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) p.qt[t][k] = (uint16_t)jpeg_enc_quant(t, quality, k);
  p.hdr_len = jpeg_enc_header(q.g, quality, p.hdr);
  const hipStream_t st = (hipStream_t)stream;
  // zero: the sums and the bit stream (OR-ed into); contiguous regions
  DRAG_CHECK(hipMemsetAsync(ws + q.off_sums, 0, (size_t)(q.total - q.off_sums), st) == hipSuccess, "drag_jpeg_encode: memset failed");
  const dim3 gsamples((unsigned)((q.g.plane_bytes + 255) / 256), (unsigned)n);
  const dim3 gblocks((unsigned)((q.g.nblocks + 255) / 256), (unsigned)n);
  const dim3 gchunks((unsigned)((q.nchunks_max + 255) / 256), (unsigned)n);
  hipLaunchKernelGGL(jpeg_enc_planes_kernel, gsamples, dim3(256), 0, st, p);
  hipLaunchKernelGGL(jpeg_enc_dct_kernel, gblocks, dim3(256), 0, st, p);
  hipLaunchKernelGGL(jpeg_enc_bits_kernel, gblocks, dim3(256), 0, st, p);
  hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3((unsigned)n), dim3(1024), 0, st, p, 0);
  hipLaunchKernelGGL(jpeg_enc_pack_kernel, gblocks, dim3(256), 0, st, p);
  hipLaunchKernelGGL(jpeg_enc_ff_kernel, gchunks, dim3(256), 0, st, p);
  hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3((unsigned)n), dim3(1024), 0, st, p, 1);
  hipLaunchKernelGGL(jpeg_enc_write_kernel, gchunks, dim3(256), 0, st, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}
