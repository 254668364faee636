// jpeg_internal.h — what csrc/jpeg.hip and csrc/jpeg_par.hip share: the kernels' argument block and the tail of a decode (lane
// entropy kernels, IDCT, colour).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "jpeg_core.h"

struct JpegArgs {
  const uint8_t* data;
  const int64_t* off;       // [n + 1] byte offsets of the files inside `data`
  const JpegInfo* info;     // [n]
  const int64_t* plan;      // [n, 3]: coefficient offset (int16 elements), plane offset (bytes), output offset (bytes)
  int16_t* coef;
  uint8_t* planes;
  uint16_t* qtab;           // [n, 3, 64] quantisation tables in natural order
  uint8_t* out;
  int32_t* scan_status;     // [n]: 0 = the entropy-coded data ended at the EOI marker, as a clean file's does
  const int32_t* mask;      // [n] or null: jpeg_huffman_kernel decodes file i only if mask[i] != 0 (null: every file)
  int n;
};

// jpeg_huffman_kernel (over the files the mask names), jpeg_progressive_kernel, jpeg_idct_kernel, jpeg_color_kernel on `st`; the
// coefficient buffer is zero wherever the lane kernels are going to decode.  0, or an error code with drag_last_error() set.
int jpeg_lane_and_pixels(const JpegArgs& a, int64_t max_blocks, int64_t max_pixels, hipStream_t st);
