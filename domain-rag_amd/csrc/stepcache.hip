// stepcache.hip — the kernels of the first-block step cache of the Flux DiT (flux.StepCache; opt-in, the default forward calls none of them).
//
// All address image rows as drag_layernorm_modulate_bf16 does: `rows_per_batch` rows of `cols` bf16 elements, row stride `cols`, batch
// stride `x_batch_stride` — an image's rows are one contiguous run of rows_per_batch * cols elements inside the joint [B, S, D] buffer,
// behind its text rows.  The dense operands (e, f, r, p) are [B, rows_per_batch, cols].
//
// Memory-bound streaming kernels: 16-byte loads and stores (8 bf16 per lane), a grid capped at 2048 workgroups of 256 threads with the rest
// grid-strided.  The residual ratio is summed in float64 from the first term on (bf16 -> float64 is exact, so only the order of summation
// separates the result from a float64 reference), per workgroup into `workspace`, then combined by a second launch in a fixed order: no
// floating-point atomics, the same input gives the same 64 bits on every run.
//
// The *_images / swap forms (StepCache scope "image": every image decides for itself) work on a LIST of images or of image pairs.  The list
// is a host array: the entry point validates it (range, order, disjointness) and copies it into the kernel's argument struct, so no index
// a kernel reads can lie outside [0, B).  blockIdx.y walks the list; the element loop is the whole-batch kernels'.
#include "drag_common.h"

#include <math.h>

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_GRID = 2048;

// workgroups per image: every image gets the same count, the whole grid stays at or under SC_MAX_GRID (one per image at least)
inline int sc_blocks_per_image(int B, long long n8) {
  long long g = (n8 + SC_THREADS - 1) / SC_THREADS;
  const long long cap = SC_MAX_GRID / B > 0 ? SC_MAX_GRID / B : 1;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// e <- bf16(f32(x) - f32(e)); with RATIO also this workgroup's sums of |e - f| and |f| over the stored e -> part[(b * gridDim.x + block) * 2]
template <bool RATIO>
__global__ __launch_bounds__(SC_THREADS) void stepcache_delta_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ e,
                                                                     const bf16_t* __restrict__ f, double* __restrict__ part,
                                                                     long long n8, long long x_bs) {
  const int b = blockIdx.y;
  const bf16_t* xb = x + (long long)b * x_bs;
  bf16_t* eb = e + (long long)b * n8 * 8;
  const bf16_t* fb = RATIO ? f + (long long)b * n8 * 8 : nullptr;
  double num = 0.0, den = 0.0;
  const long long stride = (long long)gridDim.x * SC_THREADS;
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < n8; i += stride) {
    const u32x4_t xr = *(const u32x4_t*)(xb + i * 8);
    const u32x4_t er = *(const u32x4_t*)(eb + i * 8);
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = pack2bf(bf2f((bf16_t)(xr[j] & 0xffff)) - bf2f((bf16_t)(er[j] & 0xffff)),
                     bf2f((bf16_t)(xr[j] >> 16)) - bf2f((bf16_t)(er[j] >> 16)));
    *(u32x4_t*)(eb + i * 8) = o;
    if (RATIO) {
      const u32x4_t fr = *(const u32x4_t*)(fb + i * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double e0 = (double)bf2f((bf16_t)(o[j] & 0xffff)), e1 = (double)bf2f((bf16_t)(o[j] >> 16));
        const double f0 = (double)bf2f((bf16_t)(fr[j] & 0xffff)), f1 = (double)bf2f((bf16_t)(fr[j] >> 16));
        num += fabs(e0 - f0);
        num += fabs(e1 - f1);
        den += fabs(f0);
        den += fabs(f1);
      }
    }
  }
  if (RATIO) {
    __shared__ double red[2][SC_THREADS / 64];
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    if (lane_id() == 0) {
      red[0][wave_id()] = num;
      red[1][wave_id()] = den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double n = red[0][0], d = red[1][0];
#pragma unroll
      for (int w = 1; w < SC_THREADS / 64; ++w) {
        n += red[0][w];
        d += red[1][w];
      }
      double* dst = part + ((long long)b * gridDim.x + blockIdx.x) * 2;
      dst[0] = n;
      dst[1] = d;
    }
  }
}

// one wave per image: lane l adds partials l, l + 64, ... in ascending order, then the fixed butterfly
__global__ __launch_bounds__(64) void stepcache_ratio_kernel(const double* __restrict__ part, double* __restrict__ ratios, int per_image) {
  const int b = blockIdx.x;
  const double* p = part + (long long)b * per_image * 2;
  double num = 0.0, den = 0.0;
  for (int i = threadIdx.x; i < per_image; i += 64) {
    num += p[2 * i];
    den += p[2 * i + 1];
  }
  num = wave_sum_f64(num);
  den = wave_sum_f64(den);
  if (threadIdx.x == 0) {
    double r;
    if (num != num || den != den) r = num + den;      // NaN propagates
    else if (den == 0.0) r = (double)INFINITY;        // nothing to compare against: never "close"
    else r = num / den;
    ratios[b] = r;
  }
}

// one image: ADD: x <- bf16(f32(x) + f32(r)); else the capture form r <- bf16(f32(x) - f32(r))
template <bool ADD>
__device__ __forceinline__ void sc_apply_image(bf16_t* __restrict__ xb, bf16_t* __restrict__ rb, long long n8) {
  const long long stride = (long long)gridDim.x * SC_THREADS;
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < n8; i += stride) {
    const u32x4_t xr = *(const u32x4_t*)(xb + i * 8);
    const u32x4_t rr = *(const u32x4_t*)(rb + i * 8);
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x0 = bf2f((bf16_t)(xr[j] & 0xffff)), x1 = bf2f((bf16_t)(xr[j] >> 16));
      const float r0 = bf2f((bf16_t)(rr[j] & 0xffff)), r1 = bf2f((bf16_t)(rr[j] >> 16));
      o[j] = ADD ? pack2bf(x0 + r0, x1 + r1) : pack2bf(x0 - r0, x1 - r1);
    }
    *(u32x4_t*)((ADD ? xb : rb) + i * 8) = o;
  }
}

// ADD: x <- bf16(f32(x) + f32(r)) (x strided, r dense); else the capture form r <- bf16(f32(x) - f32(r))
template <bool ADD>
__global__ __launch_bounds__(SC_THREADS) void stepcache_apply_kernel(bf16_t* __restrict__ x, bf16_t* __restrict__ r, long long n8,
                                                                     long long x_bs) {
  const int b = blockIdx.y;
  sc_apply_image<ADD>(x + (long long)b * x_bs, r + (long long)b * n8 * 8, n8);
}

// ---- list forms.  SC_MAX_LIST indices travel in the argument struct (256 bytes), validated on the host
constexpr int SC_MAX_LIST = 64;
struct ScList {
  int32_t v[SC_MAX_LIST];
};

// the apply kernel on the listed images only; r stays indexed by image
template <bool ADD>
__global__ __launch_bounds__(SC_THREADS) void stepcache_apply_images_kernel(bf16_t* __restrict__ x, bf16_t* __restrict__ r, long long n8,
                                                                            long long x_bs, ScList images) {
  const int b = images.v[blockIdx.y];
  sc_apply_image<ADD>(x + (long long)b * x_bs, r + (long long)b * n8 * 8, n8);
}

// the coefficients of a forecast's listed images, next to their indices in the argument struct (validated on the host: all finite)
struct ScCoef {
  float v[SC_MAX_LIST];
};

// one element of the first-order forecast: x + (c * (r - p) + r), four individually rounded float32 operations.  Contraction is off for
// the block: c * d + r must not become an FMA (the reference arithmetic is numpy float32, which cannot fuse)
__device__ __forceinline__ float sc_forecast(float x, float r, float p, float c) {
#pragma clang fp contract(off)
  const float d = r - p;
  const float m = c * d;
  const float f = m + r;
  return x + f;
}

// x[b] <- bf16(f32(x) + (c * (f32(r) - f32(p)) + f32(r))) for the listed images b = images.v[i], c = coef.v[i]; r and p stay indexed by image
__global__ __launch_bounds__(SC_THREADS) void stepcache_forecast_images_kernel(bf16_t* __restrict__ x, const bf16_t* __restrict__ r,
                                                                              const bf16_t* __restrict__ p, long long n8, long long x_bs,
                                                                              ScList images, ScCoef coef) {
  const int b = images.v[blockIdx.y];
  const float c = coef.v[blockIdx.y];
  bf16_t* xb = x + (long long)b * x_bs;
  const bf16_t* rb = r + (long long)b * n8 * 8;
  const bf16_t* pb = p + (long long)b * n8 * 8;
  const long long stride = (long long)gridDim.x * SC_THREADS;
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < n8; i += stride) {
    const u32x4_t xr = *(const u32x4_t*)(xb + i * 8);
    const u32x4_t rr = *(const u32x4_t*)(rb + i * 8);
    const u32x4_t pr = *(const u32x4_t*)(pb + i * 8);
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = pack2bf(sc_forecast(bf2f((bf16_t)(xr[j] & 0xffff)), bf2f((bf16_t)(rr[j] & 0xffff)), bf2f((bf16_t)(pr[j] & 0xffff)), c),
                     sc_forecast(bf2f((bf16_t)(xr[j] >> 16)), bf2f((bf16_t)(rr[j] >> 16)), bf2f((bf16_t)(pr[j] >> 16)), c));
    *(u32x4_t*)(xb + i * 8) = o;
  }
}

// dst[b] <- src[b] for the listed images (dst dense, src with its own batch stride)
__global__ __launch_bounds__(SC_THREADS) void stepcache_copy_images_kernel(bf16_t* __restrict__ dst, const bf16_t* __restrict__ src,
                                                                           long long n8, long long src_bs, ScList images) {
  const int b = images.v[blockIdx.y];
  bf16_t* db = dst + (long long)b * n8 * 8;
  const bf16_t* sb = src + (long long)b * src_bs;
  const long long stride = (long long)gridDim.x * SC_THREADS;
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < n8; i += stride)
    *(u32x4_t*)(db + i * 8) = *(const u32x4_t*)(sb + i * 8);
}

// exchange the rows of image pairs.v[2p] with those of image pairs.v[2p + 1], p = blockIdx.y: each lane owns its 16 bytes of both images
__global__ __launch_bounds__(SC_THREADS) void stepcache_swap_kernel(bf16_t* __restrict__ x, long long n8, long long x_bs, ScList pairs) {
  bf16_t* a = x + (long long)pairs.v[2 * blockIdx.y] * x_bs;
  bf16_t* b = x + (long long)pairs.v[2 * blockIdx.y + 1] * x_bs;
  const long long stride = (long long)gridDim.x * SC_THREADS;
  for (long long i = (long long)blockIdx.x * SC_THREADS + threadIdx.x; i < n8; i += stride) {
    const u32x4_t av = *(const u32x4_t*)(a + i * 8);
    const u32x4_t bv = *(const u32x4_t*)(b + i * 8);
    *(u32x4_t*)(a + i * 8) = bv;
    *(u32x4_t*)(b + i * 8) = av;
  }
}

inline bool sc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// a host list of image indices into `out`: at most SC_MAX_LIST entries, each in [0, B); `increasing`: strictly increasing (an image list),
// else all distinct (the 2 * n_pairs indices of a pair list)
inline bool sc_take_list(const int32_t* host, int n, int B, bool increasing, ScList* out) {
  if (!host || n < 0 || n > SC_MAX_LIST) return false;
  for (int i = 0; i < SC_MAX_LIST; ++i) out->v[i] = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t v = host[i];
    if (v < 0 || v >= B) return false;
    if (increasing && i > 0 && v <= host[i - 1]) return false;
    if (!increasing)
      for (int j = 0; j < i; ++j)
        if (host[j] == v) return false;
    out->v[i] = v;
  }
  return true;
}

}  // namespace

extern "C" int64_t drag_stepcache_workspace_bytes(int32_t B, int32_t rows_per_batch, int32_t cols) {
  if (B <= 0 || rows_per_batch <= 0 || cols <= 0) return 0;
  return (int64_t)B * sc_blocks_per_image(B, (long long)rows_per_batch * cols / 8) * 2 * (int64_t)sizeof(double);
}

extern "C" int drag_stepcache_delta_bf16(const void* x, void* e, const void* f, double* ratios, void* workspace, int32_t B,
                                         int32_t rows_per_batch, int32_t cols, int64_t x_batch_stride, void* stream) {
  DRAG_CHECK(x && e, "drag_stepcache_delta_bf16: null pointer");
  DRAG_CHECK(!f || (ratios && workspace), "drag_stepcache_delta_bf16: null pointer (f given: ratios and workspace are required)");
  DRAG_CHECK(B > 0 && B <= 65535 && rows_per_batch > 0 && cols > 0 && cols % 8 == 0,
             "drag_stepcache_delta_bf16: bad shape (B in 1..65535, rows_per_batch > 0, cols > 0, cols %% 8 == 0)");
  const long long n = (long long)rows_per_batch * cols;
  DRAG_CHECK(x_batch_stride >= n, "drag_stepcache_delta_bf16: x_batch_stride < rows_per_batch * cols");
  DRAG_CHECK(x_batch_stride % 8 == 0 && sc_aligned16(x) && sc_aligned16(e) && sc_aligned16(f) && ((uintptr_t)ratios & 7) == 0 &&
                 ((uintptr_t)workspace & 7) == 0,
             "drag_stepcache_delta_bf16: x, e, f must be 16-byte aligned (x_batch_stride %% 8 == 0), ratios and workspace 8-byte");
  const int gpi = sc_blocks_per_image(B, n / 8);
  if (f) {
    hipLaunchKernelGGL(stepcache_delta_kernel<true>, dim3(gpi, B), dim3(SC_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)e,
                       (const bf16_t*)f, (double*)workspace, n / 8, (long long)x_batch_stride);
    DRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(stepcache_ratio_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, ratios, gpi);
  } else {
    hipLaunchKernelGGL(stepcache_delta_kernel<false>, dim3(gpi, B), dim3(SC_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)e,
                       (const bf16_t*)nullptr, (double*)nullptr, n / 8, (long long)x_batch_stride);
  }
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_stepcache_apply_bf16(void* x, void* r, int32_t B, int32_t rows_per_batch, int32_t cols, int64_t x_batch_stride,
                                         int32_t sign, void* stream) {
  DRAG_CHECK(x && r, "drag_stepcache_apply_bf16: null pointer");
  DRAG_CHECK(B > 0 && B <= 65535 && rows_per_batch > 0 && cols > 0 && cols % 8 == 0,
             "drag_stepcache_apply_bf16: bad shape (B in 1..65535, rows_per_batch > 0, cols > 0, cols %% 8 == 0)");
  DRAG_CHECK(sign == 1 || sign == -1, "drag_stepcache_apply_bf16: sign must be +1 (x += r) or -1 (r = x - r)");
  const long long n = (long long)rows_per_batch * cols;
  DRAG_CHECK(x_batch_stride >= n, "drag_stepcache_apply_bf16: x_batch_stride < rows_per_batch * cols");
  DRAG_CHECK(x_batch_stride % 8 == 0 && sc_aligned16(x) && sc_aligned16(r),
             "drag_stepcache_apply_bf16: x and r must be 16-byte aligned (x_batch_stride %% 8 == 0)");
  const int gpi = sc_blocks_per_image(B, n / 8);
  if (sign > 0)
    hipLaunchKernelGGL(stepcache_apply_kernel<true>, dim3(gpi, B), dim3(SC_THREADS), 0, (hipStream_t)stream, (bf16_t*)x, (bf16_t*)r, n / 8,
                       (long long)x_batch_stride);
  else
    hipLaunchKernelGGL(stepcache_apply_kernel<false>, dim3(gpi, B), dim3(SC_THREADS), 0, (hipStream_t)stream, (bf16_t*)x, (bf16_t*)r, n / 8,
                       (long long)x_batch_stride);
  DRAG_LAUNCH_CHECK();
  return 0;
}

// ---- scope "image": the list forms

#define SC_COMMON_CHECKS(name, p0, p1, bs)                                                                                                    \
  DRAG_CHECK((p0) && (p1), name ": null pointer");                                                                                             \
  DRAG_CHECK(B > 0 && B <= 65535 && rows_per_batch > 0 && cols > 0 && cols % 8 == 0,                                                           \
             name ": bad shape (B in 1..65535, rows_per_batch > 0, cols > 0, cols %% 8 == 0)");                                                \
  const long long n = (long long)rows_per_batch * cols;                                                                                        \
  DRAG_CHECK((bs) >= n, name ": batch stride < rows_per_batch * cols");                                                                        \
  DRAG_CHECK((bs) % 8 == 0 && sc_aligned16(p0) && sc_aligned16(p1), name ": pointers must be 16-byte aligned (batch stride %% 8 == 0)")

extern "C" int drag_stepcache_swap_bf16(void* x, int32_t B, int32_t rows_per_batch, int32_t cols, int64_t x_batch_stride,
                                        const int32_t* pairs, int32_t n_pairs, void* stream) {
  SC_COMMON_CHECKS("drag_stepcache_swap_bf16", x, x, x_batch_stride);
  DRAG_CHECK(n_pairs >= 0 && n_pairs <= SC_MAX_LIST / 2, "drag_stepcache_swap_bf16: n_pairs must be in 0..32 (64 indices)");
  if (n_pairs == 0) return 0;
  ScList list;
  DRAG_CHECK(sc_take_list(pairs, 2 * n_pairs, B, false, &list),
             "drag_stepcache_swap_bf16: pairs must be a host array of distinct image indices in [0, B)");
  hipLaunchKernelGGL(stepcache_swap_kernel, dim3(sc_blocks_per_image(n_pairs, n / 8), n_pairs), dim3(SC_THREADS), 0, (hipStream_t)stream,
                     (bf16_t*)x, n / 8, (long long)x_batch_stride, list);
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_stepcache_apply_images_bf16(void* x, void* r, int32_t B, int32_t rows_per_batch, int32_t cols, int64_t x_batch_stride,
                                                int32_t sign, const int32_t* images, int32_t n_images, void* stream) {
  SC_COMMON_CHECKS("drag_stepcache_apply_images_bf16", x, r, x_batch_stride);
  DRAG_CHECK(sign == 1 || sign == -1, "drag_stepcache_apply_images_bf16: sign must be +1 (x += r) or -1 (r = x - r)");
  DRAG_CHECK(n_images >= 0 && n_images <= SC_MAX_LIST, "drag_stepcache_apply_images_bf16: n_images must be in 0..64");
  if (n_images == 0) return 0;
  ScList list;
  DRAG_CHECK(sc_take_list(images, n_images, B, true, &list),
             "drag_stepcache_apply_images_bf16: images must be a host array of strictly increasing indices in [0, B)");
  const dim3 grid(sc_blocks_per_image(n_images, n / 8), n_images);
  if (sign > 0)
    hipLaunchKernelGGL(stepcache_apply_images_kernel<true>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, (bf16_t*)x, (bf16_t*)r, n / 8,
                       (long long)x_batch_stride, list);
  else
    hipLaunchKernelGGL(stepcache_apply_images_kernel<false>, grid, dim3(SC_THREADS), 0, (hipStream_t)stream, (bf16_t*)x, (bf16_t*)r, n / 8,
                       (long long)x_batch_stride, list);
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_stepcache_copy_images_bf16(void* dst_dense, const void* src, int64_t src_batch_stride, int32_t B, int32_t rows_per_batch,
                                               int32_t cols, const int32_t* images, int32_t n_images, void* stream) {
  SC_COMMON_CHECKS("drag_stepcache_copy_images_bf16", dst_dense, src, src_batch_stride);
  DRAG_CHECK(n_images >= 0 && n_images <= SC_MAX_LIST, "drag_stepcache_copy_images_bf16: n_images must be in 0..64");
  if (n_images == 0) return 0;
  ScList list;
  DRAG_CHECK(sc_take_list(images, n_images, B, true, &list),
             "drag_stepcache_copy_images_bf16: images must be a host array of strictly increasing indices in [0, B)");
  hipLaunchKernelGGL(stepcache_copy_images_kernel, dim3(sc_blocks_per_image(n_images, n / 8), n_images), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (bf16_t*)dst_dense, (const bf16_t*)src, n / 8, (long long)src_batch_stride, list);
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_stepcache_forecast_images_bf16(void* x, const void* r, const void* p, int32_t B, int32_t rows_per_batch, int32_t cols,
                                                   int64_t x_batch_stride, const int32_t* images, const float* coef, int32_t n_images,
                                                   void* stream) {
  SC_COMMON_CHECKS("drag_stepcache_forecast_images_bf16", x, r, x_batch_stride);
  DRAG_CHECK(p && sc_aligned16(p), "drag_stepcache_forecast_images_bf16: p must be a 16-byte aligned pointer");
  DRAG_CHECK(n_images >= 0 && n_images <= SC_MAX_LIST, "drag_stepcache_forecast_images_bf16: n_images must be in 0..64");
  if (n_images == 0) return 0;
  ScList list;
  DRAG_CHECK(sc_take_list(images, n_images, B, true, &list),
             "drag_stepcache_forecast_images_bf16: images must be a host array of strictly increasing indices in [0, B)");
  DRAG_CHECK(coef, "drag_stepcache_forecast_images_bf16: coef must be a host array of n_images floats");
  ScCoef cf;
  for (int i = 0; i < SC_MAX_LIST; ++i) cf.v[i] = 0.0f;
  for (int i = 0; i < n_images; ++i) {
    DRAG_CHECK(isfinite(coef[i]), "drag_stepcache_forecast_images_bf16: every coefficient must be finite");
    cf.v[i] = coef[i];
  }
  hipLaunchKernelGGL(stepcache_forecast_images_kernel, dim3(sc_blocks_per_image(n_images, n / 8), n_images), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (bf16_t*)x, (const bf16_t*)r, (const bf16_t*)p, n / 8, (long long)x_batch_stride, list, cf);
  DRAG_LAUNCH_CHECK();
  return 0;
}
