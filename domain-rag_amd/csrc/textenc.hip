// textenc.hip — the prompt encoders' own kernels (T5-XXL encoder, CLIP-L text tower): attention over head_dim 64 with an optional
// Toeplitz relative-position bias and an optional causal mask, T5's RMSNorm, T5's gated NewGELU, and the token-embedding gather.
// Every Linear of both encoders is drag_gemm_bf16.  Each kernel rounds where upstream's bf16 eager graph rounds (transformers
// modeling_t5.py / modeling_clip.py), op for op, so the HIP encoders follow the reference's bf16 text encoders, not an idealised form.
#include "drag_common.h"
#include <math.h>

namespace {

struct TxtAttnArgs {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  const bf16_t* rel;      // [H, 2S-1] or null: bias(h, qi, ki) = rel[h][ki - qi + S - 1]
  int S, H, ld;           // q / k / v rows of ld elements, head h at column h * 64
  long long bs;           // batch stride of q / k / v (elements)
  int ldo;
  long long obs;
  float scale;
  int causal;
};

// One wave = 16 queries of one (batch, head); 4 independent waves per workgroup, no LDS.  Scores are computed transposed,
// S^T = K Q^T (16 keys x 16 queries per v_mfma_f32_16x16x32_bf16, two k-steps over head_dim 64): lane (c = l & 15, g = l >> 4) holds
// query c and keys 4g..4g+3 of each 16-key tile, which is already the A-operand layout P[query][key] of the P.V product (keys in the
// permuted order 4g+r | 16+4g+r of a 32-key step; V's operand is gathered in that same order).
//   EAGER (T5): s = bf16(q.k) [* scale, bf16] [+ bias, bf16]; p = bf16(exp(s - max) / sum) in fp32; out = bf16(P.V).  Two passes:
//               row max and row sum first (online), then normalised P.V.
//   !EAGER (CLIP, SDPA): s = (q.k) * scale [+ bias] in fp32; p = bf16(exp(s - max)); out = bf16(P.V / sum).
template <bool EAGER>
__global__ __launch_bounds__(256) void textenc_attention_kernel(TxtAttnArgs p) {
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int q0 = blockIdx.x * 64 + wave * 16;
  if (q0 >= p.S) return;
  const int h = blockIdx.y, b = blockIdx.z;
  const int c = l & 15, g = l >> 4;
  const int S = p.S;
  const bf16_t* qb = p.q + (long long)b * p.bs + h * 64;
  const bf16_t* kb = p.k + (long long)b * p.bs + h * 64;
  const bf16_t* vb = p.v + (long long)b * p.bs + h * 64;
  const bf16_t* rel = p.rel ? p.rel + (long long)h * (2 * S - 1) : nullptr;
  const int query = q0 + c;                 // this lane's query (>= S: a padding lane, computed on row S-1's data, never stored)
  const int qc = min(query, S - 1);
  bf16x8_t qf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) qf[s] = *(const bf16x8_t*)(qb + (long long)qc * p.ld + 32 * s + 8 * g);

  auto scores = [&](int k0, float* sc) {
    const int krow = min(k0 + c, S - 1);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8_t kf = *(const bf16x8_t*)(kb + (long long)krow * p.ld + 32 * s + 8 * g);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = k0 + 4 * g + r;
      float x;
      if (key >= S || (p.causal && key > query)) {
        x = -INFINITY;
      } else if (EAGER) {
        x = rbf(acc[r]);
        if (p.scale != 1.0f) x = rbf(x * p.scale);
        if (rel) x = rbf(x + bf2f(rel[key - qc + S - 1]));
      } else {
        x = acc[r] * p.scale;
        if (rel) x += bf2f(rel[key - qc + S - 1]);
      }
      sc[r] = x;
    }
  };

  const int kend = p.causal ? min(S, q0 + 16) : S;
  // pass 1: row max and row sum (this lane's keys, then the four lanes of a query combined)
  float m = -INFINITY, lsum = 0.f;
  for (int k0 = 0; k0 < kend; k0 += 16) {
    float sc[4];
    scores(k0, sc);
    const float mn = fmaxf(m, fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])));
    if (mn == -INFINITY) continue;
    lsum = lsum * expf(m - mn) + (expf(sc[0] - mn) + expf(sc[1] - mn) + expf(sc[2] - mn) + expf(sc[3] - mn));
    m = mn;
  }
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(lsum, off, 64);
    const float mn = fmaxf(m, mo);
    lsum = (m == -INFINITY ? 0.f : lsum * expf(m - mn)) + (mo == -INFINITY ? 0.f : lo * expf(mo - mn));
    m = mn;
  }
  // pass 2: P.V over 32-key steps
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kend; k0 += 32) {
    float s0[4], s1[4];
    scores(k0, s0);
    scores(k0 + 16, s1);
    bf16x8_t pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf[r] = (__bf16)(EAGER ? expf(s0[r] - m) / lsum : expf(s0[r] - m));
      pf[4 + r] = (__bf16)(EAGER ? expf(s1[r] - m) / lsum : expf(s1[r] - m));
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x8_t vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0 + (j < 4 ? 4 * g + j : 16 + 4 * g + j - 4);
        vf[j] = __builtin_bit_cast(__bf16, vb[(long long)min(key, S - 1) * p.ld + dt * 16 + c]);
      }
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, o[dt], 0, 0, 0);
    }
  }
  // o[dt][r] = out[query q0 + 4g + r][dim dt * 16 + c]
  bf16_t* ob = p.o + (long long)b * p.obs + h * 64;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float lq = __shfl(lsum, 4 * g + r, 64);
    const int qi = q0 + 4 * g + r;
    if (qi >= S) continue;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ob[(long long)qi * p.ldo + dt * 16 + c] = f2bf(EAGER ? o[dt][r] : o[dt][r] / lq);
  }
}

// T5LayerNorm: var = mean(x^2) in fp32; y = bf16(x * rsqrt(var + eps)); out = bf16(w * y).  One wave per row, D <= 4096.
constexpr int RMS_IT = 8;
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const bf16_t* x, const bf16_t* w, bf16_t* y, int M, int D, float eps) {
  const int l = lane_id();
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const bf16_t* xr = x + (long long)row * D;
  u32x4_t raw[RMS_IT];
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < RMS_IT; ++it) {
    const int c = (it * 64 + l) * 8;
    raw[it] = (u32x4_t){0u, 0u, 0u, 0u};
    if (c < D) raw[it] = *(const u32x4_t*)(xr + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = bf2f((bf16_t)(raw[it][j] & 0xffff)), bb = bf2f((bf16_t)(raw[it][j] >> 16));
      ss += a * a + bb * bb;
    }
  }
  const float r = 1.0f / sqrtf(wave_sum(ss) / (float)D + eps);
  bf16_t* yr = y + (long long)row * D;
#pragma unroll
  for (int it = 0; it < RMS_IT; ++it) {
    const int c = (it * 64 + l) * 8;
    if (c >= D) continue;
    const u32x4_t wv = *(const u32x4_t*)(w + c);
    u32x4_t pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float n0 = rbf(bf2f((bf16_t)(raw[it][j] & 0xffff)) * r), n1 = rbf(bf2f((bf16_t)(raw[it][j] >> 16)) * r);
      pk[j] = pack2bf(bf2f((bf16_t)(wv[j] & 0xffff)) * n0, bf2f((bf16_t)(wv[j] >> 16)) * n1);
    }
    *(u32x4_t*)(yr + c) = pk;
  }
}

// NewGELU (transformers.activations.NewGELUActivation) as torch evaluates it on bf16 tensors: every op is a bf16 tensor op, and
// pow(x, 3.0) is  base * base * base  in bf16 arithmetic (two roundings).
__device__ __forceinline__ float new_gelu_bf16_chain(float x) {
  const float x3 = rbf(rbf(x * x) * x);
  const float a = rbf(0.044715f * x3);
  const float s = rbf(x + a);
  const float t = rbf(0.7978845608028654f * s);
  const float th = rbf(tanhf(t));
  const float one = rbf(1.0f + th);
  const float hx = rbf(0.5f * x);
  return rbf(hx * one);
}

// y[m, f] = bf16(NewGELU(h[m, f]) * h[m, F + f]) : the fused wi_0 | wi_1 projection's [M, 2F] rows -> [M, F]
__global__ __launch_bounds__(256) void gated_new_gelu_kernel(const bf16_t* hbuf, bf16_t* y, long long n8, int F8) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const long long row = i / F8;
    const int c8 = (int)(i - row * F8);
    const bf16_t* h0 = hbuf + row * (16LL * F8) + c8 * 8;
    const u32x4_t a = *(const u32x4_t*)h0, bl = *(const u32x4_t*)(h0 + 8LL * F8);
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float g0 = new_gelu_bf16_chain(bf2f((bf16_t)(a[j] & 0xffff))), g1 = new_gelu_bf16_chain(bf2f((bf16_t)(a[j] >> 16)));
      o[j] = pack2bf(g0 * bf2f((bf16_t)(bl[j] & 0xffff)), g1 * bf2f((bf16_t)(bl[j] >> 16)));
    }
    *(u32x4_t*)(y + row * (8LL * F8) + c8 * 8) = o;
  }
}

// QuickGELU as CLIP's eager graph evaluates it on bf16 tensors: x * sigmoid(1.702 x), each of the three ops rounded to bf16 (the GEMM
// epilogue's fused form rounds once and parts from upstream's bf16 tower by as much as upstream parts from fp32)
__global__ __launch_bounds__(256) void quick_gelu_kernel(const bf16_t* x, bf16_t* y, long long n8) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const u32x4_t a = *(const u32x4_t*)(x + i * 8);
    u32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[2] = {bf2f((bf16_t)(a[j] & 0xffff)), bf2f((bf16_t)(a[j] >> 16))};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float z = rbf(1.702f * v[t]);
        v[t] = v[t] * rbf(1.0f / (1.0f + expf(-z)));
      }
      o[j] = pack2bf(v[0], v[1]);
    }
    *(u32x4_t*)(y + i * 8) = o;
  }
}

// out[r] = table[ids[r]] (+ pos[r % S], one bf16 add); an id outside [0, vocab) gives a zero row (the host validates ids first)
__global__ __launch_bounds__(256) void embed_gather_kernel(const int64_t* ids, const bf16_t* table, const bf16_t* pos, bf16_t* out,
                                                           long long rows, int S, int D8, long long vocab) {
  const long long n8 = rows * D8;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const long long r = i / D8;
    const int c8 = (int)(i - r * D8);
    const long long id = ids[r];
    u32x4_t t = {0u, 0u, 0u, 0u};
    if (id >= 0 && id < vocab) t = *(const u32x4_t*)(table + id * (8LL * D8) + c8 * 8);
    if (pos) {
      const u32x4_t pv = *(const u32x4_t*)(pos + (long long)(r % S) * (8LL * D8) + c8 * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        t[j] = pack2bf(bf2f((bf16_t)(t[j] & 0xffff)) + bf2f((bf16_t)(pv[j] & 0xffff)),
                       bf2f((bf16_t)(t[j] >> 16)) + bf2f((bf16_t)(pv[j] >> 16)));
    }
    *(u32x4_t*)(out + r * (8LL * D8) + c8 * 8) = t;
  }
}

int ew_blocks(long long n) { return (int)min((n + 255) / 256, 8192LL); }

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

}  // namespace

extern "C" int drag_textenc_attention_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t S, int32_t H,
                                           int32_t ld, int64_t batch_stride, int32_t ld_o, int64_t o_batch_stride, float scale,
                                           const void* rel_bias, int32_t causal, int32_t eager, void* stream) {
  DRAG_CHECK(q && k && v && out, "drag_textenc_attention_bf16: null pointer");
  DRAG_CHECK(B >= 1 && H >= 1 && B <= 65535 && H <= 65535, "drag_textenc_attention_bf16: bad B / H");
  DRAG_CHECK(S >= 1 && S <= 512, "drag_textenc_attention_bf16: S must be in [1, 512] (the text encoders' sequence lengths)");
  DRAG_CHECK(ld >= H * 64 && ld % 8 == 0 && batch_stride >= (int64_t)S * ld && batch_stride % 8 == 0,
             "drag_textenc_attention_bf16: q/k/v rows need ld >= 64 H, ld % 8 == 0, batch_stride >= S ld and % 8 == 0");
  DRAG_CHECK(ld_o >= H * 64 && o_batch_stride >= (int64_t)S * ld_o, "drag_textenc_attention_bf16: bad output strides");
  DRAG_CHECK(aligned16(q) && aligned16(k) && aligned16(v), "drag_textenc_attention_bf16: q / k / v must be 16-byte aligned");
  TxtAttnArgs p{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, (const bf16_t*)rel_bias, S, H, ld,
                (long long)batch_stride, ld_o, (long long)o_batch_stride, scale, causal ? 1 : 0};
  const dim3 grid((S + 63) / 64, H, B);
  if (eager)
    hipLaunchKernelGGL(textenc_attention_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(textenc_attention_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_t5_rmsnorm_bf16(const void* x, const void* weight, void* y, int32_t M, int32_t D, float eps, void* stream) {
  DRAG_CHECK(M >= 0 && D >= 8 && D % 8 == 0 && D <= RMS_IT * 512, "drag_t5_rmsnorm_bf16: need D % 8 == 0 and 8 <= D <= 4096");
  if (M == 0) return 0;      // nothing to do: an empty tensor has no address to check
  DRAG_CHECK(x && weight && y, "drag_t5_rmsnorm_bf16: null pointer");
  DRAG_CHECK(aligned16(x) && aligned16(weight) && aligned16(y), "drag_t5_rmsnorm_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)weight,
                     (bf16_t*)y, M, D, eps);
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_gated_new_gelu_bf16(const void* h, void* y, int64_t M, int32_t F, void* stream) {
  DRAG_CHECK(M >= 0 && F >= 8 && F % 8 == 0, "drag_gated_new_gelu_bf16: need F % 8 == 0");
  const long long n8 = (long long)M * (F / 8);
  if (n8 == 0) return 0;
  DRAG_CHECK(h && y, "drag_gated_new_gelu_bf16: null pointer");
  DRAG_CHECK(aligned16(h) && aligned16(y), "drag_gated_new_gelu_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(gated_new_gelu_kernel, dim3(ew_blocks(n8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h, (bf16_t*)y, n8,
                     F / 8);
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_quick_gelu_bf16(const void* x, void* y, int64_t n, void* stream) {
  DRAG_CHECK(n >= 0 && n % 8 == 0, "drag_quick_gelu_bf16: need n % 8 == 0");
  if (n == 0) return 0;
  DRAG_CHECK(x && y, "drag_quick_gelu_bf16: null pointer");
  DRAG_CHECK(aligned16(x) && aligned16(y), "drag_quick_gelu_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y,
                     (long long)(n / 8));
  DRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int drag_embed_gather_bf16(const int64_t* ids, const void* table, const void* pos, void* out, int64_t rows, int32_t S,
                                      int32_t D, int64_t vocab, void* stream) {
  DRAG_CHECK(rows >= 0 && S >= 1 && D >= 8 && D % 8 == 0 && vocab >= 1, "drag_embed_gather_bf16: need D % 8 == 0, S >= 1, vocab >= 1");
  const long long n8 = (long long)rows * (D / 8);
  if (n8 == 0) return 0;
  DRAG_CHECK(ids && table && out, "drag_embed_gather_bf16: null pointer");
  DRAG_CHECK(aligned16(table) && aligned16(out) && (!pos || aligned16(pos)), "drag_embed_gather_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(embed_gather_kernel, dim3(ew_blocks(n8)), dim3(256), 0, (hipStream_t)stream, ids, (const bf16_t*)table,
                     (const bf16_t*)pos, (bf16_t*)out, (long long)rows, S, D / 8, (long long)vocab);
  DRAG_LAUNCH_CHECK();
  return 0;
}
