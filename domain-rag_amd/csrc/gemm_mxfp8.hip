// gemm_mxfp8.hip — host side of drag_gemm_mxfp8: argument checks, kernel choice, launch.  The kernels: gemm_mxfp8_simple.hip.
#include "gemm_mxfp8.h"

using namespace drag_gemm;

extern "C" int drag_gemm_mxfp8(const drag_gemm_mx_args* a, void* stream) {
  DRAG_CHECK(a != nullptr, "drag_gemm_mxfp8: null args");
  DRAG_CHECK(a->Aq && a->Ascale && a->Wq && a->Wscale && a->C, "drag_gemm_mxfp8: null operand pointer");
  DRAG_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "drag_gemm_mxfp8: M, N, K must be positive");
  DRAG_CHECK(a->K % 128 == 0, "drag_gemm_mxfp8: K must be a multiple of 128");
  DRAG_CHECK(a->N % 8 == 0, "drag_gemm_mxfp8: N must be a multiple of 8");
  DRAG_CHECK(a->ldc % 4 == 0 && a->ldc >= a->N, "drag_gemm_mxfp8: ldc %% 4 == 0 and ldc >= N required");
  DRAG_CHECK((((uintptr_t)a->Aq | (uintptr_t)a->Wq) & 15) == 0, "drag_gemm_mxfp8: Aq and Wq must be 16-byte aligned");
  DRAG_CHECK((((uintptr_t)a->Ascale | (uintptr_t)a->Wscale) & 3) == 0, "drag_gemm_mxfp8: Ascale and Wscale must be 4-byte aligned");
  DRAG_CHECK(((uintptr_t)a->C & 7) == 0 && (!a->resid || ((uintptr_t)a->resid & 7) == 0) && (!a->bias || ((uintptr_t)a->bias & 7) == 0) &&
                 (!a->gate || (((uintptr_t)a->gate & 7) == 0 && a->ldg % 4 == 0)),
             "drag_gemm_mxfp8: C, bias, gate and resid must be 8-byte aligned (ldg %% 4 == 0)");
  DRAG_CHECK(!(a->gate && !a->resid), "drag_gemm_mxfp8: gate needs resid");
  DRAG_CHECK(a->act == DRAG_ACT_NONE || a->act == DRAG_ACT_GELU_TANH || a->act == DRAG_ACT_SILU || a->act == DRAG_ACT_QUICK_GELU,
             "drag_gemm_mxfp8: fused activation must be none, gelu-tanh, silu or quick-gelu");
  const int rpb = a->c_rows_per_batch > 0 ? a->c_rows_per_batch : a->M;
  DRAG_CHECK(rpb >= a->M || a->c_batch_stride % 4 == 0, "drag_gemm_mxfp8: c_batch_stride %% 4 == 0 required");
  // "gemm_mx_kernel": 0 = policy, 1 = the 128x128 kernel, 2 = the wide (256x256, persistent) kernel — which this library does not build
  // yet: the policy gives every launch to the 128x128 kernel
  const int force = drag_opt(DRAG_OPT_GEMM_MX_KERNEL);
  DRAG_CHECK(force == 0 || force == 1, "drag_gemm_mxfp8: gemm_mx_kernel must be 0 (policy) or 1 (the 128x128 kernel); the wide kernel (2) is not built");

  MxKArgs k;
  GemmKArgs& g = k.g;
  g.A = nullptr; g.W = nullptr; g.C = a->C;
  g.bias = (const bf16_t*)a->bias; g.gate = (const bf16_t*)a->gate; g.resid = (const bf16_t*)a->resid;
  g.M = a->M; g.N = a->N; g.K = a->K;
  g.am = RowMap{a->M, 0, a->K};
  g.cm = RowMap{rpb, a->c_batch_stride, a->ldc};
  g.cv = ConvMap{1, 1, 1, 1, 64, 1, 0, 0};
  g.ldg = a->ldg; g.act = a->act; g.act_n0 = a->act_n0; g.out_f32 = 0;
  g.a_bytes = 0; g.w_bytes = 0;
  g.tiles_m = (a->M + BM - 1) / BM; g.tiles_n = (a->N + BN - 1) / BN;
  // the staged 16-byte epilogue where rows allow it (the bf16 GEMM's rule)
  g.wide = a->ldc % 8 == 0 && ((uintptr_t)a->C & 15) == 0 && (rpb >= a->M || a->c_batch_stride % 8 == 0) &&
           (!a->resid || ((uintptr_t)a->resid & 15) == 0) && (!a->gate || (((uintptr_t)a->gate & 15) == 0 && a->ldg % 8 == 0)) &&
           !drag_opt(DRAG_OPT_GEMM_NARROW);
  g.C2 = nullptr; g.ld2 = 0; g.n_split = 0;
  g.group_m = drag_opt(DRAG_OPT_GEMM_GROUP_M) > 0 ? drag_opt(DRAG_OPT_GEMM_GROUP_M) : 8;
  g.ldw = a->K; g.w_boff = 0; g.split_m1 = 0; g.w4_late_state = 0;
  g.epi_generic = drag_opt(DRAG_OPT_GEMM_EPILOGUE) == 1;
  g.seg_tiles_m = 0; g.A2 = nullptr; g.W2 = nullptr; g.Cs2 = nullptr; g.bias2 = nullptr; g.gate2 = nullptr; g.resid2 = nullptr;
  g.M2 = 0; g.ldg2 = 0; g.wide2 = 0; g.am2 = RowMap{1, 0, 0}; g.cm2 = RowMap{1, 0, 0};
  k.Aq = (const uint8_t*)a->Aq; k.As = (const uint8_t*)a->Ascale; k.Wq = (const uint8_t*)a->Wq; k.Ws = (const uint8_t*)a->Wscale;
  DRAG_CHECK((long long)g.tiles_m * g.tiles_n < (1ll << 31), "drag_gemm_mxfp8: too many tiles");
  hipLaunchKernelGGL(gemm_mxfp8_simple, dim3(g.tiles_m * g.tiles_n), dim3(256), 0, (hipStream_t)stream, k);
  DRAG_LAUNCH_CHECK();
  return 0;
}
