// gemm_bf16.hip — C[M,N] = epilogue(A[M,K] · W[N,K]^T) on gfx950 MFMA (bf16 in, fp32 accumulate).
//
// Replaces every torch.nn.Linear the reference reaches through diffusers/transformers/clip
// (FluxTransformerBlock / FluxSingleTransformerBlock projections and MLPs,
// embedders, SigLIP / CLIP ViT linears; call sites batch_generate_flux_kshot.py:467-474 and
// outpainting_updown_sampling_redux.py:1246-1257).  Both operands are K-contiguous
// (torch Linear weight layout), which is the natural MFMA operand layout.
//
// This file is the host side: tile policy, launch, split-K and the C ABI.  The kernels, their shared epilogue code and what each is for:
// gemm_bf16_kernels.h and the gemm_bf16_*.hip sources it names.
#include "gemm_bf16_kernels.h"
#include "drag_launch.h"
#include <stdio.h>
#include <stdlib.h>

using namespace drag_gemm;

// tile policy: the 256x256 kernel needs enough tiles to fill 256 CUs and rows to amortise its prologue
// tile policy (both kernels give bit-identical results: same k-order per output element).  The 256x256 kernel is the
// faster one per tile, but it needs enough tiles to fill the 256 CUs and loses to the 128x128 kernel when the last round of
// tiles is mostly empty (measured at M = 1024 / 1536 / 1753, scripts/bench_gemm_small_m.py: 216 tiles 1226 vs 957 TFLOP/s,
// 504 tiles 1384 vs 1069, but 72 tiles 510 vs 680 and 288 tiles 927 vs 993).
// rows of tiles of height tm over one problem, or over the two row segments of a pair (each segment starts on a tile boundary)
static long long tile_rows(long long M1, long long M2, int tm) { return (M1 + tm - 1) / tm + (M2 > 0 ? (M2 + tm - 1) / tm : 0); }

static bool use_t256(long long M1, long long M2, int N, int K) {
  if (drag_opt(DRAG_OPT_GEMM_T128) || N < 256 || K < 256) return false;
  const long long M = M1 + M2;
  if (M >= 2048 && M2 == 0) return true;
  if (M < 1024) return false;
  const long long tiles = tile_rows(M1, M2, 256) * ((N + 255) / 256);
  if (tiles < 128) return false;
  if (tiles <= 256) return true;
  const long long rounds = (tiles + 255) / 256;
  return tiles * 10 >= rounds * 256 * 7;              // last-round efficiency >= 0.7
}

// Which kernel a launch the 256x256 rule above does not take should use: 0 = t128, 2 = the 256x256 kernel after all, else
// gemm_bf16_deep<MI, ST, NI> as 100 * (NI == 6) + 10 * MI + ST.  Every choice gives the same bits; the choice is a function of the shape.
//
// Model.  A launch of few tiles is bound by what its busiest CU pulls through the L2 -> LDS path:
//   cost = (workgroups the busiest CU runs) x (tile rows + tile columns)          [per K-step; comparable at equal K]
// and the measurements that calibrate it are taken with COLD weights (COLD=1 in scripts/bench_gemm_small_m.py / bench_gemm_pair.py:
// every launch reads a matrix no recent launch touched) — inside a batch-1 forward 24 GB of weights pass a 256 MB Infinity Cache, so a
// pipeline never sees the hot state in which an isolated benchmark re-reads one matrix (hot, K = 3072 launches tip towards t128's two
// workgroups per CU: (512, 12288, 3072) t128 879 vs 128x192 825; cold 580 vs 839).
//
// Rules, in order (TFLOP/s cold, old choice -> new):
//  * <= 32 rows or < 64 tiles of 64 rows: 32-row tiles, 4-stage ring — (8, 18432, 3072), the AdaLN modulation at batch 8: an HBM
//    stream of the weight, 27 -> 46 hot (5.7 TB/s); (64, 3072, 3072) 38 -> 68.
//  * fallback by tile count: <= 128 tiles of 128x128 -> 64x128 tiles, one workgroup per CU, 4-stage ring; <= 256 -> 64x128, two per CU,
//    3-stage; more -> t128 (two workgroups per CU, 128x128) or 96x128 tiles with a 2-stage ring (two per CU as well) when the model
//    prefers them: the pair (1024 + 512, 3072, 3072) 288 128-row tiles (32 CUs carry two) 696 -> 408 96-row tiles 806 hot;
//    (512, 9216, 3072) 673 -> 820 hot; not (1458, 4304, 1152) 699 vs 497.  Past one round such workgroups come in rounds of 512 and a
//    partly filled last round costs a full one (paired_rounds).
//  * ONE round of one-workgroup-per-CU ring tiles on >= 75 % of the CUs — the cheapest (32 MI) x (128 | 192) tiling that is — replaces the
//    fallback when it cuts the cost by >= 10 %: (1536, 3072, 15360) t128 686 -> 96x192 873 (128x192 821); (512, 12288, 3072) 580 -> 128x192
//    839; the pair (1024 + 512, 3072, 12288) with gate + residual 622 -> 128x192 781; (1024, 3072, 12288) 64x128 511 -> 128x128 681
//    (64x192 632); (729, 4096, 1152) 64x128 393 -> 96x128 487.  Ring depths 2 and 4 of the 192-column tiles were measured too (codes
//    1x2 / 1x4): 4 changes nothing, 2 (two workgroups per CU) loses.
//  * a partly filled second round of 256x256 tiles when even that is cheaper: (1536, 12288, 3072) 96x128 797 / t128 772 -> 908.
// M2 > 0: the rows of a drag_gemm_bf16_pair launch (tile counts are per segment).  *cost_out: the chosen tiling's cost.
static long long paired_rounds(long long tiles) { return tiles <= 256 ? 1 : 2 * ((tiles + 511) / 512); }

static int deep_policy(long long M1, long long M2, int N, int K, long long* cost_out) {
  const long long M = M1 + M2;
  const long long tn = (N + 127) / 128;
  int pick;
  long long cost;                                   // of the 128-column choice, in the units above
  const long long tiles128 = tile_rows(M1, M2, 128) * tn, tiles64 = tile_rows(M1, M2, 64) * tn;
  if (M <= 32 || tiles64 < 64) {                   // 32-row tiles: no MFMA work on rows that do not exist, more workgroups
    if (cost_out) *cost_out = ((tile_rows(M1, M2, 32) * tn + 255) / 256) * (32 + 128);
    return 14;
  }
  if (tiles128 <= 128) { pick = 24; cost = ((tiles64 + 255) / 256) * (64 + 128); }        // <= 256 workgroups of 64 x 128: one per CU, 4-stage ring (96 KiB)
  else if (tiles128 <= 256) { pick = 23; cost = ((tiles64 + 255) / 256) * (64 + 128); }   // <= 512 workgroups: two per CU, 3-stage ring (72 KiB each)
  else { pick = 0; cost = paired_rounds(tiles128) * (128 + 128); }
  if (pick == 0 && !drag_opt(DRAG_OPT_GEMM_NO_96)) {
    const long long c96 = paired_rounds(tile_rows(M1, M2, 96) * tn) * (96 + 128);
    if (c96 < cost) { pick = 32; cost = c96; }
  }
  // one round of ring tiles (ties: the larger MI at 128 columns)
  const bool no192 = drag_opt(DRAG_OPT_GEMM_NO_192) != 0;
  long long cbest = 0;
  int best = 0;
  if (M >= 256) {
    for (int mi = 4; mi >= 1; --mi)
      for (int ni = 4; ni <= 6; ni += 2) {
        if (ni == 6 && (N % 192 != 0 || no192)) continue;
        const long long tiles = tile_rows(M1, M2, 32 * mi) * ((N + 32 * ni - 1) / (32 * ni));
        if (tiles > 256 || tiles < 192) continue;
        const long long c = 32 * mi + 32 * ni;
        if (best == 0 || c < cbest) { best = ni == 6 ? 100 + 10 * mi + 3 : (mi >= 3 ? 10 * mi + 3 : 10 * mi + 4); cbest = c; }
      }
  }
  if (best && cbest * 10 <= cost * 9) {
    if (cost_out) *cost_out = cbest;
    return best;
  }
  // a partly filled second round of 256x256 tiles
  if (pick != 24 && pick != 23 && M >= 1024 && N >= 256 && K >= 256 && !drag_opt(DRAG_OPT_GEMM_T128)) {
    const long long c256 = ((tile_rows(M1, M2, 256) * ((N + 255) / 256) + 255) / 256) * (256 + 256);
    if (c256 < cost) { pick = 2; cost = c256; }
  }
  if (cost_out) *cost_out = cost;
  return pick;
}

// persistent grid of the 256x256 kernel: one workgroup per CU (128 KiB of LDS each), fewer when there are fewer tiles
static int t256_grid(int ntiles) {
  if (drag_opt(DRAG_OPT_GEMM_NONPERSISTENT)) return ntiles;
  int ncu = drag_cu_count() & ~7;                  // multiple of the 8 XCDs, so a workgroup's tiles stay on its XCD's L2
  if (ncu == 0) ncu = 8;
  return ntiles < ncu ? ntiles : ncu;
}

// ---- THE table of the kernels behind drag_gemm_bf16 / drag_gemm_bf16_pair / drag_conv3x3_bf16: one row per code ("gemm_kernel",
// drag_gemm_bf16_choice) with everything a launch needs.  gemm_launch, the "not built" refusal, drag_gemm_bf16_kernel_code and
// drag_gemm_bf16_kernel_name read it; the ring rows come from the lists of gemm_bf16_kernels.h.
namespace drag_gemm {
using LaunchFn = int (*)(dim3 grid, int block, int lds, hipStream_t st, const GemmKArgs& p);
// a code's kernel per form: batched rows | a merged pair, where that is a kernel of its own (else the rows kernel runs it) | conv3x3
enum { FORM_ROWS, FORM_PAIR, FORM_CONV, FORMS };
struct KernelForm { const char* name; LaunchFn launch; };      // the name as a profiler prints it; {null, null}: not built
struct KernelRow {
  int code, tm, tn, block, lds;      // tile rows x columns, threads per workgroup, dynamic LDS bytes
  bool persistent;                   // one workgroup per CU walks the tiles (t256_grid), else one workgroup per tile
  KernelForm form[FORMS];
};
#define DRAG_FORM(...) {#__VA_ARGS__, drag_launch<__VA_ARGS__>}
#define DRAG_NI_NAME_4 ""
#define DRAG_NI_NAME_6 ", 6"
#define DRAG_DEEP_ROW(MI_, ST_, NI_)                                                                                       \
  {(NI_ == 6 ? 100 : 0) + 10 * MI_ + ST_, 32 * MI_, 32 * NI_, 256, ST_ * (32 * MI_ + 32 * NI_) * 128, false,              \
   {{"gemm_bf16_deep<" #MI_ ", " #ST_ DRAG_NI_NAME_##NI_ ">", drag_launch<gemm_bf16_deep<MI_, ST_, NI_>>}}},
#define DRAG_W4_ROW(V_) {400 + V_, 256, 256, 256, 131072, false, {DRAG_FORM(gemm_bf16_w4<V_>)}},
constexpr KernelRow kernel_table[] = {
    {0, BM, BN, 256, 0, false, {DRAG_FORM(gemm_bf16_t128<0>), {}, DRAG_FORM(gemm_bf16_t128<1>)}},
    {2, 256, 256, 512, 0, true, {DRAG_FORM(gemm_bf16_t256<0>), DRAG_FORM(gemm_bf16_t256_pair), DRAG_FORM(gemm_bf16_t256<1>)}},
    {3, 256, 256, 256, 131072 + 4 * 4096, true, {DRAG_FORM(gemm_bf16_w4p)}},      // one segment, K % 128 == 0: gemm_choice
    DRAG_GEMM_DEEP_N128(DRAG_DEEP_ROW) DRAG_GEMM_DEEP_N192A(DRAG_DEEP_ROW) DRAG_GEMM_DEEP_N192B(DRAG_DEEP_ROW)
#if DRAG_EXP
    DRAG_GEMM_W4_VARIANTS(DRAG_W4_ROW)      // round-5 experiment: gemm_bf16_w4<variant>
#endif
};
#undef DRAG_FORM
#undef DRAG_DEEP_ROW
#undef DRAG_W4_ROW
constexpr int kernel_rows = (int)(sizeof(kernel_table) / sizeof(kernel_table[0]));

static const KernelRow* kernel_row(int code) {
  for (const KernelRow& r : kernel_table)
    if (r.code == code) return &r;
  return nullptr;
}
}  // namespace drag_gemm

// one form of a row over the k.tiles_m x k.tiles_n tiles of k
static int launch_row(const KernelRow& row, int form, const GemmKArgs& k, void* stream) {
  const int tiles = k.tiles_m * k.tiles_n;
  return row.form[form].launch(dim3(row.persistent ? t256_grid(tiles) : tiles), row.block, row.lds, (hipStream_t)stream, k);
}

extern "C" int32_t drag_gemm_bf16_kernel_code(int32_t index) { return index >= 0 && index < kernel_rows ? kernel_table[index].code : -1; }
extern "C" const char* drag_gemm_bf16_kernel_name(int32_t code, int32_t form) {
  const KernelRow* row = kernel_row(code);
  return row != nullptr && form >= 0 && form < FORMS ? row->form[form].name : nullptr;
}

static int fill_common(GemmKArgs& k, const void* A, const void* W, void* C, const void* bias, const void* gate,
                       const void* resid, int M, int N, int K, int ldc, int c_rpb, long long c_bs, int ldg, int act,
                       int act_n0, int out_f32) {
  k.A = (const bf16_t*)A; k.W = (const bf16_t*)W; k.C = C;
  k.bias = (const bf16_t*)bias; k.gate = (const bf16_t*)gate; k.resid = (const bf16_t*)resid;
  k.M = M; k.N = N; k.K = K;
  k.cm.rpb = c_rpb > 0 ? c_rpb : M; k.cm.bs = c_bs; k.cm.ld = ldc;
  k.ldg = ldg; k.act = act; k.act_n0 = act_n0; k.out_f32 = out_f32;
  k.a_bytes = 0; k.w_bytes = 0;
  k.ldw = K; k.w_boff = 0; k.split_m1 = 0;
  k.C2 = nullptr; k.ld2 = 0; k.n_split = 0;
  k.seg_tiles_m = 0; k.A2 = nullptr; k.W2 = nullptr; k.Cs2 = nullptr; k.bias2 = nullptr; k.gate2 = nullptr; k.resid2 = nullptr;
  k.M2 = 0; k.ldg2 = 0; k.wide2 = 0; k.am2 = RowMap{1, 0, 0}; k.cm2 = RowMap{1, 0, 0};
  // M tiles per group of the tile walk: the 32 concurrent tiles of an XCD form a group_m x (32 / group_m) super-tile.  4 and 8 tie on
  // the K = 3072 shapes (8 ahead by 1-3 % at N = 3072), 4 is 2-3 % ahead at K >= 12288; 16 / 32 (towards W-stationary) lose 5-10 %
  // everywhere (scripts/bench_gemm_group_m.py, two boxes).  Order only: the bits do not depend on it.
  k.epi_generic = drag_opt(DRAG_OPT_GEMM_EPILOGUE) == 1;
  k.w4_late_state = drag_opt(DRAG_OPT_GEMM_EPILOGUE) == 2;
  // Round 5 (profiles/r05_gemm_tile_walk_fetch_clock.txt: bytes the L2s pull per launch and the clock the launch gets, per setting): the
  // fabric traffic of a launch is A x tiles_n / (32 / g) + W x tiles_m / g and the chip — at its 1400 W socket cap in this kernel — pays for
  // it in clock (g = 1 on (42696, 21504, 3072): 23.4 GB and 1.48 GHz; g = 4: 11.5 GB and 1.77 GHz).  4 | 8 are the two minima; the wide
  // launches (N >= 16384: the single blocks' q|k|v|mlp Linear) run 1.5 % faster on 4.
  k.group_m = drag_opt(DRAG_OPT_GEMM_GROUP_M) > 0 ? drag_opt(DRAG_OPT_GEMM_GROUP_M) : (K >= 8192 || N >= 16384 ? 4 : 8);
  k.wide = !out_f32 && N % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)C & 15) == 0 && (k.cm.rpb >= M || c_bs % 8 == 0) &&
           (!resid || ((uintptr_t)resid & 15) == 0) && (!gate || (((uintptr_t)gate & 15) == 0 && ldg % 8 == 0)) &&
           !drag_opt(DRAG_OPT_GEMM_NARROW);
  k.tiles_m = (M + BM - 1) / BM; k.tiles_n = (N + BN - 1) / BN;
  return k.tiles_m * k.tiles_n;
}

// argument checks + kernel arguments of one row segment
static int gemm_prepare(GemmKArgs& k, const drag_gemm_args* a, bool k_slices = false) {
  DRAG_CHECK(a != nullptr, "drag_gemm_bf16: null args");
  DRAG_CHECK(a->A && a->W && a->C, "drag_gemm_bf16: null operand pointer");
  DRAG_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "drag_gemm_bf16: M, N, K must be positive");
  DRAG_CHECK(a->K % BK == 0, "drag_gemm_bf16: K must be a multiple of 64 (pad the weight)");
  DRAG_CHECK(a->N % 4 == 0, "drag_gemm_bf16: N must be a multiple of 4");
  DRAG_CHECK(a->lda % 8 == 0 && a->ldc % 4 == 0, "drag_gemm_bf16: lda %% 8 and ldc %% 4 required");
  DRAG_CHECK(!(a->gate && !a->resid), "drag_gemm_bf16: gate needs resid");
  DRAG_CHECK(a->act == DRAG_ACT_NONE || a->act == DRAG_ACT_GELU_TANH || a->act == DRAG_ACT_SILU || a->act == DRAG_ACT_QUICK_GELU,
             "drag_gemm_bf16: fused activation must be none, gelu-tanh, silu or quick-gelu (erf GELU: use drag_act_bf16)");
  fill_common(k, a->A, a->W, a->C, a->bias, a->gate, a->resid, a->M, a->N, a->K, a->ldc, a->c_rows_per_batch, a->c_batch_stride, a->ldg,
              a->act, a->act_n0, a->out_f32);
  k.am.rpb = a->a_rows_per_batch > 0 ? a->a_rows_per_batch : a->M;
  k.am.bs = a->a_batch_stride; k.am.ld = a->lda;
  k.cv = ConvMap{1, 1, 1, 1, 64, 1, 0, 0};
  // in-tile offsets are 32-bit and must grow with the row index
  // (k_slices: the row batches of a split-K launch are K slices of the SAME rows — batch stride = the slice width; its tiles never
  //  cross a batch: M % 256 == 0)
  DRAG_CHECK(k_slices || k.am.rpb >= a->M || k.am.bs >= (long long)(k.am.rpb - 1) * k.am.ld,
             "drag_gemm_bf16: a_batch_stride must not be smaller than one batch of rows");
  DRAG_CHECK(((long long)BM * a->lda + a->K) * 2 < (1ll << 30) && (long long)BN * a->K * 2 < (1ll << 31) &&
                 (k_slices || k.am.rpb >= a->M || (k.am.bs - (long long)(k.am.rpb - 1) * k.am.ld) * 2 < (1ll << 30)),
             "drag_gemm_bf16: tile span too large for 32-bit offsets");
  if (a->C2 != nullptr) {
    DRAG_CHECK(a->n_split > 0 && a->n_split < a->N && a->n_split % 256 == 0, "drag_gemm_bf16: n_split must be a multiple of 256 inside (0, N)");
    DRAG_CHECK(!a->out_f32 && !a->gate && !a->resid && a->c_rows_per_batch <= 0, "drag_gemm_bf16: the two-destination form takes dense bf16 outputs without gate / residual");
    DRAG_CHECK(a->ldc2 >= a->N - a->n_split && a->ldc >= a->n_split, "drag_gemm_bf16: ldc / ldc2 too small for their column ranges");
    k.C2 = a->C2; k.ld2 = a->ldc2; k.n_split = a->n_split;
    k.wide = k.wide && a->ldc2 % 8 == 0 && ((uintptr_t)a->C2 & 15) == 0;
    DRAG_CHECK(k.wide || a->ldc2 % 4 == 0, "drag_gemm_bf16: ldc2 % 4 required");
  }
  return 0;
}

// kernel choice for M rows (the sum over the segments of a pair): 2 = t256, 0 = t128, else a gemm_bf16_deep code.
// "gemm_kernel" (drag_set_option, measurement only): 0 = policy, 1 = t128, 2 = t256, 10*MI + ST = gemm_bf16_deep<MI, ST>
static int gemm_choice(long long M1, long long M2, int N, int K, long long* cost_out = nullptr) {
  const int force = drag_opt(DRAG_OPT_GEMM_KERNEL);
  long long cost = 0;
  int choice;
  // 3 = gemm_bf16_w4p (round 5): the same 256 x 256 tiles as four waves x (128 x 128) with the hand-placed K loop — same bits, +1...+5 % on
  // the launches the persistent 8-wave kernel takes (profiles/r05_gemm_w4p_*.log) once a launch has enough tiles (below); one row
  // segment, K a multiple of 128 ("gemm_w4" = 1: never; "gemm_kernel" = 3 forces it wherever it can run)
  const bool w4_ok = M2 == 0 && N >= 256 && K >= 256 && K % 128 == 0;
  if (force >= 10) choice = force;
  else if (force == 3) choice = w4_ok ? 3 : ((N >= 256 && K >= 256) ? 2 : 0);
  else if (force == 2) choice = (N >= 256 && K >= 256) ? 2 : 0;
  else if (force == 1) choice = 0;
  else if (use_t256(M1, M2, N, K)) {
    choice = 2;
    cost = ((tile_rows(M1, M2, 256) * ((N + 255) / 256) + 255) / 256) * (256 + 256);
    // its fixed cost per tile is 7 us against 4.5 and its first tile starts cold: three rounds of tiles, or one with long K loops, amortise
    // that (configs[1]'s two-round (1536, 21 504, 3072) launch lost 2 %: profiles/r05_gemm_w4p_fixed_cost.log)
    const long long tiles4 = tile_rows(M1, 0, 256) * ((N + 255) / 256);
    const int w4 = drag_opt(DRAG_OPT_GEMM_W4);      // 1 never | 2 every launch of the 8-wave kernel it can run | 3 those of >= 256 tiles
    const bool enough = w4 == 2 ? true : w4 == 3 ? tiles4 >= 256 : tiles4 >= 256 && (K >= 8192 || tiles4 >= 768);
    if (w4_ok && w4 != 1 && enough) choice = 3;
  } else choice = deep_policy(M1, M2, N, K, &cost);
  if (cost_out) *cost_out = cost;
  return choice;
}

// one launch over the rows of `a` and, when b != nullptr, of a second segment with the same N, K and epilogue form
// w_total_k > 0: `a` is the stacked form of a split-K launch (gemm_splitk): row batch b of A is K slice b, W's rows are w_total_k wide
static int gemm_launch(const drag_gemm_args* a, const drag_gemm_args* b, void* stream, int w_total_k = 0, const drag_gemm_args* split_second = nullptr) {
  GemmKArgs k, k2;
  if (int rc = gemm_prepare(k, a, w_total_k > 0)) return rc;
  if (w_total_k > 0) {
    k.ldw = w_total_k; k.w_boff = a->K;
    if (split_second) { k.split_m1 = a->a_rows_per_batch - split_second->M; k.A2 = (const bf16_t*)split_second->A; k.W2 = (const bf16_t*)split_second->W; }
  }
  if (b != nullptr) {
    if (int rc = gemm_prepare(k2, b)) return rc;
    k.A2 = k2.A; k.W2 = k2.W; k.Cs2 = k2.C; k.bias2 = k2.bias; k.gate2 = k2.gate; k.resid2 = k2.resid;
    k.M2 = k2.M; k.ldg2 = k2.ldg; k.wide2 = k2.wide; k.am2 = k2.am; k.cm2 = k2.cm;
  }
  const int choice = w_total_k > 0 ? 3 : gemm_choice(a->M, b ? b->M : 0, a->N, a->K);      // (the W offsets of the slices exist in gemm_bf16_w4p only)
  const KernelRow* row = kernel_row(choice);
  if (row == nullptr) {
    char msg[512];
    size_t n = (size_t)snprintf(msg, sizeof(msg), "drag_gemm_bf16: gemm_kernel names a kernel that is not built (built, as drag_gemm_bf16_kernel_code lists them:");
    for (int i = 0; i < kernel_rows && n < sizeof(msg); ++i) n += (size_t)snprintf(msg + n, sizeof(msg) - n, " %d", kernel_table[i].code);
    if (n < sizeof(msg)) snprintf(msg + n, sizeof(msg) - n, ")");
    drag_set_error(msg);
    return -1;
  }
  if (choice >= 400)            // round-5 experiment: gemm_bf16_w4<variant>
    DRAG_CHECK(a->K % 128 == 0 && a->K >= 256 && b == nullptr, "drag_gemm_bf16: gemm_kernel 400 (gemm_bf16_w4) needs K % 128 == 0, K >= 256, one segment");
  // the 4-wave persistent kernel's own tile walk (profiles/r05_gemm_w4p_group_m.log, interleaved, TFLOP/s at g = 2 | 4 | 8): (42 696, 21 504, 3072)
  // 1468 | 1449 | 1419, (32 768, 9216, 3072) 1473 | 1497 | 1481, (32 768, 3072, 12 288) 1520 | 1528 | 1513, (32 768, 3072, 3072) 1456 | 1423 | 1451
  if (choice == 3 && drag_opt(DRAG_OPT_GEMM_GROUP_M) <= 0) k.group_m = a->N >= 16384 ? 2 : (a->N <= 3072 && a->K < 8192 ? 8 : 4);
  k.tiles_m = (a->M + row->tm - 1) / row->tm;            // each segment starts on a tile boundary
  if (b) { k.seg_tiles_m = k.tiles_m; k.tiles_m += (b->M + row->tm - 1) / row->tm; }
  k.tiles_n = (a->N + row->tn - 1) / row->tn;
  return launch_row(*row, b && row->form[FORM_PAIR].launch ? FORM_PAIR : FORM_ROWS, k, stream);
}

// --------------------------------------------------------------------------------------------
// Split-K (round 5): a Linear with few output tiles and a long K — the single blocks' proj_out at batch 1, 1536 x 3072 x 15 360: 72 tiles
// of 256 x 256 on 256 CUs, or 256 tiles of 96 x 192 with half the arithmetic intensity (today's choice: 177 us, L2 -> LDS bound) — runs as
// ONE launch of gemm_bf16_w4p over S stacked K slices ((S M) x N x (K / S), f32 partial products into the caller's workspace: 216 tiles,
// 115 us) and one pass that adds the slices in order and applies the epilogue (splitk_reduce_kernel, the arithmetic of epi_row).  The sum
// of S f32 chains is not the single chain's bits: the one place where the kernel choice changes the last bit of an output — accuracy
// against the f32 oracle is the same (tests) — hence policy only where it pays (below) and "gemm_splitk" = 1 to switch it off.
// The workspace is the caller's (drag_gemm_set_workspace, per device): no allocation on the launch path, safe under graph capture;
// launches that use it must be ordered on one stream.
// --------------------------------------------------------------------------------------------
static void* g_splitk_ws[64];
static long long g_splitk_ws_bytes[64];
extern "C" int drag_gemm_set_workspace(void* ptr, int64_t bytes) {
  int dev = 0;
  DRAG_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "drag_gemm_set_workspace: no current device");
  DRAG_CHECK((ptr == nullptr) == (bytes <= 0) && ((uintptr_t)ptr & 255) == 0, "drag_gemm_set_workspace: a 256-byte aligned device buffer and its size, or (null, 0)");
  g_splitk_ws[dev] = ptr;
  g_splitk_ws_bytes[dev] = ptr ? (long long)bytes : 0;
  return 0;
}

struct SplitReduceArgs {
  const float* part;      // [S][slice_rows][N]; this problem's rows begin at row0 of every slice
  int slice_rows, row0;
  bf16_t* C;
  const bf16_t *bias, *gate, *resid;
  int S, M, N, ldg;
  RowMap cm;
};
// one thread = four consecutive columns of one row: v = bias + sum over the slices in order; then epi_row's forms.  Every load of the thread —
// S partial quads, bias, gate, residual — is issued before the first add (S is a template parameter: with a run-time loop the compiler
// waited for slice s before requesting s + 1: 28 us for the 75 MB of a (1536, 3072) x 3 launch, a third of the HBM rate)
template <int S>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(SplitReduceArgs p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n4 = p.N / 4;
  if (i >= (long long)p.M * n4) return;
  const int m = (int)(i / n4), n = (int)(i - (long long)m * n4) * 4;
  f32x4_t part[S];
#pragma unroll
  for (int s = 0; s < S; ++s) part[s] = __builtin_nontemporal_load((const f32x4_t*)(p.part + ((long long)s * p.slice_rows + p.row0 + m) * p.N + n));
  const long long coff = p.cm.off(m) + n;
  u32x2_t bb = {0u, 0u}, rr = {0u, 0u}, gg = {0u, 0u};
  if (p.bias) bb = *(const u32x2_t*)(p.bias + n);
  if (p.resid) rr = *(const u32x2_t*)(p.resid + coff);
  if (p.gate) gg = *(const u32x2_t*)(p.gate + (long long)(m / p.cm.rpb) * p.ldg + n);
  f32x4_t v = part[0];
#pragma unroll
  for (int s = 1; s < S; ++s) v += part[s];
  if (p.bias) { v[0] += bf_lo(bb[0]); v[1] += bf_hi(bb[0]); v[2] += bf_lo(bb[1]); v[3] += bf_hi(bb[1]); }
  if (p.resid) {
    const float x[4] = {bf_lo(rr[0]), bf_hi(rr[0]), bf_lo(rr[1]), bf_hi(rr[1])};
    if (p.gate) {      // diffusers: x + gate * y with y, gate, x bf16 tensors: y rounded first, the product rounded, then the sum
      const float g[4] = {bf_lo(gg[0]), bf_hi(gg[0]), bf_lo(gg[1]), bf_hi(gg[1])};
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * rbf(v[r]));
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(v[r]);
    }
  }
  u32x2_t o;
  o[0] = pack2bf(v[0], v[1]);
  o[1] = pack2bf(v[2], v[3]);
  *(u32x2_t*)(p.C + coff) = o;
}

// slices of a launch (0: not split).  Policy: at most 96 tiles of 256 x 256 (three eighths of the chip), K >= 12 288, as many slices as fit
// one round of workgroups (<= 8, slices of whole 128-wide K-step pairs, >= 1024 wide); "gemm_splitk": 1 never | n >= 2 that many where valid
static int splitk_slices(const drag_gemm_args* a, const drag_gemm_args* b = nullptr) {
  const int opt = drag_opt(DRAG_OPT_GEMM_SPLITK);
  if (opt == 1 || drag_opt(DRAG_OPT_GEMM_KERNEL) != 0) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || g_splitk_ws[dev] == nullptr) return 0;
  auto fits = [](const drag_gemm_args* x) {
    return x->M % 256 == 0 && x->N % 256 == 0 && !x->out_f32 && !x->C2 && x->act == DRAG_ACT_NONE &&
           !(x->a_rows_per_batch > 0 && x->a_rows_per_batch < x->M) &&          // A is one dense batch
           x->ldc % 4 == 0 && x->ldg % 4 == 0 && !(x->c_rows_per_batch > 0 && x->c_batch_stride % 4);
  };
  if (!fits(a) || (b && (!fits(b) || b->lda != a->lda || b->N != a->N || b->K != a->K))) return 0;
  const long long rows = a->M + (b ? b->M : 0);
  const long long tiles = (rows / 256) * (a->N / 256);
  int best = 0;
  for (int s = 2; s <= 8; ++s) {
    if (a->K % (128 * s) || a->K / s < 1024 || tiles * s > 256) continue;
    if ((long long)s * rows * a->N * 4 > g_splitk_ws_bytes[dev]) continue;
    best = s;
  }
  if (opt >= 2) return (opt <= 8 && a->K % (128 * opt) == 0 && a->K / opt >= 256 && (long long)opt * rows * a->N * 4 <= g_splitk_ws_bytes[dev]) ? opt : 0;
  return (tiles <= 96 && a->K >= 12288) ? best : 0;      // (K = 8192: two slices of 72 tiles lose 3 %: profiles/r05_gemm_splitk_ab.log)
}

static int splitk_reduce(const drag_gemm_args* a, int S, int slice_rows, int row0, const float* part, void* stream) {
  SplitReduceArgs r{};
  r.part = part; r.slice_rows = slice_rows; r.row0 = row0; r.C = (bf16_t*)a->C;
  r.bias = (const bf16_t*)a->bias; r.gate = (const bf16_t*)a->gate; r.resid = (const bf16_t*)a->resid;
  r.S = S; r.M = a->M; r.N = a->N; r.ldg = a->ldg;
  r.cm.rpb = a->c_rows_per_batch > 0 ? a->c_rows_per_batch : a->M; r.cm.bs = a->c_batch_stride; r.cm.ld = a->ldc;
  const long long n = (long long)a->M * (a->N / 4);
  const dim3 g((unsigned)((n + 255) / 256));
  switch (S) {
#define DRAG_RED(S_) case S_: hipLaunchKernelGGL(splitk_reduce_kernel<S_>, g, dim3(256), 0, (hipStream_t)stream, r); break
    DRAG_RED(2); DRAG_RED(3); DRAG_RED(4); DRAG_RED(5); DRAG_RED(6); DRAG_RED(7); DRAG_RED(8);
#undef DRAG_RED
    default: DRAG_CHECK(false, "drag_gemm_bf16: 2 ... 8 K slices");
  }
  DRAG_LAUNCH_CHECK();
  return 0;
}

// b != nullptr: a pair (same N, K, row stride of A): ONE partial launch over S x (M_a + M_b) rows, one reduce pass per problem
static int gemm_splitk(const drag_gemm_args* a, const drag_gemm_args* b, int S, void* stream) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int rows = a->M + (b ? b->M : 0);
  drag_gemm_args v{};
  v.A = a->A; v.W = a->W; v.C = g_splitk_ws[dev];
  v.M = S * rows; v.N = a->N; v.K = a->K / S;
  v.lda = a->lda; v.a_rows_per_batch = rows; v.a_batch_stride = a->K / S;
  v.ldc = a->N; v.c_rows_per_batch = rows; v.c_batch_stride = (long long)rows * a->N;
  v.out_f32 = 1;
  if (int rc = gemm_launch(&v, nullptr, stream, a->K, b)) return rc;
  if (int rc = splitk_reduce(a, S, rows, 0, (const float*)g_splitk_ws[dev], stream)) return rc;
  return b ? splitk_reduce(b, S, rows, a->M, (const float*)g_splitk_ws[dev], stream) : 0;
}

extern "C" int drag_gemm_bf16(const drag_gemm_args* a, void* stream) {
  if (a != nullptr && a->A && a->W && a->C && a->M > 0 && a->N > 0 && a->K > 0) {
    if (const int S = splitk_slices(a)) {
      DRAG_CHECK(!(a->gate && !a->resid), "drag_gemm_bf16: gate needs resid");
      return gemm_splitk(a, nullptr, S, stream);
    }
  }
  return gemm_launch(a, nullptr, stream);
}
extern "C" int drag_gemm_bf16_splitk_slices(const drag_gemm_args* a) { return a ? splitk_slices(a) : 0; }
extern "C" int drag_gemm_bf16_pair_splitk_slices(const drag_gemm_args* a, const drag_gemm_args* b) { return a && b ? splitk_slices(a, b) : 0; }

// which kernel a launch over M1 (+ M2: a merged pair) rows takes: 2 = the persistent 256x256 kernel, 0 = t128, else
// 100 * (192-column tiles) + 10 * MI + ST of gemm_bf16_deep<MI, ST, NI> — for callers that account launches per kernel
extern "C" int drag_gemm_bf16_choice(int M1, int M2, int N, int K) { return gemm_choice(M1, M2 > 0 ? M2 : 0, N, K); }
// the policy's cost of that launch: tile rounds on the busiest CU x (tile rows + tile columns) — proportional to the bytes the busiest CU
// pulls through its L2 -> LDS path per K-step, which is what bounds a launch of few tiles.  0 under a forced "gemm_kernel".
extern "C" int64_t drag_gemm_bf16_cost(int M1, int M2, int N, int K) {
  long long c = 0;
  gemm_choice(M1, M2 > 0 ? M2 : 0, N, K, &c);
  return (int64_t)c;
}

// Two Linears with their own operands (A, W, bias, gate, residual, output, row maps) but the same N, K, activation and output type as
// ONE launch: the second problem's rows follow the first one's in the tile walk.  Every output element is computed exactly as by
// drag_gemm_bf16 on its own problem (same MFMA chain, same epilogue), so pair(a, b) == gemm(a); gemm(b) bit for bit; what changes is
// the occupancy of launches that are small alone (a double block's 512 text + 1024 image rows at batch 1: BASELINE configs[1]).
// Merged when the cost model above (tile rounds on the busiest CU x (tile rows + tile columns), each launch under the tiling the policy
// gives it) puts the one launch below the two, or level with them while at least one of the two is too small for the persistent kernel
// (a launch of about one round of workgroups pays its ring fill and epilogue in the open; merged, they overlap other workgroups).
// At batch 1 (1024 image + 512 text rows; TFLOP/s over both problems, isolated, scripts/bench_gemm_pair.py): the q|k|v pair
// 878 -> 1282, the attention output pair 559 -> 806, the MLP down-projection pair 667 -> 906; NOT the MLP up-projection (N = 12288:
// one round of 256x256 tiles + 1.5 of t128 alone, 4.5 rounds of t128 merged: 1084 -> 987) and not launches that each fill the chip
// alone (the headline's 4096 text + 32768 image rows: the merged launch idles what the smaller one idles alone).
// "gemm_pair": 0 = this rule, 1 = never merge, 2 = always merge.
extern "C" int drag_gemm_bf16_pair_merges(int M1, int M2, int N, int K) {
  const int opt = drag_opt(DRAG_OPT_GEMM_PAIR);
  if (opt == 1) return 0;
  if (opt == 2) return 1;
  long long c1 = 0, c2 = 0, cm = 0;
  const int k1 = gemm_choice(M1, 0, N, K, &c1);
  const int k2 = gemm_choice(M2, 0, N, K, &c2);
  gemm_choice(M1, M2, N, K, &cm);
  if (cm <= 0) return 0;                           // a forced kernel ("gemm_kernel"): no model
  auto persistent = [](int k) { return k == 2 || k == 3; };      // the 8-wave or the 4-wave 256 x 256 kernel
  return cm < c1 + c2 || (cm == c1 + c2 && (!persistent(k1) || !persistent(k2)));
}

extern "C" int drag_gemm_bf16_pair(const drag_gemm_args* a, const drag_gemm_args* b, void* stream) {
  DRAG_CHECK(a != nullptr && b != nullptr, "drag_gemm_bf16_pair: null args");
  DRAG_CHECK(a->N == b->N && a->K == b->K, "drag_gemm_bf16_pair: the two problems must share N and K");
  DRAG_CHECK(a->act == b->act && a->act_n0 == b->act_n0 && a->out_f32 == b->out_f32, "drag_gemm_bf16_pair: the two problems must share activation and output type");
  DRAG_CHECK(a->C2 == nullptr && b->C2 == nullptr, "drag_gemm_bf16_pair: no two-destination outputs");
  DRAG_CHECK((a->gate != nullptr) == (b->gate != nullptr) && (a->resid != nullptr) == (b->resid != nullptr) && (a->bias != nullptr) == (b->bias != nullptr),
             "drag_gemm_bf16_pair: the two problems must have the same epilogue operands");
  // a pair of few tiles and a long K (the double blocks' ff down-projections at batch 1: (1024 + 512) x 3072 x 12 288) splits as ONE partial
  // launch over both problems' rows + a reduce pass each: 150 -> 112 us alone, configs[1] 103.6 -> 102.7 ms.  (Two separately split launches
  // were 4 % faster than the merged pair alone and 1.2 % of configs[1] slower in the pipeline: profiles/r05_gemm_splitk_pairs_in_configs1.log.)
  if (a->A && a->W && a->C && b->A && b->W && b->C && a->M > 0 && b->M > 0 && a->N > 0 && a->K > 0) {
    if (const int S = splitk_slices(a, b)) {
      DRAG_CHECK(!(a->gate && !a->resid), "drag_gemm_bf16_pair: gate needs resid");
      return gemm_splitk(a, b, S, stream);
    }
  }
  if (!drag_gemm_bf16_pair_merges(a->M, b->M, a->N, a->K)) {
    // two launches: each through drag_gemm_bf16, i.e. under the SAME policy (split-K included) a caller issuing them one by one gets —
    // domain-rag_amd/ops.py gemm_pair does exactly that to account them separately, and the two APIs must give the same bits
    if (int rc = drag_gemm_bf16(a, stream)) return rc;
    return drag_gemm_bf16(b, stream);
  }
  return gemm_launch(a, b, stream);
}

// which kernel drag_conv3x3_bf16 takes for M = B * Ho * Wo output pixels: 2 = the persistent 256x256 kernel, 0 = t128 (the convolutions use
// use_t256 alone, not the ring kernels of gemm_choice) — for callers that account launches per kernel
extern "C" int drag_conv3x3_bf16_choice(int64_t M, int Cout, int Cin) { return use_t256(M, 0, Cout, 9 * Cin) ? 2 : 0; }

extern "C" int drag_conv3x3_bf16(const drag_conv_args* a, void* stream) {
  DRAG_CHECK(a != nullptr && a->x && a->w && a->y, "drag_conv3x3_bf16: null pointer");
  DRAG_CHECK(a->B > 0 && a->Ho > 0 && a->Wo > 0 && a->Hp > 0 && a->Wp > 0, "drag_conv3x3_bf16: bad shape");
  DRAG_CHECK(a->Cin % BK == 0, "drag_conv3x3_bf16: Cin must be a multiple of 64 (zero-pad channels)");
  DRAG_CHECK(a->Cout % 4 == 0 && a->ldy % 4 == 0, "drag_conv3x3_bf16: Cout and ldy must be multiples of 4");
  DRAG_CHECK(a->stride == 1 || a->stride == 2, "drag_conv3x3_bf16: stride 1 or 2");
  DRAG_CHECK(a->act == DRAG_ACT_NONE || a->act == DRAG_ACT_GELU_TANH || a->act == DRAG_ACT_SILU || a->act == DRAG_ACT_QUICK_GELU,
             "drag_conv3x3_bf16: fused activation must be none, gelu-tanh, silu or quick-gelu");
  DRAG_CHECK((a->Ho - 1) * a->stride + a->oy + 2 <= a->Hp - 1 && (a->Wo - 1) * a->stride + a->ox + 2 <= a->Wp - 1,
             "drag_conv3x3_bf16: taps leave the padded input");
  GemmKArgs k;
  const long long M = (long long)a->B * a->Ho * a->Wo;
  DRAG_CHECK(M < (1ll << 31), "drag_conv3x3_bf16: too many output pixels");
  fill_common(k, a->x, a->w, a->y, a->bias, nullptr, a->resid, (int)M, a->Cout, 9 * a->Cin, a->ldy, 0, 0,
              0, a->act, 0, 0);
  k.am.rpb = (int)M; k.am.bs = 0; k.am.ld = a->Cin;
  k.cv = ConvMap{a->Ho, a->Wo, a->Hp, a->Wp, a->Cin, a->stride, a->oy, a->ox};
  DRAG_CHECK(((long long)(BM * a->stride + 3 * a->Wp * 2) * a->Cin) * 2 < (1ll << 30), "drag_conv3x3_bf16: tile span too large");
  const KernelRow& row = *kernel_row(drag_conv3x3_bf16_choice(M, a->Cout, a->Cin));
  k.tiles_m = (int)((M + row.tm - 1) / row.tm); k.tiles_n = (a->Cout + row.tn - 1) / row.tn;
  return launch_row(row, FORM_CONV, k, stream);
}
