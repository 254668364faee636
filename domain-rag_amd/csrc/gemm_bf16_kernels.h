// gemm_bf16_kernels.h — what the bf16 GEMM kernels share: the launch arguments, the epilogue code, the tile walk, the LDS read helpers, and
// the declarations of every kernel instantiation the library builds.  Each kernel family is compiled from its own source(s):
// gemm_bf16_t128.hip; gemm_bf16_deep_n128.hip, _n192a.hip, _n192b.hip; gemm_bf16_t256.hip, gemm_bf16_t256_pair.hip; gemm_bf16_w4p.hip.
// gemm_bf16.hip is the host side (tile policy, launch, split-K, the C ABI) and reaches the kernels through the declarations at the end.
// The library is linked without relocatable device code: nothing here may be a device-side global.
//
// Row addressing is "batched rows": logical row r lives at base + (r / rpb) * bs + (r % rpb) * ld,
// which lets the text and image streams of Flux live inside one joint [B, S, D] buffer with no
// concat copies.
#pragma once
#include "drag_common.h"
// The asm statements that write m0 (one s_add_u32 m0 per LDS-DMA piece) list "m0" as a clobber: hipcc then re-materialises m0 before its own
// next LDS-DMA builtin (checked on a two-builtin probe: without the clobber the second builtin ran on the asm's stale m0).  clang warns that m0
// is a reserved register on every such statement; the clobber is what is wanted here.
#pragma clang diagnostic ignored "-Winline-asm"

namespace drag_gemm {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;  // 16 KiB per operand tile

struct RowMap {
  int rpb;        // rows per batch
  long long bs;   // batch stride (elements)
  int ld;         // row stride (elements)
  __device__ __forceinline__ long long off(int r) const {
    int b = r / rpb;
    int s = r - b * rpb;
    return (long long)b * bs + (long long)s * ld;
  }
};

// conv mode (implicit GEMM, 3x3): A is a zero-haloed NHWC activation [B, Hp, Wp, Cin]; logical row
// m = (b, y, x) of the [B*Ho*Wo, 9*Cin] im2col matrix starts at pixel (y*stride + oy, x*stride + ox)
// and K-tile kt = (tap, channel chunk) adds ((tap/3)*Wp + tap%3)*Cin + chunk*64.
struct ConvMap {
  int Ho, Wo, Hp, Wp, Cin, stride, oy, ox;
  __device__ __forceinline__ long long off(int m) const {
    const int hw = Ho * Wo;
    const int b = m / hw;
    const int r = m - b * hw;
    const int y = r / Wo;
    const int x = r - y * Wo;
    return (((long long)b * Hp + y * stride + oy) * Wp + x * stride + ox) * Cin;
  }
};

struct GemmKArgs {
  const bf16_t* A;
  const bf16_t* W;
  void* C;
  const bf16_t* bias;   // [N] or null
  const bf16_t* gate;   // [batch, ldg] or null:  C = resid + gate[b, n] * (acc + bias)
  const bf16_t* resid;  // same row addressing as C, or null
  int M, N, K;
  RowMap am, cm;
  ConvMap cv;
  int ldg;
  int act;
  int act_n0;     // activation applies to columns >= act_n0
  int out_f32;
  unsigned a_bytes, w_bytes;
  int tiles_m, tiles_n;
  int wide;       // C / resid / gate rows are 16-B aligned and N % 8 == 0: staged epilogue
  // optional second destination: output columns >= n_split go to C2 (dense rows of ld2 elements, column n -> C2[n - n_split]).
  // Lets two Linears over the same input run as ONE launch into two buffers (Flux single blocks: to_q|k|v and proj_mlp).
  void* C2;
  int ld2, n_split;
  int group_m;    // M tiles per group of the tile walk (8; "gemm_group_m" option for measurements)
  int ldw;          // W's row stride in elements (= K, except in a split-K launch: the whole K of the Linear)
  long long w_boff; // split-K launch (gemm_bf16_w4p only): what row batch b of A adds to W's base (elements): batch b multiplies columns b K .. b K + K - 1
  int split_m1;     // split-K launch of a PAIR: rows >= split_m1 of every K slice are the second problem's (operands A2 / W2, same row stride); 0: one problem
  int w4_late_state;   // "gemm_epilogue" = 2 (measurement): gemm_bf16_w4p computes tile t + 2's state between tile t's K loop and its epilogue instead of in front of tile t + 1's K loop
  int epi_generic; // "gemm_epilogue" = 1: every tile takes the general staged epilogue (tests compare it with the specialised one bit for bit)
  // optional second row segment (drag_gemm_bf16_pair): M tiles >= seg_tiles_m belong to a second problem with its own operands and
  // row maps but the same N, K and epilogue form — a double block's text and image Linears as ONE launch of the non-persistent kernels
  int seg_tiles_m;          // 0: one segment
  const bf16_t* A2;
  const bf16_t* W2;
  void* Cs2;
  const bf16_t* bias2;
  const bf16_t* gate2;
  const bf16_t* resid2;
  int M2, ldg2, wide2;
  RowMap am2, cm2;
};

// a workgroup whose M tile lies in the second segment swaps that segment's operands in (wave-uniform: scalar moves)
__device__ __forceinline__ void pick_segment(GemmKArgs& p, int& tm) {
  if (p.seg_tiles_m > 0 && tm >= p.seg_tiles_m) {
    tm -= p.seg_tiles_m;
    p.A = p.A2; p.W = p.W2; p.C = p.Cs2; p.bias = p.bias2; p.gate = p.gate2; p.resid = p.resid2;
    p.M = p.M2; p.ldg = p.ldg2; p.wide = p.wide2; p.am = p.am2; p.cm = p.cm2;
  }
}

// the arguments as the epilogue of the tile at column n0 sees them
__device__ __forceinline__ GemmKArgs dest_of(const GemmKArgs& p, int n0) {
  GemmKArgs q = p;
  if (p.C2 != nullptr && n0 >= p.n_split) {
    q.C = (void*)((bf16_t*)p.C2 - p.n_split);
    q.cm.ld = p.ld2;
  }
  return q;
}


// per-column epilogue operands of one 4-wide column group, loaded once per tile column (not once per row)
struct ColOps {
  float b[4];      // bias
  float g[4];      // gate (valid when the tile lies inside one batch)
};
__device__ __forceinline__ void load_colops(const GemmKArgs& p, int n, int bidx, bool gate_uniform, ColOps& c) {
#pragma unroll
  for (int r = 0; r < 4; ++r) { c.b[r] = 0.f; c.g[r] = 0.f; }
  if (n >= p.N) return;
  if (p.bias) {
    const u32x2_t bb = *(const u32x2_t*)(p.bias + n);
    c.b[0] = bf2f((bf16_t)(bb[0] & 0xffff)); c.b[1] = bf2f((bf16_t)(bb[0] >> 16));
    c.b[2] = bf2f((bf16_t)(bb[1] & 0xffff)); c.b[3] = bf2f((bf16_t)(bb[1] >> 16));
  }
  if (p.gate && gate_uniform) {
    const u32x2_t gg = *(const u32x2_t*)(p.gate + (long long)bidx * p.ldg + n);
    c.g[0] = bf2f((bf16_t)(gg[0] & 0xffff)); c.g[1] = bf2f((bf16_t)(gg[0] >> 16));
    c.g[2] = bf2f((bf16_t)(gg[1] & 0xffff)); c.g[3] = bf2f((bf16_t)(gg[1] >> 16));
  }
}

// The fused activations are all  y = x * sigmoid(x * (c0 + c1 x^2)):  GELU-tanh (c0, c1) = (2k, 2k*0.044715),
// SiLU (1, 0), QuickGELU (1.702, 0) -> one branch-free body, tiny code (the epilogue is inlined 32x per lane;
// a switch over libm-style bodies there blew the instruction cache and cost >25 % on K = 3072 GEMMs).
struct ActCoef { float c0, c1; };
__device__ __forceinline__ ActCoef act_coef(int act) {
  switch (act) {
    case DRAG_ACT_GELU_TANH: return {2.0f * 0.7978845608028654f, 2.0f * 0.7978845608028654f * 0.044715f};
    case DRAG_ACT_SILU: return {1.0f, 0.0f};
    case DRAG_ACT_QUICK_GELU: return {1.702f, 0.0f};
    default: return {0.0f, 0.0f};
  }
}

// The activation of four consecutive columns, two values per instruction: the operations of  x * fast_sigmoid(x * (c0 + c1 x x))  in the
// scalar order — (c1 x), fma(.., x, c0), x *, * (-log2 e), 2^, 1 +, 1 /, x * — so the bits are those of the scalar body; the six
// non-transcendental ones become v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32 (the compiler's own vectoriser stops at the v_exp / v_rcp
// pair: 7.5 instructions per value, 5 here; the GELU epilogue of a 256 x 256 tile was 3200 instructions per wave, a tenth of the K = 3072 tile)
__device__ __forceinline__ void act4(float* v, ActCoef ac) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // torch: y = linear(x) is a bf16 tensor before the activation reads it
    const f32x2_t x = {rbf(v[2 * h]), rbf(v[2 * h + 1])};
    const f32x2_t m1 = ac.c1 * x;
    const f32x2_t t = __builtin_elementwise_fma(m1, x, (f32x2_t){ac.c0, ac.c0});
    const f32x2_t z = x * t;
    const f32x2_t a = -1.4426950408889634f * z;
    const f32x2_t e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
    const f32x2_t d = 1.0f + e;
    const f32x2_t r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    const f32x2_t y = x * r;
    v[2 * h] = y[0];
    v[2 * h + 1] = y[1];
  }
}

// epilogue of one accumulator row-group: NI groups of 4 consecutive columns of ONE output row.
// CHECK = false is the interior-tile fast path (no bounds tests, residual loads issued up front).
template <int NI, bool CHECK>
__device__ __forceinline__ void epi_row(const GemmKArgs& p, long long coff, int bidx, int nbase, const f32x4_t* a,
                                        const ColOps* c, bool gate_uniform, ActCoef ac) {
  u32x2_t rr[NI];
  if (p.resid) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = nbase + ni * 16;
      rr[ni] = (u32x2_t){0u, 0u};
      if (!CHECK || n < p.N) rr[ni] = *(const u32x2_t*)(p.resid + coff + n);
    }
  }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = nbase + ni * 16;
    if (CHECK && n >= p.N) continue;
    float v[4] = {a[ni][0] + c[ni].b[0], a[ni][1] + c[ni].b[1], a[ni][2] + c[ni].b[2], a[ni][3] + c[ni].b[3]};
    if (p.act != DRAG_ACT_NONE && n >= p.act_n0) {
      act4(v, ac);
    }
    if (p.gate) {
      // diffusers computes  x = x + gate * y  with y, gate, x bf16 tensors: y is rounded to
      // bf16 first, the product is rounded, then the sum is rounded.
      float g[4] = {c[ni].g[0], c[ni].g[1], c[ni].g[2], c[ni].g[3]};
      if (!gate_uniform) {
        const u32x2_t gg = *(const u32x2_t*)(p.gate + (long long)bidx * p.ldg + n);
        g[0] = bf2f((bf16_t)(gg[0] & 0xffff)); g[1] = bf2f((bf16_t)(gg[0] >> 16));
        g[2] = bf2f((bf16_t)(gg[1] & 0xffff)); g[3] = bf2f((bf16_t)(gg[1] >> 16));
      }
      const float x[4] = {bf2f((bf16_t)(rr[ni][0] & 0xffff)), bf2f((bf16_t)(rr[ni][0] >> 16)),
                          bf2f((bf16_t)(rr[ni][1] & 0xffff)), bf2f((bf16_t)(rr[ni][1] >> 16))};
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = x[r] + rbf(g[r] * rbf(v[r]));
    } else if (p.resid) {
      v[0] = bf2f((bf16_t)(rr[ni][0] & 0xffff)) + rbf(v[0]); v[1] = bf2f((bf16_t)(rr[ni][0] >> 16)) + rbf(v[1]);
      v[2] = bf2f((bf16_t)(rr[ni][1] & 0xffff)) + rbf(v[2]); v[3] = bf2f((bf16_t)(rr[ni][1] >> 16)) + rbf(v[3]);
    }
    if (p.out_f32) {
      *(f32x4_t*)((float*)p.C + coff + n) = (f32x4_t){v[0], v[1], v[2], v[3]};
    } else {
      u32x2_t o;
      o[0] = pack2bf(v[0], v[1]);
      o[1] = pack2bf(v[2], v[3]);
      *(u32x2_t*)((bf16_t*)p.C + coff + n) = o;
    }
  }
}

// whole-wave epilogue: MI row groups x NI column groups; rows m = mrow0 + 16*mi, columns nbase + 16*ni
template <int MI, int TM, int TN = TM, int NI = 4>
__device__ __forceinline__ void wave_epilogue(const GemmKArgs& p, int m0, int mrow0, int n0, int nbase, f32x4_t (*acc)[NI]) {
  const int b_first = m0 / p.cm.rpb;
  const bool gate_uniform = b_first == (min(m0 + TM, p.M) - 1) / p.cm.rpb;     // whole tile inside one batch
  const ActCoef ac = act_coef(p.act);
  ColOps co[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) load_colops(p, nbase + ni * 16, b_first, gate_uniform, co[ni]);
  const bool interior = m0 + TM <= p.M && n0 + TN <= p.N;
  if (interior) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int m = mrow0 + mi * 16;
      epi_row<NI, false>(p, p.cm.off(m), m / p.cm.rpb, nbase, acc[mi], co, gate_uniform, ac);
    }
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int m = mrow0 + mi * 16;
      if (m >= p.M) continue;
      epi_row<NI, true>(p, p.cm.off(m), m / p.cm.rpb, nbase, acc[mi], co, gate_uniform, ac);
    }
  }
}

// ---- staged epilogue (bf16 output, 16-B aligned rows) -------------------------------------------------------------
// Stores are priced per cache line touched per instruction (measured: the fragment-layout epilogue above, 16 rows x
// 32 B per store instruction, cost 9.7 us of a 256x256 tile's ~75 us at K = 3072 — 58 us of a 460 us GEMM — and the
// same with every tile aimed at one L2-resident location, i.e. issue-bound, not HBM-bound).  So each wave transposes
// its 128x64 sub-tile through a private 2 KiB LDS slab, 16 rows (one MFMA row block) at a time:
//   fragment side: v = acc + bias, activation, round to bf16 (every consumer below reads the bf16 value, as torch's
//                  bf16 linear output), ds_write_b64 of 4 columns;
//   row side     : lane (row l>>3 (+8), 16-B chunk l&7) reads 8 consecutive columns back, applies gate / residual
//                  with 16-B loads and stores 16 B: one store instruction = 8 full 128-B lines.
// Slab layout: row r at r*128 B; its 16-B slots are XOR-swizzled with (r & 7) and the 8-B halves of a slot with
// (r >> 3), which makes the 16-lane ds_write_b64 groups and the ds_read_b128 groups bank-conflict free.
__device__ __forceinline__ float bf_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// A wave with more than 4 column blocks (the 192-column tiles of gemm_bf16_deep: NI = 6) runs the slab pass per GROUP of <= 4
// blocks: group (NI0, NIG) covers the wave's columns 16 * NI0 .. 16 * (NI0 + NIG); nw0 is the group's first column.  A group of
// 2 blocks uses the same slab layout with the upper half of its columns (and of the row-side lanes) idle.
template <int MI, int TM, bool CHECK, int NI = 4, int NI0 = 0, int NIG = 4>
__device__ __forceinline__ void staged_rows(const GemmKArgs& p, int m0, int mw0, int n0, int nw0, int l, f32x4_t (*acc)[NI],
                                            char* scr) {
  const int q = l >> 4, r16 = l & 15;
  const int c = l & 7, rl = l >> 3;
  const ActCoef ac = act_coef(p.act);
  const int b_first = m0 / p.cm.rpb;
  const bool one_batch = b_first == (min(m0 + TM, p.M) - 1) / p.cm.rpb;     // whole tile inside one batch
  // fragment side: bias of this lane's 4 columns per column block
  float bias[4][4];
  bool actv[4];
#pragma unroll
  for (int ni = 0; ni < NIG; ++ni) {
    const int n = nw0 + ni * 16 + q * 4;
    bias[ni][0] = bias[ni][1] = bias[ni][2] = bias[ni][3] = 0.f;
    if (p.bias && (!CHECK || n < p.N)) {
      const u32x2_t bb = *(const u32x2_t*)(p.bias + n);
      bias[ni][0] = bf_lo(bb[0]); bias[ni][1] = bf_hi(bb[0]); bias[ni][2] = bf_lo(bb[1]); bias[ni][3] = bf_hi(bb[1]);
    }
    actv[ni] = p.act != DRAG_ACT_NONE && n >= p.act_n0;
  }
  int woff[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    woff[ni] = r16 * 128 + (((2 * ni + (q >> 1)) ^ (r16 & 7)) << 4) + (((q & 1) ^ (r16 >> 3)) << 3);
  const int roff = rl * 128 + ((c ^ rl) << 4);                // + j * 1024; halves swapped for j = 1
  // row side: this lane's 8 columns
  const int n = nw0 + c * 8;
  const bool col_ok = (!CHECK || n + 8 <= p.N) && (NIG == 4 || c * 8 < NIG * 16);   // N % 8 == 0 on this path; a short group's upper lanes idle
  float g[8];
  if (p.gate && one_batch && col_ok) {
    const u32x4_t gg = *(const u32x4_t*)(p.gate + (long long)b_first * p.ldg + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) { g[2 * i] = bf_lo(gg[i]); g[2 * i + 1] = bf_hi(gg[i]); }
  }
  const long long off0 = p.cm.off(min(mw0, p.M - 1));
  // residual rows are requested RD row blocks (passes) ahead of their use into a small register ring: one exposed HBM
  // latency per tile instead of one per pass (the per-pass form cost a gated GEMM 18 % at K = 3072); the whole tile at
  // once (64 VGPRs at MI = 8) pushed the 256x256 kernel into scratch spills inside its main loop
  constexpr int RD = MI < 2 ? MI : 2;
  u32x4_t rres[RD][2];
  auto load_resid = [&](int mi2) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = mw0 + mi2 * 16 + j * 8 + rl;
      rres[mi2 % RD][j] = (u32x4_t){0u, 0u, 0u, 0u};
      if ((CHECK || NIG < 4) && ((CHECK && m >= p.M) || !col_ok)) continue;
      const long long coff = (one_batch ? off0 + (long long)(m - mw0) * p.cm.ld : p.cm.off(m)) + n;
      rres[mi2 % RD][j] = *(const u32x4_t*)(p.resid + coff);
    }
  };
  if (p.resid) {
#pragma unroll
    for (int mi = 0; mi < RD; ++mi) load_resid(mi);
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NIG; ++ni) {
      float v[4] = {acc[mi][NI0 + ni][0] + bias[ni][0], acc[mi][NI0 + ni][1] + bias[ni][1], acc[mi][NI0 + ni][2] + bias[ni][2],
                    acc[mi][NI0 + ni][3] + bias[ni][3]};
      if (actv[ni]) {
        act4(v, ac);
      }
      u32x2_t o;
      o[0] = pack2bf(v[0], v[1]);
      o[1] = pack2bf(v[2], v[3]);
      *(u32x2_t*)(scr + woff[ni]) = o;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = mw0 + mi * 16 + j * 8 + rl;
      u32x4_t y = *(const u32x4_t*)(scr + roff + j * 1024);
      if (j == 1) y = (u32x4_t){y[2], y[3], y[0], y[1]};
      if ((CHECK || NIG < 4) && ((CHECK && m >= p.M) || !col_ok)) continue;
      const long long coff = (one_batch ? off0 + (long long)(m - mw0) * p.cm.ld : p.cm.off(m)) + n;
      if (p.resid) {
        const u32x4_t x = rres[mi % RD][j];
        if (p.gate) {
          // diffusers computes  x = x + gate * y  with y, gate, x bf16 tensors: the product is rounded, then the sum
          if (!one_batch) {
            const u32x4_t gg = *(const u32x4_t*)(p.gate + (long long)(m / p.cm.rpb) * p.ldg + n);
#pragma unroll
            for (int i = 0; i < 4; ++i) { g[2 * i] = bf_lo(gg[i]); g[2 * i + 1] = bf_hi(gg[i]); }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
            y[i] = pack2bf(bf_lo(x[i]) + rbf(g[2 * i] * bf_lo(y[i])), bf_hi(x[i]) + rbf(g[2 * i + 1] * bf_hi(y[i])));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = pack2bf(bf_lo(x[i]) + bf_lo(y[i]), bf_hi(x[i]) + bf_hi(y[i]));
        }
      }
      *(u32x4_t*)((bf16_t*)p.C + coff) = y;
    }
    if (p.resid && mi + RD < MI) load_resid(mi + RD);
  }
}

// Fast form of the staged epilogue for the common tile: interior, inside ONE batch of the output's row map, four column blocks per wave
// that are all alike (activation on all of them or on none).  Same arithmetic, operation for operation, as staged_rows — what goes is
// everything staged_rows decides at run time per row block (residual? gate? which columns are activated? does the tile cross a batch?
// the row map's integer division per store when it does): the ablations of round 4 (profiles/r04_gemm_epilogue_ablations.log) put the
// epilogue at 10 % of a K = 3072 tile with only 1.5-2.6 % of it in the LDS transpose and < 2 % in HBM writes — the rest is its own
// instruction stream.  FORM: 0 = y, 1 = resid + y, 3 = resid + gate * y;  ACT: the activation applies to every column of the tile.
template <int MI, int FORM, bool ACT, int NI = 4, int NI0 = 0>      // NI / NI0: the wave's accumulator row has NI column blocks; this call takes blocks NI0 .. NI0 + 3
__device__ __forceinline__ void staged_rows_fast(const GemmKArgs& p, long long off0, int bidx, int nw0, int l, f32x4_t (*acc)[NI], char* scr) {
  const int q = l >> 4, r16 = l & 15;
  const int c = l & 7, rl = l >> 3;
  const ActCoef ac = act_coef(p.act);
  float bias[4][4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    bias[ni][0] = bias[ni][1] = bias[ni][2] = bias[ni][3] = 0.f;
    if (p.bias) {
      const u32x2_t bb = *(const u32x2_t*)(p.bias + nw0 + ni * 16 + q * 4);
      bias[ni][0] = bf_lo(bb[0]); bias[ni][1] = bf_hi(bb[0]); bias[ni][2] = bf_lo(bb[1]); bias[ni][3] = bf_hi(bb[1]);
    }
  }
  int woff[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    woff[ni] = r16 * 128 + (((2 * ni + (q >> 1)) ^ (r16 & 7)) << 4) + (((q & 1) ^ (r16 >> 3)) << 3);
  const int roff = rl * 128 + ((c ^ rl) << 4);
  const int n = nw0 + c * 8;
  float g[8];
  if constexpr (FORM == 3) {
    const u32x4_t gg = *(const u32x4_t*)(p.gate + (long long)bidx * p.ldg + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) { g[2 * i] = bf_lo(gg[i]); g[2 * i + 1] = bf_hi(gg[i]); }
  }
  // row (mi, j, rl) of the wave's sub-tile lives at off0 + (16 mi + 8 j + rl) * ld: a wave-uniform base per (mi, j) + one 32-bit lane offset
  const unsigned lane_off = (unsigned)(rl * p.cm.ld + n);
  bf16_t* const Cb = (bf16_t*)p.C + off0;
  const bf16_t* const Rb = FORM ? p.resid + off0 : nullptr;
  constexpr int RD = MI < 2 ? MI : 2;
  u32x4_t rres[RD][2];
  auto load_resid = [&](int mi2) {
#pragma unroll
    for (int j = 0; j < 2; ++j) rres[mi2 % RD][j] = *(const u32x4_t*)(Rb + (long long)(mi2 * 16 + j * 8) * p.cm.ld + lane_off);
  };
  if constexpr (FORM != 0) {
#pragma unroll
    for (int mi = 0; mi < RD; ++mi) load_resid(mi);
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float v[4] = {acc[mi][NI0 + ni][0] + bias[ni][0], acc[mi][NI0 + ni][1] + bias[ni][1], acc[mi][NI0 + ni][2] + bias[ni][2],
                    acc[mi][NI0 + ni][3] + bias[ni][3]};
      if constexpr (ACT) {
        act4(v, ac);
      }
      u32x2_t o;
      o[0] = pack2bf(v[0], v[1]);
      o[1] = pack2bf(v[2], v[3]);
      *(u32x2_t*)(scr + woff[ni]) = o;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      u32x4_t y = *(const u32x4_t*)(scr + roff + j * 1024);
      if (j == 1) y = (u32x4_t){y[2], y[3], y[0], y[1]};
      if constexpr (FORM != 0) {
        const u32x4_t x = rres[mi % RD][j];
        if constexpr (FORM == 3) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            y[i] = pack2bf(bf_lo(x[i]) + rbf(g[2 * i] * bf_lo(y[i])), bf_hi(x[i]) + rbf(g[2 * i + 1] * bf_hi(y[i])));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) y[i] = pack2bf(bf_lo(x[i]) + bf_lo(y[i]), bf_hi(x[i]) + bf_hi(y[i]));
        }
      }
      *(u32x4_t*)(Cb + (long long)(mi * 16 + j * 8) * p.cm.ld + lane_off) = y;
    }
    if constexpr (FORM != 0) {
      if (mi + RD < MI) load_resid(mi + RD);
    }
  }
}

// The same for a wave tile of EIGHT column blocks (the 4-wave kernel's 128 x 128): two column groups through two slabs, software-pipelined by
// hand — with one wave per SIMD nothing else covers the LDS round trip of a pass, so the slab writes of the next row block are issued
// between a group's slab reads and its stores.  Operation for operation the arithmetic of staged_rows_fast (same bits).
// EDGE: the wave's rows may end before 128 (a ragged M edge: rows >= rows_valid are neither loaded nor stored) and may cross ONE batch
// boundary of the output's row map (rows >= split belong to the next batch: base `off1 + row * ld` and the next batch's gate vector) — the
// DiT's text stream is 8 batches of 1241 rows, its joint stream 8 of 5337: tiles that straddle a batch are the rule there.  Same
// arithmetic; the interior form carries none of it.
template <int MI, int FORM, bool ACT, bool EDGE = false>
__device__ __forceinline__ void staged_rows_fast8(const GemmKArgs& p, long long off0, int bidx, int nw0, int l, f32x4_t (*acc)[8], char* scr,
                                                  int rows_valid = 1 << 30, int split = 1 << 30, long long off1 = 0) {
  const int q = l >> 4, r16 = l & 15;
  const int c = l & 7, rl = l >> 3;
  const ActCoef ac = act_coef(p.act);
  float bias[2][4][4];
#pragma unroll
  for (int grp = 0; grp < 2; ++grp)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      bias[grp][ni][0] = bias[grp][ni][1] = bias[grp][ni][2] = bias[grp][ni][3] = 0.f;
      if (p.bias) {
        const u32x2_t bb = *(const u32x2_t*)(p.bias + nw0 + 64 * grp + ni * 16 + q * 4);
        bias[grp][ni][0] = bf_lo(bb[0]); bias[grp][ni][1] = bf_hi(bb[0]); bias[grp][ni][2] = bf_lo(bb[1]); bias[grp][ni][3] = bf_hi(bb[1]);
      }
    }
  int woff[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    woff[ni] = r16 * 128 + (((2 * ni + (q >> 1)) ^ (r16 & 7)) << 4) + (((q & 1) ^ (r16 >> 3)) << 3);
  const int roff = rl * 128 + ((c ^ rl) << 4);
  const int n = nw0 + c * 8;
  u32x4_t gq[2][2];                // gate words [batch side][group] (EDGE: both sides of the batch boundary)
  if constexpr (FORM == 3) {
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      gq[0][grp] = *(const u32x4_t*)(p.gate + (long long)bidx * p.ldg + n + 64 * grp);
      if constexpr (EDGE) gq[1][grp] = split < rows_valid && split < 128 ? *(const u32x4_t*)(p.gate + (long long)(bidx + 1) * p.ldg + n + 64 * grp) : gq[0][grp];
    }
  }
  const unsigned lane_off = (unsigned)(rl * p.cm.ld + n);
  const long long d01 = off1 - off0;         // EDGE: what a row past the boundary adds to its address (elements; >= 0: batches ascend)
  bf16_t* const Cb = (bf16_t*)p.C + off0;
  const bf16_t* const Rb = FORM ? p.resid + off0 : nullptr;
  // EDGE: the row predicate is the DESCRIPTOR's bound, not a branch (64 predicated loads / stores split the straight-line code into as
  // many basic blocks with spills between them: the first version ran as slowly as the general epilogue): accesses at or past the first
  // invalid row's byte offset are dropped / return zero by the load-store unit
  __amdgpu_buffer_rsrc_t rsC, rsR;
  unsigned d01b = 0;
  if constexpr (EDGE) {
    // (the bound is the first invalid row's FIRST byte in this wave's column range: a destination whose base is shifted — the second
    //  buffer of a two-destination launch is addressed from C2 - n_split — has valid columns beyond row_start + ld)
    const long long end = rows_valid >= 128 ? (1ll << 31) - 16 : ((long long)rows_valid * p.cm.ld + nw0 + (rows_valid > split ? d01 : 0ll)) * 2;
    rsC = __builtin_amdgcn_make_buffer_rsrc((void*)Cb, 0, (unsigned)end, 0x00020000);
    rsR = __builtin_amdgcn_make_buffer_rsrc((void*)(FORM ? Rb : (const bf16_t*)Cb), 0, (unsigned)end, 0x00020000);
    d01b = (unsigned)(d01 * 2);
  }
  constexpr int RD = 2;
  u32x4_t rres[RD][2][2];          // [ring][group][j]
  auto load_resid = [&](int mi2) {
#pragma unroll
    for (int grp = 0; grp < 2; ++grp)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = mi2 * 16 + j * 8 + rl;
        if constexpr (EDGE) {
          const unsigned vo = (unsigned)(((mi2 * 16 + j * 8) * p.cm.ld + lane_off + 64 * grp) * 2) + (r >= split ? d01b : 0u);
          rres[mi2 % RD][grp][j] = __builtin_amdgcn_raw_buffer_load_b128(rsR, (int)vo, 0, 0);
        } else {
          rres[mi2 % RD][grp][j] = *(const u32x4_t*)(Rb + (long long)(mi2 * 16 + j * 8) * p.cm.ld + lane_off + 64 * grp);
        }
      }
  };
  auto slab_values = [&](int mi, int grp, u32x2_t* o) {      // the arithmetic of one slab (registers only)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float v[4] = {acc[mi][4 * grp + ni][0] + bias[grp][ni][0], acc[mi][4 * grp + ni][1] + bias[grp][ni][1],
                    acc[mi][4 * grp + ni][2] + bias[grp][ni][2], acc[mi][4 * grp + ni][3] + bias[grp][ni][3]};
      if constexpr (ACT) {
        act4(v, ac);
      }
      o[ni][0] = pack2bf(v[0], v[1]);
      o[ni][1] = pack2bf(v[2], v[3]);
    }
  };
  auto slab_store = [&](int grp, const u32x2_t* o) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) *(u32x2_t*)(scr + grp * 2048 + woff[ni]) = o[ni];
  };
  auto write_slab = [&](int mi, int grp) {
    u32x2_t o[4];
    slab_values(mi, grp, o);
    slab_store(grp, o);
  };
  if constexpr (FORM != 0) {
#pragma unroll
    for (int mi = 0; mi < RD; ++mi) load_resid(mi);
  }
  write_slab(0, 0);
  write_slab(0, 1);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      u32x4_t y[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        y[j] = *(const u32x4_t*)(scr + grp * 2048 + roff + j * 1024);
      }
      // The slab's two reads are ISSUED; the next row block's arithmetic runs under their latency, and its writes to the same slab follow
      // without a wait: the LDS operations of a wave execute in issue order, so a write issued behind a read cannot overtake it.  (Round 5
      // measured the form that waited for the reads first — 16 exposed LDS round trips per tile, 7300 cycles for 707 instructions.)
      __builtin_amdgcn_sched_barrier(0);
      if (mi + 1 < MI) {
        u32x2_t o[4];
        slab_values(mi + 1, grp, o);
        __builtin_amdgcn_sched_barrier(0);
        slab_store(grp, o);
      }
      __builtin_amdgcn_sched_barrier(0);
      y[1] = (u32x4_t){y[1][2], y[1][3], y[1][0], y[1][1]};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = mi * 16 + j * 8 + rl;
        if constexpr (FORM != 0) {
          const u32x4_t x = rres[mi % RD][grp][j];
          if constexpr (FORM == 3) {
            u32x4_t gw = gq[0][grp];
            if constexpr (EDGE) gw = r >= split ? gq[1][grp] : gq[0][grp];
#pragma unroll
            for (int i = 0; i < 4; ++i)
              y[j][i] = pack2bf(bf_lo(x[i]) + rbf(bf_lo(gw[i]) * bf_lo(y[j][i])), bf_hi(x[i]) + rbf(bf_hi(gw[i]) * bf_hi(y[j][i])));
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) y[j][i] = pack2bf(bf_lo(x[i]) + bf_lo(y[j][i]), bf_hi(x[i]) + bf_hi(y[j][i]));
          }
        }
        if constexpr (EDGE) {
          const unsigned vo = (unsigned)(((mi * 16 + j * 8) * p.cm.ld + lane_off + 64 * grp) * 2) + (r >= split ? d01b : 0u);
          __builtin_amdgcn_raw_buffer_store_b128(y[j], rsC, (int)vo, 0, 0);
        } else {
          *(u32x4_t*)(Cb + (long long)(mi * 16 + j * 8) * p.cm.ld + lane_off + 64 * grp) = y[j];
        }
      }
    }
    if constexpr (FORM != 0) {
      if (mi + RD < MI) load_resid(mi + RD);
    }
  }
}

template <int MI, int TM, int TN = TM, int NI = 4>      // returns true when the tile took the specialised form (a fixed number of stores per wave)
__device__ __forceinline__ bool staged_epilogue(const GemmKArgs& p, int m0, int mw0, int n0, int nw0, int l, f32x4_t (*acc)[NI],
                                                char* scr) {
  constexpr int G0 = NI < 4 ? NI : 4;
  if constexpr (NI == 4 || NI == 8) {
    const int b_first = m0 / p.cm.rpb;
    const bool fast = m0 + TM <= p.M && n0 + TN <= p.N && b_first == (m0 + TM - 1) / p.cm.rpb && (long long)8 * p.cm.ld + p.N < (1ll << 31);
    const bool act_none = p.act == DRAG_ACT_NONE || p.act_n0 >= n0 + TN, act_all = p.act != DRAG_ACT_NONE && p.act_n0 <= n0;
    if (fast && !p.epi_generic && (act_none || (act_all && !p.resid)) && !(p.gate && !p.resid)) {
      const long long off0 = p.cm.off(mw0);
      // (NI = 8, the 4-wave kernel's 128-column wave tile: two column groups of four blocks through the same slab, one after the other)
#define DRAG_FAST(FORM_, ACT_)                                                                              \
  do {                                                                                                      \
    if constexpr (NI == 8) staged_rows_fast8<MI, FORM_, ACT_>(p, off0, b_first, nw0, l, acc, scr);          \
    else staged_rows_fast<MI, FORM_, ACT_, NI, 0>(p, off0, b_first, nw0, l, acc, scr);                      \
  } while (0)
      if (!p.resid) {
        if (act_none) DRAG_FAST(0, false);
        else DRAG_FAST(0, true);
      } else if (p.gate) DRAG_FAST(3, false);
      else DRAG_FAST(1, false);
#undef DRAG_FAST
      return true;
    }
    if constexpr (NI == 8) {
      // full columns, but a ragged M edge and / or ONE batch boundary of the row map inside the tile (batches of >= 256 rows): the
      // straight-line form with a row predicate and a per-row choice between the two batches' bases / gate vectors
      const long long jump = p.cm.rpb < p.M ? p.cm.bs - (long long)p.cm.rpb * p.cm.ld : 0;      // what crossing a batch adds to a row's offset
      const bool edge = n0 + TN <= p.N && p.cm.rpb >= TM && p.cm.ld >= TN / 2 && jump >= 0 && ((long long)(TM / 2 + 8) * p.cm.ld + p.N + jump) * 2 < (1ll << 31) - 16;
      if (edge && !p.epi_generic && (act_none || (act_all && !p.resid)) && !(p.gate && !p.resid)) {
        const int rows_valid = p.M - mw0;
        if (rows_valid > 0) {
          const int bA = mw0 / p.cm.rpb;                              // the batch of the wave's first row
          const int split = (bA + 1) * p.cm.rpb - mw0;                 // local row where the next batch starts (>= 128: not in this wave)
          const long long off0 = p.cm.off(mw0);
          const long long off1 = split < 128 && mw0 + split < p.M ? p.cm.off(mw0 + split) - (long long)split * p.cm.ld : off0;
          if (!p.resid) {
            if (act_none) staged_rows_fast8<MI, 0, false, true>(p, off0, bA, nw0, l, acc, scr, rows_valid, split, off1);
            else staged_rows_fast8<MI, 0, true, true>(p, off0, bA, nw0, l, acc, scr, rows_valid, split, off1);
          } else if (p.gate) staged_rows_fast8<MI, 3, false, true>(p, off0, bA, nw0, l, acc, scr, rows_valid, split, off1);
          else staged_rows_fast8<MI, 1, false, true>(p, off0, bA, nw0, l, acc, scr, rows_valid, split, off1);
        }
        return m0 + TM <= p.M;          // every row stored: 32 stores per wave, as in the interior form
      }
    }
  }
  if (m0 + TM <= p.M && n0 + TN <= p.N) {
    staged_rows<MI, TM, false, NI, 0, G0>(p, m0, mw0, n0, nw0, l, acc, scr);
    if constexpr (NI > 4) staged_rows<MI, TM, false, NI, 4, NI - 4>(p, m0, mw0, n0, nw0 + 64, l, acc, scr);
  } else {
    staged_rows<MI, TM, true, NI, 0, G0>(p, m0, mw0, n0, nw0, l, acc, scr);
    if constexpr (NI > 4) staged_rows<MI, TM, true, NI, 4, NI - 4>(p, m0, mw0, n0, nw0 + 64, l, acc, scr);
  }
  return false;
}

// tile selection shared by both kernels: XCD-contiguous, grouped along M for L2 reuse of the W panel
__device__ __forceinline__ void pick_tile(const GemmKArgs& p, int bid, int& tm, int& tn) {
  const int nwg = p.tiles_m * p.tiles_n;
  const int wg = xcd_remap(bid, nwg);
  const int GROUP_M = p.group_m;
  const int in_group = GROUP_M * p.tiles_n;
  const int gid = wg / in_group;
  const int first_m = gid * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int rem = wg - gid * in_group;
  tm = first_m + rem % gsz;
  tn = rem / gsz;
}

// one ds_read_b128 the compiler does not see (no automatic s_waitcnt: the caller counts), N of them 2 KiB apart from BASE
template <int OFF>
__device__ __forceinline__ void lds_read_b128(bf16x8_t& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int N, int BASE, int I = 0>
__device__ __forceinline__ void lds_read_frags(bf16x8_t* f, unsigned addr) {
  if constexpr (I < N) {
    lds_read_b128<BASE + I * 2048>(f[I], addr);
    lds_read_frags<N, BASE, I + 1>(f, addr);
  }
}

// ---- the kernels: one definition each, in the source named; every other object reaches them through these declarations ----
template <int MODE>  // 0: batched rows, 1: conv3x3 implicit GEMM
__global__ __launch_bounds__(256, 2) void gemm_bf16_t128(GemmKArgs p);                        // gemm_bf16_t128.hip
extern template __global__ void gemm_bf16_t128<0>(GemmKArgs);
extern template __global__ void gemm_bf16_t128<1>(GemmKArgs);

template <int MI, int ST, int NI>
__global__ __launch_bounds__(256, 2) void gemm_bf16_deep(GemmKArgs p);                        // gemm_bf16_deep.h, instantiated in:
// The ring forms X(MI, ST, NI), one list per instantiating source (three sources: the compile time is balanced between them).  The lists
// are the only place a form is written: from them come the declarations below, each source's instantiations (DRAG_GEMM_DEEP_DEFINE) and
// the host's table rows (gemm_bf16.hip), where a form's code is 100 * (NI == 6) + 10 * MI + ST.
#define DRAG_GEMM_DEEP_N128(X) X(4, 2, 4) X(4, 3, 4) X(3, 2, 4) X(3, 3, 4) X(2, 2, 4) X(2, 3, 4) X(2, 4, 4) X(1, 3, 4) X(1, 4, 4)      // gemm_bf16_deep_n128.hip
#define DRAG_GEMM_DEEP_N192A(X) X(1, 3, 6) X(2, 3, 6) X(3, 3, 6) X(4, 3, 6)                                                            // gemm_bf16_deep_n192a.hip
#define DRAG_GEMM_DEEP_N192B(X) X(3, 2, 6) X(4, 2, 6) X(3, 4, 6) X(4, 4, 6)                                                            // gemm_bf16_deep_n192b.hip
#define DRAG_GEMM_DEEP_DEFINE(MI_, ST_, NI_) template __global__ void gemm_bf16_deep<MI_, ST_, NI_>(GemmKArgs);
#define DRAG_GEMM_DEEP_EXTERN(MI_, ST_, NI_) extern DRAG_GEMM_DEEP_DEFINE(MI_, ST_, NI_)
DRAG_GEMM_DEEP_N128(DRAG_GEMM_DEEP_EXTERN)
DRAG_GEMM_DEEP_N192A(DRAG_GEMM_DEEP_EXTERN)
DRAG_GEMM_DEEP_N192B(DRAG_GEMM_DEEP_EXTERN)
#undef DRAG_GEMM_DEEP_EXTERN

template <int MODE>
__global__ __launch_bounds__(512, 2) void gemm_bf16_t256(GemmKArgs p);                        // gemm_bf16_t256.h, instantiated in gemm_bf16_t256.hip
extern template __global__ void gemm_bf16_t256<0>(GemmKArgs);
extern template __global__ void gemm_bf16_t256<1>(GemmKArgs);
__global__ __launch_bounds__(512, 2) void gemm_bf16_t256_pair(GemmKArgs p);                   // gemm_bf16_t256_pair.hip

__global__ __launch_bounds__(256, 1) void gemm_bf16_w4p(GemmKArgs p);                         // gemm_bf16_w4p.hip
#if DRAG_EXP
template <int V>
__global__ __launch_bounds__(256, 1) void gemm_bf16_w4(GemmKArgs p);
#define DRAG_GEMM_W4_VARIANTS(X) X(0) X(1) X(2) X(3) X(4) X(5)      // "gemm_kernel" = 400 + V
#define DRAG_GEMM_W4_DEFINE(V_) template __global__ void gemm_bf16_w4<V_>(GemmKArgs);
#define DRAG_GEMM_W4_EXTERN(V_) extern DRAG_GEMM_W4_DEFINE(V_)
DRAG_GEMM_W4_VARIANTS(DRAG_GEMM_W4_EXTERN)
#undef DRAG_GEMM_W4_EXTERN
#endif

}  // namespace drag_gemm
