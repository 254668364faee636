// gemm_bf16_w4p.hip — the 4-wave 256x256x64 kernels whose K loop is generated asm text (gemm4w_kloop.h): gemm_bf16_w4p, the product kernel
// of the large Linears, and, in experiment builds, its non-persistent ancestors gemm_bf16_w4<V> with the stamp buffer of gemm_bf16_w4p.
#include "gemm_bf16_kernels.h"

namespace drag_gemm {

// --------------------------------------------------------------------------------------------
// gemm_bf16_w4 (round 5; EXPERIMENT, DRAG_EXPERIMENTS builds only: "gemm_kernel" = 400 + V) — the 256x256x64 tile as FOUR waves x (128 x 128),
// one wave per SIMD with the whole register file (256 accumulators in AGPRs): a third less LDS -> register traffic per flop than the
// 8-wave kernel below, the shape of the vendor library's kernel on this chip.  hipcc cannot schedule a 512-register wave
// (gemm_bf16_deep<8, 2, 8>: waterfall loops around every LDS-DMA, 168 v_accvgpr moves per K-step), so the K loop is ONE asm statement whose
// text scripts/gen/gemm4w_kloop.py generates (register map and schedule there); the kernel binds its operands to the physical registers
// the text names.  Plain tiles (not persistent), K a multiple of 128.  Bit-identical to every other GEMM kernel here.
// MEASURED (profiles/r05_gemm_w4_*.log; us per K-step and tile round, the 8-wave kernel 1.45-1.49 on the same boxes): V1 = refill by
// LDS-DMA 1.50-1.53, V0 = refill through registers (every chunk a full K-step in flight) 1.58; ablations: no refill 1.12-1.15 (= 2048
// MFMA cycles at 96 %: the MFMA + fragment-read skeleton is fine), no barrier -0.07...-0.16, every chunk from an L2-resident K-step 1.26.
// So 0.3 us of a K-step is the operand stream pushing back on the ISSUE of a lone wave's loads (not latency: a K-step of flight per chunk
// does not help) — exactly what the 8-wave kernel's second wave group hides.  Not the product kernel.
// --------------------------------------------------------------------------------------------
#include "gemm4w_kloop.h"
typedef __attribute__((ext_vector_type(32))) float f32x32_t;
typedef __attribute__((ext_vector_type(8))) uint32_t u32x8_t;

#if DRAG_EXP
template <int V>
__global__ __launch_bounds__(256, 1) void gemm_bf16_w4(GemmKArgs p) {
  constexpr int A_BYTES = 256 * 128, STAGE = 2 * A_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // 2 * STAGE = 128 KiB
  const int w = wave_id();
  const int l = lane_id();
  const int wr = w >> 1, wc = w & 1;
  int tm, tn;
  pick_tile(p, (int)blockIdx.x, tm, tn);
  pick_segment(p, tm);
  const int m0 = tm * 256, n0 = tn * 256;
  const long long a0 = p.am.off(m0);
  const int wrows = min(256, p.N - n0);
  // descriptors as four dwords each (base, base_hi, num_records, flags): operands of the asm statement
  const unsigned long long pa = (unsigned long long)(uintptr_t)(p.A + a0), pw = (unsigned long long)(uintptr_t)(p.W + (long long)n0 * p.K);
  auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };      // wave-uniform by construction: say so
  // bounded: the register form requests up to one K-step past K in its last iterations (zeros / the next row's start, never used)
  const long long a_span = (p.am.off(min(m0 + 255, p.M - 1)) - a0 + p.K) * 2;
  const u32x4_t rsA = {uni((uint32_t)pa), uni((uint32_t)(pa >> 32) & 0xffffu), uni((uint32_t)a_span), 0x00020000u};
  const u32x4_t rsW = {uni((uint32_t)pw), uni((uint32_t)(pw >> 32) & 0xffffu), uni((uint32_t)((long long)wrows * p.K * 2)), 0x00020000u};
  u32x8_t voA, voW;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (w * 8 + i) * 8 + (l >> 3);
    const int slot = (l & 7) ^ ((row >> 1) & 7);
    const int ra = min(m0 + row, p.M - 1);                 // clamp: rows past the edge are never stored
    voA[i] = (unsigned)((p.am.off(ra) - a0 + slot * 8) * 2);
    const int rw = min(row, wrows - 1);
    voW[i] = (unsigned)(((long long)rw * p.K + slot * 8) * 2);
  }
  const unsigned lds0 = (unsigned)(size_t)(DRAG_LDS char*)smem;
  const unsigned ldsw = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + (unsigned)w * 8192u));
  const int p0 = (l >> 4) ^ ((l & 15) >> 1);
  const int fa = (wr * 128 + (l & 15)) * 128;
  const int fb = A_BYTES + (wc * 128 + (l & 15)) * 128;
  u32x8_t rd;      // [buffer][X k-half 0, X k-half 1, W k-half 0, W k-half 1]
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      rd[4 * b + ks] = lds0 + (unsigned)(b * STAGE + fa + ((p0 ^ (ks * 4)) << 4));
      rd[4 * b + 2 + ks] = lds0 + (unsigned)(b * STAGE + fb + ((p0 ^ (ks * 4)) << 4));
    }
  f32x32_t accrow[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 32; ++r) accrow[i][r] = 0.f;
  unsigned n2 = (unsigned)(p.K / 128 - 1);       // pairs of K-steps in the steady loop; the last pair is the tail
  unsigned soff = 0;
  // prologue: K-steps 0 and 1 into the two stage buffers, then K-step 0 visible to every wave
  const u32x2_t wrv = {lds0 + (unsigned)(w * 8192 + l * 16), lds0 + (unsigned)(STAGE + w * 8192 + l * 16)};
#define G4W_OUTS                                                                                                                              \
  "+{a[0:31]}"(accrow[0]), "+{a[32:63]}"(accrow[1]), "+{a[64:95]}"(accrow[2]), "+{a[96:127]}"(accrow[3]), "+{a[128:159]}"(accrow[4]),        \
      "+{a[160:191]}"(accrow[5]), "+{a[192:223]}"(accrow[6]), "+{a[224:255]}"(accrow[7]), [n2] "+s"(n2), [soff] "+s"(soff)
#define G4W_INS "{v[128:135]}"(voA), "{v[136:143]}"(voW), "{v[144:151]}"(rd), [rsa] "s"(rsA), [rsw] "s"(rsW), [ldsw] "s"(ldsw)
  if constexpr (V == 1) {          // form D: refill by LDS-DMA
    asm volatile(G4W_D_STAGE0 G4W_FIRST_READS G4W_D_LOOP G4W_D_TAIL : G4W_OUTS : G4W_INS : G4W_CLOBBERS, "scc", "memory");
  } else if constexpr (V == 2) {   // form D2: LDS-DMA, two barriers per K-step, the refill spread from the first barrier on
    asm volatile(G4W_D_STAGE0 G4W_FIRST_READS G4W_D2_LOOP G4W_D_TAIL : G4W_OUTS : G4W_INS : G4W_CLOBBERS, "scc", "memory");
  } else if constexpr (V == 3) {
    asm volatile(G4W_D_STAGE0 G4W_FIRST_READS G4W_D2_LOOP_A G4W_D_TAIL : G4W_OUTS : G4W_INS : G4W_CLOBBERS, "scc", "memory");
  } else if constexpr (V == 4) {
    asm volatile(G4W_D_STAGE0 G4W_FIRST_READS G4W_D2_LOOP_B G4W_D_TAIL : G4W_OUTS : G4W_INS : G4W_CLOBBERS, "scc", "memory");
  } else if constexpr (V == 5) {
    asm volatile(G4W_D_STAGE0 G4W_FIRST_READS G4W_D2_LOOP_C G4W_D_TAIL : G4W_OUTS : G4W_INS : G4W_CLOBBERS, "scc", "memory");
  } else {                         // form R: refill through registers
    asm volatile(G4W_R_STAGE0 G4W_FIRST_READS G4W_R_LOOP G4W_R_TAIL : G4W_OUTS : G4W_INS, "{v[152:153]}"(wrv) : G4W_CLOBBERS_R, "scc", "memory");
  }
#undef G4W_OUTS
#undef G4W_INS
  f32x4_t acc[8][8];
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 8; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = accrow[mi][4 * ni + r];
  const GemmKArgs pd = dest_of(p, n0);
  if (p.wide) {
    __syncthreads();                              // the slabs alias the stage buffers
    staged_epilogue<8, 256, 256, 8>(pd, m0, m0 + wr * 128, n0, n0 + wc * 128, l, acc, smem + w * 4096);
  } else {
    wave_epilogue<8, 256, 256, 8>(pd, m0, m0 + wr * 128 + (l & 15), n0, n0 + wc * 128 + (l >> 4) * 4, acc);
  }
}

#endif

// gemm_bf16_w4p — PRODUCT kernel of the large Linears since round 5: the persistent form of gemm_bf16_w4 (form D2 of the K loop): one workgroup per CU walks tiles b, b + P, ... (all on its
// XCD); a tile is ONE asm statement (K-steps 0 and 1 already staged, steady loop, a tail whose two K-steps stage K-steps 0 and 1 of the
// workgroup's next tile), then the C++ epilogue on slabs that do not alias the stage buffers — so the epilogue overlaps the next tile's
// loads.  K a multiple of 128; batched rows / two destinations / every epilogue form like gemm_bf16_t256<0>; no conv mode, no pair.
typedef __attribute__((ext_vector_type(16))) uint32_t u32x16_t;
struct W4Tile {
  u32x4_t rsA, rsW;
  u32x16_t vo;      // [0:7] X chunks, [8:15] W chunks
  int m0, n0;       // the tile's first row / column (wave-uniform, in SGPRs: the epilogue of the tile reuses them instead of walking again)
};
// An INTERIOR tile inside one batch of the row map has offsets row * ld (no clamp, no division); edge tiles and tiles that cross a batch
// take the general form
__device__ __forceinline__ void w4_tile_state(const GemmKArgs& p, int tile, int w, int l, bool valid, W4Tile& t) {
  auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  int tm, tn;
  pick_tile(p, tile, tm, tn);
  const int m0 = __builtin_amdgcn_readfirstlane(tm * 256), n0 = __builtin_amdgcn_readfirstlane(tn * 256);
  t.m0 = m0;
  t.n0 = n0;
  long long a0 = p.am.off(m0);
  const int wrows = min(256, p.N - n0);
  const bf16_t *Ab = p.A, *Wb = p.W;
  if (p.w_boff) {                            // split-K: row batch = K slice; in a pair's launch the rows behind split_m1 are the second problem's
    const int sl = m0 / p.am.rpb, r = m0 - sl * p.am.rpb;
    Wb += (long long)sl * p.w_boff;
    if (p.split_m1 > 0 && r >= p.split_m1) {
      Ab = p.A2; Wb = p.W2 + (long long)sl * p.w_boff;
      a0 = (long long)sl * p.am.bs + (long long)(r - p.split_m1) * p.am.ld;
    }
  }
  const unsigned long long pa = (unsigned long long)(uintptr_t)(Ab + a0), pw = (unsigned long long)(uintptr_t)(Wb + (long long)n0 * p.ldw);
  const bool interior = m0 + 256 <= p.M && wrows == 256 && m0 / p.am.rpb == (m0 + 255) / p.am.rpb;
  const long long a_span = interior ? ((long long)255 * p.am.ld + p.K) * 2 : (p.am.off(min(m0 + 255, p.M - 1)) - a0 + p.K) * 2;
  // no next tile: descriptors with zero records — the tail's loads return zeros without touching memory
  t.rsA = (u32x4_t){uni((uint32_t)pa), uni((uint32_t)(pa >> 32) & 0xffffu), valid ? uni((uint32_t)a_span) : 0u, 0x00020000u};
  t.rsW = (u32x4_t){uni((uint32_t)pw), uni((uint32_t)(pw >> 32) & 0xffffu), valid ? uni((uint32_t)(((long long)(wrows - 1) * p.ldw + p.K) * 2)) : 0u, 0x00020000u};
  if (interior) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = (w * 8 + i) * 8 + (l >> 3);
      const int slot = (l & 7) ^ ((row >> 1) & 7);
      t.vo[i] = (unsigned)((row * p.am.ld + slot * 8) * 2);
      t.vo[8 + i] = (unsigned)((row * p.ldw + slot * 8) * 2);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = (w * 8 + i) * 8 + (l >> 3);
    const int slot = (l & 7) ^ ((row >> 1) & 7);
    const int ra = min(m0 + row, p.M - 1);                 // clamp: rows past the edge are never stored
    t.vo[i] = (unsigned)((p.am.off(ra) - a0 + slot * 8) * 2);
    const int rw = min(row, wrows - 1);
    t.vo[8 + i] = (unsigned)(((long long)rw * p.ldw + slot * 8) * 2);
  }
}

#if DRAG_EXP
// experiment builds: shader-clock stamps of workgroup 0 / wave 0 around the pieces of a tile (drag_debug_w4_stamps copies them out)
namespace {      // internal linkage: a device global exists in this object only
__device__ unsigned long long g_w4_stamps[8 * 64];
}
#define W4_STAMP(slot)                                                                                   \
  do {                                                                                                   \
    if (blockIdx.x == 0 && w == 0 && l == 0 && tile_no < 64) g_w4_stamps[tile_no * 8 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define W4_STAMP(slot) do { } while (0)
#endif

__global__ __launch_bounds__(256, 1) void gemm_bf16_w4p(GemmKArgs p) {
  constexpr int A_BYTES = 256 * 128, STAGE = 2 * A_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // 2 * STAGE + 4 x 2 epilogue slabs of 2 KiB
  const int w = wave_id();
  const int l = lane_id();
  const int wr = w >> 1, wc = w & 1;
  const int P = (int)gridDim.x;
  const int nwg = p.tiles_m * p.tiles_n;
  int vb = (int)blockIdx.x;
  const unsigned lds0 = (unsigned)(size_t)(DRAG_LDS char*)smem;
  const unsigned ldsw = (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + (unsigned)w * 8192u));
  // Per-lane constants are RECOMPUTED from a laundered lane id in every tile (a handful of VALU instructions): hoisted out of the tile loop
  // they are live across the K loop's statement, which leaves the compiler 88 free VGPRs (v0-v127 clobbered, v128-v151 / v224-v239 bound) —
  // it spilled them to scratch, and every reload is an s_waitcnt vmcnt(0) that drains the previous epilogue's 32 stores before the next K
  // loop may start (stamps: 2800 cycles of "tile state" per tile, all of it that wait)
  auto lane_now = [&]() { int v = l; asm volatile("" : "+v"(v)); return v; };
  // the same for the divisors of the tile walk and the row maps: the reciprocals of wave-uniform divisions are computed by the VALU, and
  // hoisted they sit in VGPRs across the statement
  auto args_now = [&]() {
    GemmKArgs q = p;
    asm volatile("" : "+s"(q.tiles_n), "+s"(q.tiles_m), "+s"(q.group_m), "+s"(q.am.rpb), "+s"(q.cm.rpb), "+s"(q.M), "+s"(q.K), "+s"(q.am.ld), "+s"(q.cm.ld), "+s"(q.ldw));
    return q;
  };
  auto read_addrs = [&](int lv) {      // [buffer][X k-half 0, X k-half 1, W k-half 0, W k-half 1]
    const int p0 = (lv >> 4) ^ ((lv & 15) >> 1);
    const int fa = (wr * 128 + (lv & 15)) * 128;
    const int fb = A_BYTES + (wc * 128 + (lv & 15)) * 128;
    u32x8_t rd;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        rd[4 * b + ks] = lds0 + (unsigned)(b * STAGE + fa + ((p0 ^ (ks * 4)) << 4));
        rd[4 * b + 2 + ks] = lds0 + (unsigned)(b * STAGE + fb + ((p0 ^ (ks * 4)) << 4));
      }
    return rd;
  };
  W4Tile cur, nxt;
  w4_tile_state(p, vb, w, lane_now(), true, cur);
  unsigned soff = 0;
  // the workgroup's first tile: K-steps 0 and 1 into the two stage buffers (every later tile finds them staged by its predecessor's tail)
  asm volatile(G4W_D_STAGE0_NOWAIT : [soff] "+s"(soff)
               : "{v[128:143]}"(cur.vo), [rsa] "s"(cur.rsA), [rsw] "s"(cur.rsW), [ldsw] "s"(ldsw) : "scc", "m0", "memory");
  int stores_behind = 0;
  [[maybe_unused]] int tile_no = 0;
  const bool late = DRAG_EXP && p.w4_late_state != 0;      // (experiment builds only: the product kernel must not carry the variant's 64 B of scratch)
  if (late) w4_tile_state(args_now(), vb + P < nwg ? vb + P : vb, w, lane_now(), vb + P < nwg, nxt);
  for (;;) {
    W4_STAMP(0);
    const bool have_next = vb + P < nwg;
    const int lt = lane_now();
    if (!late) w4_tile_state(args_now(), have_next ? vb + P : vb, w, lt, have_next, nxt);
    const u32x8_t rd = read_addrs(lt);
    W4_STAMP(1);
    // K-steps 0 and 1 of this tile landed (this wave's pieces; the statement below opens with the barrier).  Behind an interior tile's fast
    // epilogue exactly 32 stores are younger than those pieces (VMEM operations of a wave retire in issue order): they may stay in flight
    if (stores_behind == 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    W4_STAMP(2);
    f32x32_t accrow[8];                            // written by the statement (the first K-step's MFMAs start from the constant 0)
    unsigned n2 = (unsigned)(p.K / 128 - 2);       // pairs of K-steps in the steady loop: all but the first pair and the tail
    asm volatile(G4W_P_FIRST G4W_P_PAIR0 G4W_P_LOOP G4W_P_TAIL
                 : "={a[0:31]}"(accrow[0]), "={a[32:63]}"(accrow[1]), "={a[64:95]}"(accrow[2]), "={a[96:127]}"(accrow[3]),
                   "={a[128:159]}"(accrow[4]), "={a[160:191]}"(accrow[5]), "={a[192:223]}"(accrow[6]), "={a[224:255]}"(accrow[7]),
                   [n2] "+s"(n2), [soff] "+s"(soff)
                 : "{v[128:143]}"(cur.vo), "{v[224:239]}"(nxt.vo), "{v[144:151]}"(rd), [rsa] "s"(cur.rsA), [rsw] "s"(cur.rsW),
                   [rsa2] "s"(nxt.rsA), [rsw2] "s"(nxt.rsW), [ldsw] "s"(ldsw)
                 : G4W_CLOBBERS, "scc", "memory");
    W4_STAMP(3);
    W4Tile nn;
    if (late) {            // (measurement) the state of the tile after next, in front of this tile's epilogue
      const bool have2 = vb + 2 * P < nwg;
      w4_tile_state(args_now(), have2 ? vb + 2 * P : vb, w, lane_now(), have2, nn);
    }
    const int le = lane_now();
    f32x4_t acc[8][8];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
      for (int ni = 0; ni < 8; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = accrow[mi][4 * ni + r];
    const GemmKArgs pe = args_now();
    const int m0 = cur.m0, n0 = cur.n0;
    const GemmKArgs pd = dest_of(pe, n0);
    bool fast = false;
    if (pd.wide) fast = staged_epilogue<8, 256, 256, 8>(pd, m0, m0 + wr * 128, n0, n0 + wc * 128, le, acc, smem + 2 * STAGE + w * 4096);
    else wave_epilogue<8, 256, 256, 8>(pd, m0, m0 + wr * 128 + (le & 15), n0, n0 + wc * 128 + (le >> 4) * 4, acc);
    stores_behind = fast ? 32 : 0;
    W4_STAMP(4);
    ++tile_no;
    if (!have_next) break;
    cur = nxt;
    if (late) nxt = nn;
    vb += P;
  }
}

#if DRAG_EXP
DRAG_GEMM_W4_VARIANTS(DRAG_GEMM_W4_DEFINE)
#endif

}  // namespace drag_gemm

#if DRAG_EXP
// (hipMemcpyFromSymbol resolves a device global in the object that defines it: the library is linked without relocatable device code)
extern "C" int drag_debug_w4_stamps(unsigned long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(drag_gemm::g_w4_stamps), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
