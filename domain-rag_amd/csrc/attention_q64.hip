// attention_q64.hip — attention_q64_kernel, the 64-query kernel whose KV loop is a hand-placed stream of asm statements, with its stamp buffer
// (experiment builds).
#include "attn_q64_common.h"

namespace drag_attn {

// --------------------------------------------------------------------------------------------
// attention_q64_kernel — 4 waves x 64 queries, ONE wave per SIMD with the whole 512-entry register file: the kernel of the long
// sequences (S >= 4096: the DiT's joint attention) since round 4.
// Each wave owns two 32-query groups and runs both against every K / V^T fragment it reads, which halves the LDS fragment
// reads per flop.  Same arithmetic per query group, same deferred-rescale decisions (taken per group), so the outputs equal the 8-wave
// kernel's bit for bit (test_attention_schedules_are_bit_identical).  Why it wins (profiles/r04_pmc_attention_8wave_vs_q64_hand_placed.txt,
// B = 8, S = 5337, isolated, one --pmc pass): both kernels keep the matrix pipe busy 61-62 % of the time, but the chip — power-limited in
// attention — gives the 8-wave kernel 1.61 GHz and this one 1.82 GHz: half the LDS traffic (SQ_LDS_IDX_ACTIVE 185 M vs 360 M per launch)
// is the difference.  Round 2's form of it (hipcc's instruction order) kept the pipe busy 42 % of the time and lost (0.86 x); the KV loop
// below is a hand-placed instruction stream (see `body`).  1200-1208 vs 1148-1158 TFLOP/s isolated, 2410 vs 2533 us for the DiT's call with the
// fused q preparation, +0.7 % on the whole composite batch (profiles/r04_attention_q64_*.log).
// --------------------------------------------------------------------------------------------
// MFMAs of the 64-query kernel are inline asm so that the operand FILES are fixed: O accumulators and the Q fragments live
// in the AGPR half (only MFMAs touch them), the S accumulators in arch VGPRs (the softmax reads them).  With builtins hipcc
// puts S into AGPRs as well and copies 200-400 registers per KV tile back and forth (measured: 473-668 v_accvgpr / scratch
// instructions per 64 MFMAs).  hipcc neither counts nor pads what is inside an asm statement (guide 5.7):
//   * a VALU-written A / B operand needs 2 wait states before the MFMA reads it — the packed P words are a step old when their P V MFMA
//     issues, but hipcc may also RESTORE an operand it parked (v_accvgpr_read) in the instruction right before an asm statement: the step
//     statements open with two softmax instructions for that reason, and scripts/check_asm_loads.py checks every MFMA of the compiled kernel;
//   * an MFMA result needs 18 wait states (16-pass op) before anything but the next MFMA of its chain touches it: Q64_SETTLE
//     passes the registers through a nop statement before compiler-generated code may read them.
#define Q64_MFMA_S0(d, a, b) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(d) : "v"(a), "a"(b))
#define Q64_MFMA_S(d, a, b) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(b))
#define Q64_SETTLE_S(s4) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(s4[0][0]), "+v"(s4[0][1]), "+v"(s4[1][0]), "+v"(s4[1][1]))
#define Q64_SETTLE_O(o, qg) asm volatile("s_nop 15\n\ts_nop 7" : "+a"(o[qg][0]), "+a"(o[qg][1]), "+a"(o[qg][2]), "+a"(o[qg][3]))

// pieces of the hand-placed stream (round 4) that are single statements: hipcc neither moves them against each other nor waits for them
template <int OFF>
__device__ __forceinline__ void q64_lds_read(bf16x8_t& d, unsigned addr) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF)); }
// the wait that retires asm-issued fragment reads names the fragments as in/out operands: whatever the compiler does with a fragment (a
// copy to split its live range, a v_accvgpr_write to park it) then depends on the WAIT, not on the read — a copy of the read's own result
// can be scheduled straight behind the ds_read, in front of the next asm statement, before the LDS has written the registers (asm volatile
// orders asm statements, not the compiler's instructions around them)
template <int N>
__device__ __forceinline__ void q64_landed(bf16x8_t& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N)); }
template <int N>
__device__ __forceinline__ void q64_landed(bf16x8_t& a, bf16x8_t& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N)); }
template <int N>
__device__ __forceinline__ void q64_landed(bf16x8_t& a, bf16x8_t& b, bf16x8_t& c, bf16x8_t& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
__device__ __forceinline__ void q64_max3(float& d, float a, float b, float c) { asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); }
// P V: the packed P words were written >= one step (dozens of instructions) before: no VALU -> MFMA wait states to pad
#define Q64P_MFMA_O(d, a, pw) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(d) : "v"(a), "v"(pw))
// A step of the stream as TWO asm statements (the LDS-DMA piece of the step, which is compiler code, sits between them).  hipcc cannot see
// into an asm statement, so whenever a statement reads a register that an earlier STATEMENT wrote and no instruction of its own has been
// issued since, its hazard recogniser pads with an s_nop (asm statements count as zero wait states): with one instruction per statement the
// softmax chain fma -> exp -> add -> cvt cost six s_nop per step, an eighth of the wave's issue slots.  Inside a statement nothing is padded
// and nothing needs to be: every v_exp result has one instruction between it and its first non-transcendental reader (the one software
// hazard of this stream on gfx950), the packed P words an MFMA reads were written a step or more before.
// softmax of two elements per query group (a: group 0, b: group 1), in place: y = s c - m c ; y = 2^y ; ps += y0 + y1 ; w = bf16x2(y0, y1)
#define Q64_V1 "v_fma_f32 %[ya0], %[sa0], %[c], %[nma]\n\t"
#define Q64_V2 "v_fma_f32 %[ya1], %[sa1], %[c], %[nma]\n\t"
#define Q64_V3 "v_exp_f32 %[ya0], %[ya0]\n\t"
#define Q64_V4 "v_fma_f32 %[yb0], %[sb0], %[c], %[nmb]\n\t"
#define Q64_V5 "v_exp_f32 %[ya1], %[ya1]\n\t"
#define Q64_V6 "v_fma_f32 %[yb1], %[sb1], %[c], %[nmb]\n\t"
#define Q64_V7 "v_add_f32 %[ta], %[ya0], %[ya1]\n\t"
#define Q64_V8 "v_exp_f32 %[yb0], %[yb0]\n\t"
#define Q64_V9 "v_add_f32 %[psa], %[psa], %[ta]\n\t"
#define Q64_V10 "v_exp_f32 %[yb1], %[yb1]\n\t"
#define Q64_V11 "v_cvt_pk_bf16_f32 %[wa], %[ya0], %[ya1]\n\t"
#define Q64_V12 "v_add_f32 %[tb], %[yb0], %[yb1]\n\t"
#define Q64_V13 "v_add_f32 %[psb], %[psb], %[tb]\n\t"
#define Q64_V14 "v_cvt_pk_bf16_f32 %[wb], %[yb0], %[yb1]"
#define Q64_SC_IN(sc, T, E0) [sa0] "v"(sc[0][T][E0]), [sa1] "v"(sc[0][T][E0 + 1]), [sb0] "v"(sc[1][T][E0]), [sb1] "v"(sc[1][T][E0 + 1])
// Every statement that holds an MFMA opens with two VALU instructions of the softmax (or more): hipcc may restore a parked operand (a K / V^T
// fragment or packed P word it kept in AGPRs across the rescale branch: v_accvgpr_read) in the instruction right before the statement, and an
// MFMA reads a VALU-written operand correctly only two wait states later — a hazard hipcc pads for its own MFMAs, not for one inside asm.
// steps 4..15, first half: wait | V1 V2 | P V (group 0) | read | V3 | P V (group 1) | read | V4-V6 | S (group 0).  C0 = "0" opens a key half
#define Q64_STEP_HI_A(C0, S0CONS, N, o0_, o1_, vf_, p0_, p1_, s0_, kf_, q0_, d1_, a1_, F1, d2_, a2_, F2, sc, T, E0, cc, nma_, nmb_)        \
  asm volatile("s_waitcnt lgkmcnt(%[n])\n\t" Q64_V1 Q64_V2                                                                                \
               "v_mfma_f32_32x32x16_bf16 %[o0], %[vf], %[p0], %[o0]\n\t"                                                                  \
               "ds_read_b128 %[d1], %[a1] offset:%[f1]\n\t" Q64_V3                                                                        \
               "v_mfma_f32_32x32x16_bf16 %[o1], %[vf], %[p1], %[o1]\n\t"                                                                  \
               "ds_read_b128 %[d2], %[a2] offset:%[f2]\n\t" Q64_V4 Q64_V5 Q64_V6                                                          \
               "v_mfma_f32_32x32x16_bf16 %[s0], %[kf], %[q0], " C0                                                                        \
               : [o0] "+a"(o0_), [o1] "+a"(o1_), [s0] S0CONS(s0_), [d1] "=&v"(d1_), [d2] "=&v"(d2_), [ya0] "=&v"(yA0), [ya1] "=&v"(yA1),  \
                 [yb0] "=&v"(yB0), [yb1] "=&v"(yB1)                                                                                       \
               : [n] "n"(N), [vf] "v"(vf_), [p0] "v"(p0_), [p1] "v"(p1_), [kf] "v"(kf_), [q0] "a"(q0_), [a1] "v"(a1_), [f1] "n"(F1),      \
                 [a2] "v"(a2_), [f2] "n"(F2), Q64_SC_IN(sc, T, E0), [c] "s"(cc), [nma] "v"(nma_), [nmb] "v"(nmb_))
// steps 4..15, second half: V7-V10 | S (group 1) | V11-V14
#define Q64_STEP_HI_B(C1, S1CONS, s1_, kf_, q1_)                                                                                          \
  asm volatile(Q64_V7 Q64_V8 Q64_V9 Q64_V10 "v_mfma_f32_32x32x16_bf16 %[s1], %[kf], %[q1], " C1 "\n\t" Q64_V11 Q64_V12 Q64_V13 Q64_V14    \
               : [s1] S1CONS(s1_), [yb0] "+v"(yB0), [yb1] "+v"(yB1), [psa] "+v"(ps[0]), [psb] "+v"(ps[1]), [wa] "=&v"(wA),                \
                 [wb] "=&v"(wB), [ta] "=&v"(sA), [tb] "=&v"(sB)                                                                           \
               : [kf] "v"(kf_), [q1] "a"(q1_), [ya0] "v"(yA0), [ya1] "v"(yA1))
// steps 0..3 (no P V yet), first half: [wait] | V1 V2 | S (group 0) | read [| read] | V3-V7 | S (group 1)
#define Q64_STEP_LO_A(WAIT, READ2, C0, C1, SCONS, N, s0_, s1_, kf_, q0_, q1_, d1_, a1_, F1, d2_, a2_, F2, sc, T, E0, cc, nma_, nmb_)       \
  asm volatile(WAIT Q64_V1 Q64_V2 "v_mfma_f32_32x32x16_bf16 %[s0], %[kf], %[q0], " C0 "\n\t"                                              \
               "ds_read_b128 %[d1], %[a1] offset:%[f1]\n\t" READ2 Q64_V3 Q64_V4 Q64_V5 Q64_V6 Q64_V7                                      \
               "v_mfma_f32_32x32x16_bf16 %[s1], %[kf], %[q1], " C1                                                                        \
               : [s0] SCONS(s0_), [s1] SCONS(s1_), [d1] "=&v"(d1_), [d2] "=&v"(d2_), [ya0] "=&v"(yA0), [ya1] "=&v"(yA1), [yb0] "=&v"(yB0),\
                 [yb1] "=&v"(yB1), [ta] "=&v"(sA)                                                                                         \
               : [n] "n"(N), [kf] "v"(kf_), [q0] "a"(q0_), [q1] "a"(q1_), [a1] "v"(a1_), [f1] "n"(F1), [a2] "v"(a2_), [f2] "n"(F2),       \
                 Q64_SC_IN(sc, T, E0), [c] "s"(cc), [nma] "v"(nma_), [nmb] "v"(nmb_))
// steps 0..3, second half: V8-V14 (the K fragment stays an operand: its registers are not the compiler's to reuse for the LDS-DMA address
// arithmetic between the two halves while the MFMA that closed the first half is a few cycles old)
#define Q64_STEP_LO_B(kf_)                                                                                                                \
  asm volatile(Q64_V8 Q64_V9 Q64_V10 Q64_V11 Q64_V12 Q64_V13 Q64_V14                                                                      \
               : [yb0] "+v"(yB0), [yb1] "+v"(yB1), [psa] "+v"(ps[0]), [psb] "+v"(ps[1]), [wa] "=&v"(wA), [wb] "=&v"(wB), [tb] "=&v"(sB)   \
               : [ya0] "v"(yA0), [ya1] "v"(yA1), [ta] "v"(sA), "v"(kf_))
template <class F, int G = 0>
__device__ __forceinline__ void q64_unroll16(F&& f) {
  if constexpr (G < 16) {
    f(std::integral_constant<int, G>{});
    q64_unroll16<F, G + 1>(f);
  }
}

#if DRAG_EXP
// experiment builds: shader-clock stamps of workgroup 0 / wave 0: [0] kernel start, [1] before the KV loop, then per tile [2 + 2 it] the wave
// reaches the tile's vmcnt(0) + barrier, [3 + 2 it] it is past them; [2 + 2 nkv] loop done, [3 + 2 nkv] kernel end
namespace {      // internal linkage: a device global exists in this object only
__device__ unsigned long long g_attn_stamps[512];
}
#define ATTN_STAMP(slot)                                                                                                  \
  do {                                                                                                                     \
    if (blockIdx.x == 0 && w == 0 && l == 0 && (slot) < 512) g_attn_stamps[(slot)] = __builtin_amdgcn_s_memtime();         \
  } while (0)
#else
#define ATTN_STAMP(slot) do { } while (0)
#endif
template <bool QPREP>
__global__ __launch_bounds__(256, 1) void attention_q64_kernel(AttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];      // 2 K tiles | 2 V^T tiles | 4 x 16 KiB of q rows on their way to registers
  const int w = wave_id(), l = lane_id();
  ATTN_STAMP(0);
  const int hh = l >> 5;
  constexpr int QB = 256, CPW = 4;
  const int nqb = (p.S + QB - 1) / QB;
  // An ITEM is a (batch, head) and a block of 256 queries: item & 7 = the XCD (heads 8 g + xcd share an L2), item >> 3 = (group, query block).
  // A grid of p.items workgroups runs one item each; a smaller grid (a multiple of 8: one workgroup per CU) walks items i, i + grid, ... —
  // all on the workgroup's XCD — and the KV stream of an item's last two tiles stages the NEXT item's K(0), K(1), V(0) where it would
  // stage tiles that do not exist, the next item's q rows are requested before this item's output is stored: with one workgroup per CU
  // (512 registers per wave) nothing else overlaps an item's seam — 6.5 % of an 84-tile item (profiles/r05_attn_q64_stamps.log)
  // (decode and the two descriptors stay written out here: as q64_decode / q64_k_descr / q64_v_descr of attn_q64_common.h, which
  //  attention_q64g_kernel uses, they change this kernel's SGPR spills and the branches of the peeled tiles)
  using Item = Q64Item;
  auto decode = [&](int item, Item& t) -> bool {
    const int xcd = item & 7, loc = item >> 3;
    const int bh = (loc / nqb) * 8 + xcd;
    t.b = bh / p.H;
    t.h = bh - t.b * p.H;
    t.q0 = (loc - (loc / nqb) * nqb) * QB + w * 64;              // group qg: queries q0 + 32 qg + (l & 31)
    return bh < p.B * p.H;
  };
  int item = (int)blockIdx.x;
  Item cur;
  if (!decode(item, cur)) return;      // (grids smaller than p.items are launched only when B * H is a multiple of 8: every item exists)

  bf16x8_t qf[2][8];
  auto k_descr = [&](const Item& t) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + (long long)t.b * p.qk_bs + t.h * 128), 0, p.k_bytes, 0x00020000);
  };
  auto v_descr = [&](const Item& t) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(p.vt + ((long long)(t.b * p.H + t.h) * 128) * p.s_pad), 0, p.vt_bytes, 0x00020000);
  };
  // the descriptors the LDS-DMA pieces go through, and what is subtracted from a piece's key index: in an item's last two tiles they are
  // switched to the NEXT item's K (from tile nkv - 2 on) and V^T (tile nkv - 1) with s_pad subtracted — K(nkv), K(nkv + 1), V(nkv) become
  // the next item's K(0), K(1), V(0), in the buffers where its prologue and first tile look for them (nkv even)
  __amdgpu_buffer_rsrc_t rsK = k_descr(cur), rsV = v_descr(cur);
  int ksub = 0, vsub = 0;
  unsigned koff[4], voff[4];      // (K / V^T staging offsets: q64_stage_offsets)
#pragma unroll
  for (int i = 0; i < 4; ++i) q64_stage_offsets(p, w, l, i, koff[i], voff[i]);
  auto stage_k1 = [&](int buf, int kv0, int i) {
    const int c = w * CPW + i;
    const unsigned ko = koff[i] + (unsigned)(kv0 - ksub) * (unsigned)(p.ld_qk * 2);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, (DRAG_LDS void*)((DRAG_LDS char*)smem + buf * KT_BYTES + c * 1024), 16, ko, 0, 0, 0);
  };
  auto stage_v1 = [&](int buf, int kv0, int i) {
    const int c = w * CPW + i;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (DRAG_LDS void*)((DRAG_LDS char*)smem + 2 * KT_BYTES + buf * VT_BYTES + c * 1024),
                                             16, voff[i], (kv0 - vsub) * 2, 0, 0);
  };
  const int krd = (l & 31) * 256, kx = l & 15;
  const int vrd = (l & 31) * 128, vx = ((l & 31) >> 1) & 7;
  int ak[8], av[4];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) ak[ks] = krd + (((2 * ks + hh) ^ kx) << 4);
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) av[s2] = vrd + (((2 * s2 + hh) ^ vx) << 4);
  // LDS byte addresses of this lane's K / V^T fragment slots: one register each, added once (inside the steps hipcc re-derived them per read)
  const unsigned lds0 = (unsigned)(size_t)(DRAG_LDS char*)smem;
  unsigned akl[8], avl[4];
  {
#pragma unroll
    for (int i = 0; i < 8; ++i) akl[i] = lds0 + (unsigned)ak[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) avl[i] = lds0 + (unsigned)av[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(akl[i]));
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(avl[i]));
  }

  const int nkv = p.s_pad / 64;
  const bool paired = (nkv & 1) == 0 && nkv >= 4;      // the last two tiles are peeled bodies that stage for the next item (buffer parities line up)
  const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto stage_first = [&]() {       // K(0), V(0), K(1) of the item rsK / rsV name
#pragma unroll
    for (int i = 0; i < 4; ++i) stage_k1(0, 0, i);
#pragma unroll
    for (int i = 0; i < 4; ++i) stage_v1(0, 0, i);
    if (nkv > 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) stage_k1(1, 64, i);
    }
  };
  // Q load in two parts: the rows are REQUESTED (q64_request) and turned into fragments later (q_fragments)
  DRAG_LDS char* const qlds = (DRAG_LDS char*)smem + 2 * KT_BYTES + 2 * VT_BYTES + w * 16384;
  auto q_fragments = [&](const Item& t, const int ll) {       // (the wave's own pieces: behind its s_waitcnt vmcnt(0), no barrier)
    const int hh = ll >> 5;
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      u32x4_t raw[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) raw[ks] = *(const DRAG_LDS u32x4_t*)(qlds + (qg * 8 + ks) * 1024 + ll * 16);
      if constexpr (!QPREP) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[qg][ks] = __builtin_bit_cast(bf16x8_t, raw[ks]);
      } else {
        const int qr = min(t.q0 + 32 * qg + (ll & 31), p.S - 1);
        u32x4_t o[8];
        q_norm_rope<false>(p, raw, qr, hh, [&](int ks, int j, uint32_t word) { o[ks][j] = word; });
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[qg][ks] = __builtin_bit_cast(bf16x8_t, o[ks]);
      }
    }
  };
  stage_first();
  q64_request(p, qlds, cur, l);               // while those tiles are in flight
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  q_fragments(cur, l);
  // From here on the Q fragments exist ONLY in the AGPR half: the tied operand makes hipcc copy each fragment into an AGPR
  // tuple once; a fragment that merely gets "a"-constrained at its uses stays in VGPRs and is re-copied before every use
  // (64 v_accvgpr_write per KV tile and 64 VGPRs gone).  The next item's fragments go there as soon as they exist (the AGPR half has
  // room beside the output accumulators; 64 more live VGPRs across the epilogue were spilled)
  bf16x8_t qa[2][8];
  auto q_to_agprs = [&]() {
#pragma unroll
    for (int qg = 0; qg < 2; ++qg)
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) asm volatile("; q fragment -> AGPR" : "=a"(qa[qg][ks]) : "0"(qf[qg][ks]));
  };
  q_to_agprs();
  bool staged = true;              // K(0), V(0), K(1) of the item at hand are in the LDS (or on their way)
  int stores_behind = 0;           // (q64_wait_older_than_stores)
  for (;;) {                       // items of this workgroup
  ATTN_STAMP(4 + 2 * (p.s_pad / 64));
  const int b = cur.b, h = cur.h, q0 = cur.q0;
  const bool has_next = item + (int)gridDim.x < p.items;
  if (!staged) {                   // (an odd number of tiles: no peeled bodies staged for this item)
    __syncthreads();               // every wave is done with the previous item's tiles
    stage_first();
    stores_behind = 0;             // (these pieces are YOUNGER than the previous item's stores: the wait below has to cover everything)
  }
  f32x16_t oacc[2][4];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[qg][i][r] = 0.f;
  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  q64_wait_older_than_stores(stores_behind);                  // K(0), V(0), K(1) landed
  __syncthreads();
  f32x16_t scur[2][2], snext[2][2];          // [query group][key half]
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8_t kf = *(const bf16x8_t*)(smem + ((akl[ks] - lds0) + t * (32 * 256)));
#pragma unroll
      for (int qg = 0; qg < 2; ++qg) {
        if (ks == 0) Q64_MFMA_S0(scur[qg][t], kf, qa[qg][ks]);
        else Q64_MFMA_S(scur[qg][t], kf, qa[qg][ks]);
      }
    }
  Q64_SETTLE_S(scur);
  auto mask_and_max = [&](f32x16_t (&sx)[2], const int kvs) -> float {
    if (kvs + 64 > p.S) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kvs + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh;
          if (key >= p.S) sx[t][r] = -INFINITY;
        }
    }
    float m = sx[0][0];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, sx[t][r]);
    return fmaxf(m, __shfl_xor(m, 32, 64));
  };
  float mt_carry[2];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) mt_carry[qg] = mask_and_max(scur[qg], 0);

  // ---- round 4: the KV loop as a HAND-PLACED instruction stream.  One wave per SIMD issues in order: two MFMAs back to back stall the wave
  // for the 28 cycles the first one still occupies the pipe, and nothing behind them issues — the round-2 form of this loop (hipcc's order
  // between sched_barriers: PV PV reads QK QK, then the step's 18 VALU as one block) kept the pipe busy 42 % of the time (PMC).  Here every
  // MFMA is followed by its share of the step's other work — at most 5 single-issue instructions per gap, what a lone wave hides behind
  // a 32-cycle MFMA: the step's 14 softmax VALU in a hazard-free order (a transcendental's input / result is never produced / consumed by
  // the neighbouring instruction), the two fragment reads of step g + 2 (the reads run TWO steps ahead: nobody else covers a lone wave's
  // LDS latency) and one LDS-DMA piece.  Everything is `asm volatile`: hipcc keeps the order and inserts no waits; lgkmcnt is counted by hand.
  // Same arithmetic per query group as before: same bits as the 8-wave kernel.
  // The last key group's P V (8 MFMAs on fragments and P words already in registers) and the row maxima of the tile that follows are
  // one block at the TOP of the next iteration: behind the barrier, with the first K fragment reads of the new tile already issued, the
  // eight MFMAs cover both the reads' latency and the 32 v_max3 of the two row-maximum trees (4 per gap).
  bf16x8_t vtr[4];              // the four V^T fragments of the trailing P V MFMAs (read in steps 14 / 15, used after the next barrier)
  u32x4_t pk[2][4];             // packed P: key group kg of a tile is consumed in its steps 4 kg + 4 .. 4 kg + 7, group 3 after the next barrier
  // knext / vnext: the K / V^T pieces of this tile's stream are the NEXT item's (the item's last two tiles, whose own pieces would be tiles
  // that do not exist): K(0) into buffer 0 from tile nkv - 2, K(1) into buffer 1 and V(0) into buffer 0 from tile nkv - 1
  auto body = [&](const int it, auto par, f32x16_t (&sc)[2][2], f32x16_t (&sn)[2][2], auto firstc) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool FIRST = decltype(firstc)::value;
    if constexpr (!FIRST) {
      if (paired && it >= nkv - 2) {                 // (two scalar compares per tile; the switch itself once per item)
        Item nx;
        const bool have = has_next && decode(item + (int)gridDim.x, nx);
        if (PAR == 0) {
          rsK = have ? k_descr(nx) : __builtin_amdgcn_make_buffer_rsrc((void*)p.k, 0, 0, 0x00020000);    // (no next item: zero records, the pieces stage zeros)
          ksub = p.s_pad;
        } else {
          rsV = have ? v_descr(nx) : __builtin_amdgcn_make_buffer_rsrc((void*)p.vt, 0, 0, 0x00020000);
          vsub = p.s_pad;
        }
      }
    }
    constexpr int KN = ((PAR + 1) & 1) * KT_BYTES;
    constexpr int VB = 2 * KT_BYTES + PAR * VT_BYTES;
    const int kv0 = it * 64;
#if DRAG_EXP
    const unsigned long long t_reach = __builtin_amdgcn_s_memtime();      // (stored behind the barrier: a store here would be waited for by the vmcnt(0))
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#if DRAG_EXP
    if (blockIdx.x == 0 && w == 0 && l == 0 && 3 + 2 * it < 512) {
      g_attn_stamps[2 + 2 * it] = t_reach;
      g_attn_stamps[3 + 2 * it] = __builtin_amdgcn_s_memtime();
    }
#endif
    bf16x8_t kfr[3], vfr[3];      // fragment rings (step g uses slot g % 3)
    // RULE of this kernel: a fragment requested by an asm ds_read reaches compiler-visible code only through q64_landed (the s_waitcnt
    // that retires it, with the fragment as an in/out operand), and between the read and that wait there are asm statements only.  hipcc
    // takes the read's destination for defined the moment the statement ends: a build that kept K(0) / K(1) in flight across the rescale
    // branch below had them parked in AGPRs one instruction after the request (v_accvgpr_write of registers the LDS had not written yet:
    // NaNs that came and went with register allocation).  scripts/check_asm_loads.py walks the compiled kernel for exactly that
    // (tests/test_asm_load_discipline.py).
    // K(0), K(1) of the next tile first: their latency hides behind the trailing P V block, which is asm only; they have landed before
    // the compiler's code (maxima across lane halves, rescale decision) begins
    q64_lds_read<KN>(kfr[0], akl[0]);
    q64_lds_read<KN>(kfr[1], akl[1]);
    if constexpr (FIRST) q64_landed<0>(kfr[0], kfr[1]);
    if constexpr (!FIRST) {
      // row maxima of sc (32 scores per lane and query group) as two v_max3 trees: 10 + 4 + 2 instructions each, group A and B interleaved
      float ta[10], tb[10], ua[4], ub[4], ra, rb;
      auto el = [&](int qg, int i) -> float { return sc[qg][i >> 4][i & 15]; };
      auto L1 = [&](float* t, int qg, int i) { q64_max3(t[i], el(qg, 3 * i), el(qg, 3 * i + 1), el(qg, 3 * i + 2)); };
      auto L2 = [&](float* u, const float* t, int qg, int i) {
        if (i < 3) q64_max3(u[i], t[3 * i], t[3 * i + 1], t[3 * i + 2]);
        else q64_max3(u[3], t[9], el(qg, 30), el(qg, 31));
      };
#define Q64P_T(dt, qg) Q64P_MFMA_O(oacc[qg][dt], vtr[dt], pk[qg][3])
      // six v_max3 behind each of the first five MFMAs (what a lone wave hides behind 32 cycles); the joining of the lane halves behind the
      // last three: the other 32 keys of a query live in lane ^ 32, v_permlane32_swap pairs the halves of both groups (no LDS round trip: a
      // ds_bpermute here waits out the K fragment reads already in flight).  swap(ra, rb) = ((ra.lo | rb.lo), (ra.hi | rb.hi)): lanes < 32 then
      // hold group A's two halves of query l, lanes >= 32 group B's of query l - 32; their maximum, swapped with itself, is group A's value in
      // both halves of the first result and group B's in the second.  (The swap needs two wait states after the VALU write of its operands:
      // the MFMA between and one s_nop.)
      // As asm: hipcc (ROCm 7.2) folds fmaxf(sw[0], sw[1]) of __builtin_amdgcn_permlane32_swap's two results to sw[0], and the two results
      // of swap(x, x) to one value (the optimised IR holds a single extractvalue): the maxima then covered the keys of ONE lane half — every
      // parity test passed (any reference value below the true maximum gives the same softmax until 2^(max - reference) overflows) and a key 128
      // octaves above its row's running maximum gave NaN.  scripts/probe/dbg_attn_rescale*.py; test_attention_hot_key_in_every_lane_half.
      Q64P_T(0, 0); L1(ta, 0, 0); L1(ta, 0, 1); L1(ta, 0, 2); L1(ta, 0, 3); L1(ta, 0, 4); L1(ta, 0, 5);
      Q64P_T(0, 1); L1(ta, 0, 6); L1(ta, 0, 7); L1(ta, 0, 8); L1(ta, 0, 9); L1(tb, 1, 0); L1(tb, 1, 1);
      Q64P_T(1, 0); L1(tb, 1, 2); L1(tb, 1, 3); L1(tb, 1, 4); L1(tb, 1, 5); L1(tb, 1, 6); L1(tb, 1, 7);
      Q64P_T(1, 1); L1(tb, 1, 8); L1(tb, 1, 9); L2(ua, ta, 0, 0); L2(ua, ta, 0, 1); L2(ua, ta, 0, 2); L2(ua, ta, 0, 3);
      Q64P_T(2, 0); L2(ub, tb, 1, 0); L2(ub, tb, 1, 1); L2(ub, tb, 1, 2); L2(ub, tb, 1, 3); q64_max3(ra, ua[0], ua[1], ua[2]); q64_max3(rb, ub[0], ub[1], ub[2]);
      asm volatile("v_max_f32 %0, %0, %2\n\tv_max_f32 %1, %1, %3" : "+v"(ra), "+v"(rb) : "v"(ua[3]), "v"(ub[3]));
      Q64P_T(2, 1);
      asm volatile("s_nop 0\n\tv_permlane32_swap_b32 %0, %1\n\tv_max_f32 %0, %0, %1\n\tv_mov_b32 %1, %0" : "+v"(ra), "+v"(rb));
      Q64P_T(3, 0);
      asm volatile("s_nop 0\n\tv_permlane32_swap_b32 %0, %1" : "+v"(ra), "+v"(rb));
      Q64P_T(3, 1);
#undef Q64P_T
      q64_landed<0>(kfr[0], kfr[1]);
      mt_carry[0] = ra;                                     // group A's maximum in both lane halves
      mt_carry[1] = rb;                                     // group B's
      if (kv0 + 64 > p.S) {       // the ragged last tile: keys >= S do not exist (the trees above saw them) — once per (batch, head, query block)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) mt_carry[qg] = mask_and_max(sc[qg], kv0);
      }
    }
    float nmc[2];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      const float mt = mt_carry[qg];
      if (!__all((mt - m_run[qg]) * p.c <= DEFER_THR)) {
        Q64_SETTLE_O(oacc, qg);
        const float m_new = fmaxf(m_run[qg], mt);
        const float alpha = __builtin_amdgcn_exp2f((m_run[qg] - m_new) * p.c);
        l_run[qg] *= alpha;
        m_run[qg] = m_new;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[qg][i][r] *= alpha;
      }
      nmc[qg] = -(m_run[qg] * p.c);
    }
    float ps[2] = {0.f, 0.f};
    // one step; G is a compile-time constant (ring slots, immediate offsets, which pieces exist)
    auto step = [&](auto gc) {
      constexpr int G = decltype(gc)::value;
      constexpr int T = G >> 3, E0 = (2 * G) & 15;
      // reads issued in step s (in order): K(s+2) if s+2 <= 15; V(s+2) if 4 <= s+2 <= 15; the 4 trailing fragments in steps 14 / 15
      constexpr int prev = G - 1;
      // the step's wait: K(G) (and V(G)) landed; step G-1's reads stay in flight
      constexpr int younger = prev < 0 ? 0 : ((prev + 2 <= 15) + (prev + 2 >= 4 && prev + 2 <= 15) + (prev >= 14 ? 2 : 0));
      float yA0, yA1, yB0, yB1, sA, sB;
      uint32_t wA, wB;
      auto dma = [&]() { if constexpr (G < CPW) stage_k1(PAR, kv0 + 128, G); else if constexpr (G < 2 * CPW) stage_v1((PAR + 1) & 1, kv0 + 64, G - CPW); };
      constexpr int KOFF = KN + ((G + 2) >> 3) * (32 * 256), VOFF = VB + ((G + 2) & 3) * (32 * 128);
      if constexpr (G >= 14) {            // P V + S; the reads are the trailing V^T fragments (two per step)
        constexpr int F1 = VB + (2 * (G - 14)) * (32 * 128), F2 = F1 + 32 * 128;
        Q64_STEP_HI_A("%[s0]", "+v", younger, oacc[0][G & 3], oacc[1][G & 3], vfr[G % 3], pk[0][(G >> 2) - 1], pk[1][(G >> 2) - 1], sn[0][T],
                      kfr[G % 3], qa[0][G & 7], vtr[2 * (G - 14)], avl[3], F1, vtr[2 * (G - 14) + 1], avl[3], F2, sc, T, E0, p.c, nmc[0], nmc[1]);
        dma();
        Q64_STEP_HI_B("%[s1]", "+v", sn[1][T], kfr[G % 3], qa[1][G & 7]);
      } else if constexpr (G == 8) {      // opens the second key half of S: C = 0
        Q64_STEP_HI_A("0", "=&v", younger, oacc[0][G & 3], oacc[1][G & 3], vfr[G % 3], pk[0][(G >> 2) - 1], pk[1][(G >> 2) - 1], sn[0][T],
                      kfr[G % 3], qa[0][G & 7], kfr[(G + 2) % 3], akl[(G + 2) & 7], KOFF, vfr[(G + 2) % 3], avl[((G + 2) >> 2) - 1], VOFF, sc, T, E0,
                      p.c, nmc[0], nmc[1]);
        dma();
        Q64_STEP_HI_B("0", "=&v", sn[1][T], kfr[G % 3], qa[1][G & 7]);
      } else if constexpr (G >= 4) {
        Q64_STEP_HI_A("%[s0]", "+v", younger, oacc[0][G & 3], oacc[1][G & 3], vfr[G % 3], pk[0][(G >> 2) - 1], pk[1][(G >> 2) - 1], sn[0][T],
                      kfr[G % 3], qa[0][G & 7], kfr[(G + 2) % 3], akl[(G + 2) & 7], KOFF, vfr[(G + 2) % 3], avl[((G + 2) >> 2) - 1], VOFF, sc, T, E0,
                      p.c, nmc[0], nmc[1]);
        dma();
        Q64_STEP_HI_B("%[s1]", "+v", sn[1][T], kfr[G % 3], qa[1][G & 7]);
      } else if constexpr (G == 0) {      // K(0) landed at the top of the body; opens the first key half: C = 0; one read (K(2))
        bf16x8_t none;
        Q64_STEP_LO_A("", "", "0", "0", "=&v", 0, sn[0][T], sn[1][T], kfr[0], qa[0][0], qa[1][0], kfr[2], akl[2], KOFF, none, akl[2], 0, sc, T, E0,
                      p.c, nmc[0], nmc[1]);
        dma();
        Q64_STEP_LO_B(kfr[0]);
      } else if constexpr (G == 1) {      // one read (K(3))
        bf16x8_t none;
        Q64_STEP_LO_A("s_waitcnt lgkmcnt(%[n])\n\t", "", "%[s0]", "%[s1]", "+v", younger, sn[0][T], sn[1][T], kfr[G % 3], qa[0][G], qa[1][G],
                      kfr[(G + 2) % 3], akl[G + 2], KOFF, none, akl[2], 0, sc, T, E0, p.c, nmc[0], nmc[1]);
        dma();
        Q64_STEP_LO_B(kfr[G % 3]);
      } else {                            // G = 2, 3: K(G+2) and V(G+2)
        Q64_STEP_LO_A("s_waitcnt lgkmcnt(%[n])\n\t", "ds_read_b128 %[d2], %[a2] offset:%[f2]\n\t", "%[s0]", "%[s1]", "+v", younger, sn[0][T],
                      sn[1][T], kfr[G % 3], qa[0][G], qa[1][G], kfr[(G + 2) % 3], akl[G + 2], KOFF, vfr[(G + 2) % 3], avl[((G + 2) >> 2) - 1], VOFF,
                      sc, T, E0, p.c, nmc[0], nmc[1]);
        dma();
        Q64_STEP_LO_B(kfr[G % 3]);
      }
      pk[0][G >> 2][G & 3] = wA;
      pk[1][G >> 2][G & 3] = wB;
    };
    q64_unroll16(step);
    q64_landed<0>(vtr[0], vtr[1], vtr[2], vtr[3]);              // the trailing fragments landed: every read of this tile's buffers is complete
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) l_run[qg] += ps[qg];
  };
  {
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    ATTN_STAMP(1);
    body(0, P0{}, scur, snext, std::true_type{});                // (the first tile's row maxima come from the prologue)
    if (nkv > 1) body(1, P1{}, snext, scur, std::false_type{});
    for (int it = 2; it < nkv; it += 2) {
      body(it, P0{}, scur, snext, std::false_type{});
      if (it + 1 < nkv) body(it + 1, P1{}, snext, scur, std::false_type{});
    }
    // the last tile's last key group
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int qg = 0; qg < 2; ++qg) Q64P_MFMA_O(oacc[qg][dt], vtr[dt], pk[qg][3]);
    ATTN_STAMP(2 + 2 * nkv);
  }
  const int le = q64_lane_now(l);         // the epilogue's and the next item's lane arithmetic (see q64_lane_now)
  Item nxt = cur;
  if (has_next) {                    // the next item's q rows: requested before this item's output is stored, in flight under the epilogue
    decode(item + (int)gridDim.x, nxt);
    q64_request(p, qlds, nxt, le);
  }

#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    Q64_SETTLE_O(oacc, qg);
    const float lt = l_run[qg] + __shfl_xor(l_run[qg], 32, 64);
    const float inv = 1.0f / lt;
    const int qrow = q0 + 32 * qg + (le & 31);
    store_out_row(p, b, h, qrow, le, inv, [&](int dt, int r) -> float { return oacc[qg][dt][r]; });
  }
  ATTN_STAMP(3 + 2 * (p.s_pad / 64));
  if (!has_next) break;
  stores_behind = q0 + 64 <= p.S ? ((p.tune & 2) ? 16 : 32) : 0;      // (every row of the wave valid: every store instruction was issued)
  q64_wait_older_than_stores(stores_behind);        // the q rows (the RoPE table rows q_fragments loads queue behind the stores; Q fragments computed BEFORE the
                                   //  epilogue instead — rows requested a tile earlier — cost spills in the q-preparation instantiation)
  q_fragments(nxt, le);
  q_to_agprs();
  ATTN_STAMP(5 + 2 * (p.s_pad / 64));
  item += (int)gridDim.x;
  cur = nxt;
  if (!paired) {                   // (paired: the stream switched both already)
    rsK = k_descr(cur);
    rsV = v_descr(cur);
  }
  ksub = vsub = 0;
  staged = paired;
  }
}

template __global__ void attention_q64_kernel<true>(AttnArgs);
template __global__ void attention_q64_kernel<false>(AttnArgs);

}  // namespace drag_attn

#if DRAG_EXP
// (hipMemcpyFromSymbol resolves a device global in the object that defines it: the library is linked without relocatable device code)
extern "C" int drag_debug_attn_stamps(unsigned long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(drag_attn::g_attn_stamps), (size_t)n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
