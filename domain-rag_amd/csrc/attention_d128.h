// attention_d128.h — attention_d128_kernel's body: 8 or 4 waves x 32 queries.  attention_d128_w8.hip and attention_d128_w4.hip instantiate it.
#pragma once
#include "attention_kernels.h"

namespace drag_attn {

// --------------------------------------------------------------------------------------------
// flash attention, D = 128.   grid (ceil(S/128), H, B), block 256.
// --------------------------------------------------------------------------------------------
// SCHED 0: per KV tile, 16 {S(j+1) MFMA | exp of S(j)} steps, then the 16 P V MFMAs.
// SCHED 2 (experiment, "attn_sched" 3): SCHED 1 with every V^T fragment read one step ahead of its MFMA.
// SCHED 1: the P V MFMAs of key group s2 are issued as soon as that group's 16 probabilities are packed (from step 4 on, one
//          per step next to the S MFMA), so the exp stream is spread over 28 MFMAs instead of 16 and only 4 P V MFMAs trail
//          the loop.  Same arithmetic, same order per accumulator: bit-identical outputs.
// PMAX: the row maxima of S(j+1) are taken at the END of iteration j (next to the trailing P V MFMAs, which need no VALU)
//       instead of at the start of iteration j+1, where the matrix pipe has nothing to do.  Same values, same order.
// VROW: V is read ROW-MAJOR, straight from the qkv buffer (no V^T pass, no V^T buffer).  The V tile [64 keys][128 d] is staged like
//       the K tile (4 key rows per LDS-DMA instruction) and the A operand of O^T += V^T P^T — per lane 8 keys of one d — comes from
//       two ds_read_b64_tr_b16: within a 16-lane group source lane 4j + r supplies 4 consecutive d of key j, result lane 4r + e
//       receives (key 0..3) at d = 4r + e (probed on the hardware: scripts/probe/probe_tr16.hip).  The first read fetches the key
//       quad that this half-wave's P registers 0-3 hold, the second the quad of registers 4-7, so the key permutation the V^T
//       image needed is absorbed by the addresses.  16-byte units of a key row are XOR-swizzled with 4 * (key & 3): the 16 units
//       (4 keys x 64 B) a 32-lane access touches fall into 16 different bank groups.  Same MFMA operands -> same bits as the V^T kernels.
// PERSIST (round 3; measured 1 % slower than one item per workgroup, kept off the product path — see attention_launch): one workgroup per CU walks the items (batch-head, query block) loc = slot, slot + P/8, ... of its XCD's list and
//       the K / V^T LDS-DMA stream runs CONTINUOUSLY across them: the last two KV iterations of an item — whose prefetches used to
//       fetch tiles past the sequence end that nobody reads — fetch tiles 0, 0, 1 of the NEXT item instead, so the next item starts
//       with its operands in LDS and pays neither a workgroup dispatch nor the first HBM round trip.  Measured per workgroup outside
//       its KV loop before this (scripts/bench_attn_seams.py, B=8 S=5337): 6.6 us plain, 10.9 us with the q preparation = 4.3 % / 7.0 %
//       of an 84-tile workgroup.  The descriptors span the whole K / V^T tensors and an item is a scalar byte offset, so switching
//       items costs two SGPRs.  Same arithmetic per item: bit-identical outputs.
namespace {
// The kernel's K / V^T tiles: every instantiation allocates its own 64 KiB.  Internal linkage, at namespace scope: as a static local of a kernel
// that other objects launch the array is linkonce_odr, and hipcc then orders the address arithmetic of the first staging pieces differently
// (same instructions, another order, one s_nop more in <4, 1, true, true, true>); this form compiles to the assembly the kernels had as
// internal functions of attention.hip.  Include this header only from a source that instantiates the kernel.
__shared__ __attribute__((aligned(16))) char smem[2 * KT_BYTES + 2 * VT_BYTES];
}
template <int NW, int SCHED, bool QPREP, bool PMAX, bool VROW, bool PERSIST>   // NW: waves per block (4 or 8), 32 queries each; QPREP: RMSNorm + RoPE of q on load
__global__ __launch_bounds__(512, 2) void attention_d128_kernel(AttnArgs p) {
  const int w = wave_id(), l = lane_id();
  const int hh = l >> 5;            // half-wave
  // XCD-aware mapping (speed only): block id -> XCD id%8; all query blocks of one (batch, head) run on ONE XCD so
  // its K / V^T stream is fetched into a single private L2 instead of all eight.
  constexpr int QB = NW * 32;          // queries per block
  constexpr int CPW = 16 / NW;         // 1-KiB DMA chunks per wave per tile (K and V^T tiles have 16 each)
  const int nqb = (p.S + QB - 1) / QB;
  const int xcd = blockIdx.x & 7;
  int loc = blockIdx.x >> 3;           // index into this XCD's item list: item -> (bh = (loc / nqb) * 8 + xcd, query block loc % nqb)
  const int nloc = ((p.B * p.H + 7) / 8) * nqb;
  const int lstep = PERSIST ? (int)(gridDim.x >> 3) : nloc;
  if (((loc / nqb) * 8 + xcd) >= p.B * p.H) return;      // (PERSIST launches only when B * H is a multiple of 8: every item exists)
  int b, h, q0;
  unsigned soK, soV;                  // scalar byte offsets of this item's (batch, head) inside the K tensor / the V^T (or V) tensor
  auto item_offsets = [&](int lc, int& bb, int& hd, unsigned& ok, unsigned& ov) {
    const int bh = (lc / nqb) * 8 + xcd;
    bb = bh / p.H; hd = bh - bb * p.H;
    ok = (unsigned)(((long long)bb * p.qk_bs + hd * 128) * 2);
    ov = VROW ? ok : (unsigned)((((long long)(bb * p.H + hd)) * 128) * p.s_pad * 2);
  };
  item_offsets(loc, b, h, soK, soV);
  q0 = (loc - (loc / nqb) * nqb) * QB + w * 32;

  // ---- Q fragments stay in registers: B operand, lane -> query (l&31), k = 16ks + 8hh .. +8 (loaded below, after the
  // first K / V^T tiles have been requested: one workgroup per CU, so nothing else hides this prologue's latency) ----
  bf16x8_t qf[8];
  // ---- staging descriptors.  One item per workgroup (the product): based at the item's (batch, head), spanning that (batch, head) only —
  // tensors of any size work as long as ONE (batch, head) stays below 2 GiB (whole-tensor descriptors had put a 4 GiB cap on
  // B x S for the sake of the persistent experiment).  PERSIST: the WHOLE K / V^T tensor, the item is a scalar offset.
  __amdgpu_buffer_rsrc_t rsK, rsV;
  if constexpr (PERSIST) {
    rsK = __builtin_amdgcn_make_buffer_rsrc((void*)p.k, 0, p.k_bytes_all, 0x00020000);
    rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(VROW ? p.v : p.vt), 0, VROW ? p.k_bytes_all : p.vt_bytes_all, 0x00020000);
  } else {
    const long long kb = ((long long)b * p.qk_bs + h * 128) * 2;
    rsK = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.k + kb), 0, p.k_bytes, 0x00020000);
    if constexpr (VROW) rsV = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.v + kb), 0, p.k_bytes, 0x00020000);
    else rsV = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.vt + (long long)(b * p.H + h) * 128 * p.s_pad * 2), 0, p.vt_bytes, 0x00020000);
    soK = 0; soV = 0;
  }
  unsigned soKn = soK, soVn = soV;    // the NEXT item's offsets (PERSIST; = this item's when there is none: harmless re-reads)
  // K chunk c (1 KiB) = key rows 4c..4c+3; lane: row 4c + (l>>4), physical slot l&15
  // V chunk c (1 KiB) = d rows 8c..8c+7;   lane: row 8c + (l>>3), physical slot l&7
  int krow[4];                        // (fixed-size: a template-dependent array bound here makes hipcc drop the host stub)
  unsigned kslot[4], voff[4];
  // VROW: V chunk c = key rows 4c..4c+3 like K; physical slot l&15 holds logical 16-byte unit (l&15) ^ 4*(key&3)
  const unsigned vrslot = (unsigned)(((l & 15) ^ (4 * ((l >> 4) & 3))) * 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= CPW) break;
    const int c = w * CPW + i;
    krow[i] = c * 4 + (l >> 4);
    kslot[i] = (unsigned)(((l & 15) ^ (krow[i] & 15)) * 16);
    const int vrow = c * 8 + (l >> 3);
    const int vslot = (l & 7) ^ ((vrow >> 1) & 7);
    voff[i] = (unsigned)(((long long)vrow * p.s_pad + vslot * 8) * 2);
  }
  // tile index kv0 >= s_pad names tile kv0 - s_pad of the NEXT item (PERSIST): wave-uniform selects, no branches
  auto stage_k1 = [&](int buf, int kv0, int i) {
    const int c = w * CPW + i;
    const bool nx = PERSIST && kv0 >= p.s_pad;
    const int kvr = nx ? kv0 - p.s_pad : kv0;
    const int kr = min(kvr + krow[i], p.S - 1);
    const unsigned ko = (unsigned)((long long)kr * p.ld_qk * 2) + kslot[i];
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, (DRAG_LDS void*)((DRAG_LDS char*)smem + buf * KT_BYTES + c * 1024), 16, ko, nx ? soKn : soK, 0, 0);
  };
  auto stage_k = [&](int buf, int kv0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= CPW) break;
      stage_k1(buf, kv0, i);
    }
  };
  auto stage_v1 = [&](int buf, int kv0, int i) {
    const int c = w * CPW + i;
    const bool nx = PERSIST && kv0 >= p.s_pad;
    const int kvr = nx ? kv0 - p.s_pad : kv0;
    const unsigned so = nx ? soVn : soV;
    DRAG_LDS char* dV = (DRAG_LDS char*)smem + 2 * KT_BYTES + buf * VT_BYTES + c * 1024;
    if constexpr (VROW) {
      const int vr = min(kvr + krow[i], p.S - 1);          // rows past S are real rows: finite values under a zero probability
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (DRAG_LDS void*)dV, 16, (unsigned)((long long)vr * p.ld_qk * 2) + vrslot, so, 0, 0);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (DRAG_LDS void*)dV, 16, voff[i], so + (unsigned)(kvr * 2), 0, 0);
    }
  };
  auto stage_v = [&](int buf, int kv0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= CPW) break;
      stage_v1(buf, kv0, i);
    }
  };

  // ---- fragment read offsets ----
  // K: row (l&31)+32t, logical slot 2ks+hh, physical = logical ^ (row&15)
  const int krd = (l & 31) * 256;
  const int kx = l & 15;
  // V^T: row (l&31)+32dt, logical slot 2s+hh, physical = logical ^ ((row>>1)&7)
  const int vrd = (l & 31) * 128;
  const int vx = ((l & 31) >> 1) & 7;

  f32x16_t oacc[4];
  float m_run, l_run;

  const int nkv = p.s_pad / 64;
  f32x16_t scur[2], snext[2];
  {
  // ---- depth-1 pipeline: while the VALU works on the softmax of tile j, the matrix pipe already computes
  // S(j+1) = K(j+1) Q^T (independent of it), then O += P(j) V(j).  K therefore runs one tile ahead of V:
  // iteration j needs K(j+1) and V(j) in LDS and stages K(j+2), V(j+1).
  // The loop is unrolled by two with the buffer parity as a compile-time constant: every ds_read address is one of 12
  // loop-invariant VGPRs (8 K slots, 4 V^T slots: the XOR swizzle makes them lane-dependent) plus an immediate, the
  // S accumulators ping-pong between two register sets instead of being copied, and the first MFMA of a chain takes
  // C = 0 as an inline constant.
  // Measured alternatives (same box, interleaved runs, B=8 S=5337): a depth-2 pipeline that also overlaps P(j-1) V(j-1)
  // with the softmax of tile j (32 uniform {MFMA, exp} steps, fragment ring 3 deep) 1003 vs 1058 TFLOP/s for this loop;
  // this loop without its barrier +4 %, without barrier and vmcnt wait +4 % (synchronisation is not the limiter);
  // K / V^T staged through registers (buffer_load -> ds_write_b128 at the end of the iteration) instead of LDS-DMA
  // 1041 vs 1088 TFLOP/s; the two wave halves run half an iteration apart (softmax half of one SIMD partner beside the
  // P V half of the other, two barriers per tile, V^T triple-buffered) 1047 vs 1068.
  // PMC (B=8 S=5337): effective clock 1.70 GHz (power-limited; 2.4 nominal), MFMA pipe 52-59 % busy at that clock.
  int ak[8], av[4];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) ak[ks] = krd + (((2 * ks + hh) ^ kx) << 4);
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) av[s2] = vrd + (((2 * s2 + hh) ^ vx) << 4);
  // VROW: byte offset of this lane's 8-byte source piece for d block dt (32 rows of V^T): key 4 hh + (si>>2) of a quad pair,
  // 16-byte unit 4 dt + 2 g1 + ((si>>1)&1) swizzled with 4 * (key & 3), half (si & 1); + 4096 per 16-key group, + 2048 for the second quad
  int avd[4];
  {
    const int si = l & 15, g1 = (l >> 4) & 1;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      avd[dt] = (4 * hh + (si >> 2)) * 256 + ((4 * (dt ^ (si >> 2)) + 2 * g1 + ((si >> 1) & 1)) << 4) + (si & 1) * 8;
  }
  auto read_v = [&](const int s2, const int dt, const int vb) -> bf16x8_t {
    if constexpr (VROW) {
      typedef short s16x4_t __attribute__((ext_vector_type(4)));
      typedef short s16x8_t __attribute__((ext_vector_type(8)));
      DRAG_LDS char* a = (DRAG_LDS char*)smem + (avd[dt] + (vb + s2 * 4096));
      const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DRAG_LDS s16x4_t*)a);
      const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DRAG_LDS s16x4_t*)(a + 2048));
      return __builtin_bit_cast(bf16x8_t, (s16x8_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    } else {
      return *(const bf16x8_t*)(smem + (av[s2] + (vb + dt * (32 * 128))));
    }
  };
  const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  stage_k(0, 0);
  stage_v(0, 0);
  if (nkv > 1) stage_k(1, 64);
  for (;;) {                           // items of this workgroup (one, unless PERSIST)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
  m_run = -INFINITY; l_run = 0.f;
  const bool has_next = PERSIST && loc + lstep < nloc;
  if (PERSIST) {                       // where the stream goes when this item's tiles run out
    int bn, hn;
    if (has_next) item_offsets(loc + lstep, bn, hn, soKn, soVn);
    else { soKn = soK; soVn = soV; }
  }
  // Q load (+ RMSNorm / RoPE when QPREP) while those tiles are in flight
  {
    const int qr = min(q0 + (l & 31), p.S - 1);
    const bf16_t* qp = p.q + (long long)b * p.qk_bs + (long long)qr * p.ld_qk + h * 128 + hh * 8;
    if constexpr (!QPREP) {
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8_t*)(qp + ks * 16);
    } else {
      // (this kernel's own copy of q_norm_rope, attention_kernels.h: through the function the loads come in another order and the multiplies pack differently)
      // per-head RMSNorm(128) + interleaved RoPE of this lane's query row, with the rounding points of the separate pass
      // (qk_norm_rope_vt_kernel): rbf(rbf(x * rs) * w), rotation in fp32, one rounding to bf16.  The lane holds 64 of the
      // row's 128 elements (d = 16 ks + 8 hh + 0..7), lane ^ 32 the other 64; RoPE pairs (2j, 2j+1) never straddle lanes.
      // All 32 loads are issued before anything is consumed: one memory latency, overlapped with the K / V^T prologue DMA
      // (a per-ks `if (table != null)` form compiled to eight serialised load-wait-branch rounds: +91 us per B=8 launch).
      const bf16_t* wsel = (qr < p.s_txt ? p.wq_txt : p.wq_img) + hh * 8;
      const float* cp = p.cosT + (long long)qr * 64 + hh * 4;
      const float* sp = p.sinT + (long long)qr * 64 + hh * 4;
      u32x4_t raw[8], wr[8];
      f32x4_t c4[8], s4[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        raw[ks] = *(const u32x4_t*)(qp + ks * 16);
        wr[ks] = *(const u32x4_t*)(wsel + ks * 16);
        c4[ks] = *(const f32x4_t*)(cp + ks * 8);
        s4[ks] = *(const f32x4_t*)(sp + ks * 8);
      }
      float ss = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a0 = bf2f((bf16_t)(raw[ks][j] & 0xffff)), a1 = bf2f((bf16_t)(raw[ks][j] >> 16));
          ss += a0 * a0;
          ss += a1 * a1;
        }
      ss += __shfl_xor(ss, 32, 64);
      const float rs = rsqrtf(ss * (1.0f / 128.0f) + p.eps);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        u32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float a0 = rbf(rbf(bf2f((bf16_t)(raw[ks][j] & 0xffff)) * rs) * bf2f((bf16_t)(wr[ks][j] & 0xffff)));
          const float a1 = rbf(rbf(bf2f((bf16_t)(raw[ks][j] >> 16)) * rs) * bf2f((bf16_t)(wr[ks][j] >> 16)));
          o[j] = pack2bf(a0 * c4[ks][j] - a1 * s4[ks][j], a1 * c4[ks][j] + a0 * s4[ks][j]);
        }
        qf[ks] = __builtin_bit_cast(bf16x8_t, o);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8_t kf = *(const bf16x8_t*)(smem + (ak[ks] + t * (32 * 256)));
      scur[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], ks == 0 ? zero16 : scur[t], 0, 0, 0);
    }
  // one KV tile; PAR = it & 1 is a compile-time constant; reads S from sc, writes S(it+1) to sn
  // keys >= S of a ragged last tile do not exist: -inf before the row maximum is taken
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
  float mt_carry = 0.f;
  if (PMAX) mt_carry = mask_and_max(scur, 0);
  if (p.tune & 1) {       // T5 static form: the second-dispatched wave half loses VALU arbitration to the older half on every segment
    if (w >= NW / 2) __builtin_amdgcn_s_setprio(1);
  }
  auto body = [&](const int it, auto par, f32x16_t (&sc)[2], f32x16_t (&sn)[2]) {
    constexpr int PAR = decltype(par)::value;
    constexpr int KN = ((PAR + 1) & 1) * KT_BYTES;                 // K(it+1)
    constexpr int VB = 2 * KT_BYTES + PAR * VT_BYTES;              // V(it)
    const int kv0 = it * 64;
    // K(it+1), V(it) landed (issued one iteration ago); every wave is done with K(it) and V(it-1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // (the LDS-DMA for K(it+2) / V(it+1) is issued piecewise between the MFMAs of the interleaved loop below:
    //  a burst of 2*CPW buffer_load..lds per wave right after the barrier idles the matrix pipe of every SIMD)
    // ---- online softmax (exp2 domain), deferred rescale ----
    const float mt = PMAX ? mt_carry : mask_and_max(sc, kv0);
    // Only move the running max (and rescale O, l) when some row's max grew by more than 2^8 in the
    // exp2 domain; otherwise P = exp2(s - m_old) is bounded by 2^8, which fp32 accumulation and the
    // bf16 P operand (relative precision is scale-free) absorb.  The previous tile's P·V is complete
    // at this point, so everything still at the old scale (O, l) is rescaled exactly once.
    if (!__all((mt - m_run) * p.c <= DEFER_THR)) {
      const float m_new = fmaxf(m_run, mt);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.c);
      l_run *= alpha;
      m_run = m_new;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
    }
    // ---- matrix pipe: S(it+1) = K(it+1) Q^T   ||   VALU: P(it) = exp2(S(it) - m), row sums, bf16 packing.
    // The two streams are independent, but hipcc emits 16 back-to-back MFMAs followed by the whole softmax, so the
    // interleave is written out: 16 steps of {prefetch next K fragment, 1 MFMA, 2 exps + pack}, each fenced with
    // sched_barrier so the order survives.  S(it+1) is computed unconditionally (in the last iteration it reads a
    // stale K buffer and is discarded).
    const float nmc = -(m_run * p.c);
    float ps = 0.f;
    u32x4_t pk[4];
    {
      bf16x8_t kf = *(const bf16x8_t*)(smem + (ak[0] + KN));
      bf16x8_t vpipe;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const bf16x8_t kcur = kf;
        if (g < 15) {
          const int t1 = (g + 1) >> 3, ks1 = (g + 1) & 7;
          kf = *(const bf16x8_t*)(smem + (ak[ks1] + (KN + t1 * (32 * 256))));
        }
        bf16x8_t vfg;
        if (SCHED == 1 && g >= 4) vfg = read_v((g >> 2) - 1, g & 3, VB);
        if (SCHED == 2) {      // the V^T fragment of step g was read in step g-1: a whole step (2 MFMAs + the softmax slice) covers its latency
          vfg = vpipe;
          if (g >= 3 && g < 15) vpipe = read_v(((g + 1) >> 2) - 1, (g + 1) & 3, VB);
        }
        sn[g >> 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kcur, qf[g & 7], (g & 7) == 0 ? zero16 : sn[g >> 3], 0, 0, 0);
        // unconditional (no branches: a branch here splits the block and hipcc then hoists the whole softmax out of the
        // interleave): past the last tile the K rows clamp to S-1 and the V^T offsets fall outside the descriptor's range
        // (reads return 0); both land in buffers nobody reads any more
        if (g < CPW) stage_k1(PAR, kv0 + 128, g);
        else if (g < 2 * CPW) stage_v1((PAR + 1) & 1, kv0 + 64, g - CPW);
        // the softmax arithmetic is side-effect free, so instruction selection is free to cluster all of it ahead of the
        // first step (it did: the steps then held only ds_read + MFMA).  Two empty asm volatile statements chain its
        // inputs after the previous step and its results before this step's fence.
        float y0, y1;      // s * c - m*c; written as asm so that the chain anchor costs no register copies
        asm volatile("v_fma_f32 %0, %2, %4, %5\n\tv_fma_f32 %1, %3, %4, %5"
                     : "=&v"(y0), "=&v"(y1) : "v"(sc[g >> 3][(2 * g) & 15]), "v"(sc[g >> 3][((2 * g) & 15) + 1]), "s"(p.c), "v"(nmc));
        const float e0 = __builtin_amdgcn_exp2f(y0);
        const float e1 = __builtin_amdgcn_exp2f(y1);
        ps += e0 + e1;
        uint32_t wd = pack2bf(e0, e1);
        asm volatile("" : "+v"(wd), "+v"(ps));
        pk[g >> 2][g & 3] = wd;
        if (SCHED >= 1 && g >= 4)       // O^T[dt = g & 3] += V^T[.., keys of group (g >> 2) - 1] P^T: that group was packed >= 1 step ago
          oacc[g & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfg, __builtin_bit_cast(bf16x8_t, pk[(g >> 2) - 1]), oacc[g & 3], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    l_run += ps;
    bf16x8_t pf[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) pf[s2] = __builtin_bit_cast(bf16x8_t, pk[s2]);
    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int s2 = (SCHED >= 1 ? 3 : 0); s2 < 4; ++s2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x8_t vf = read_v(s2, dt, VB);
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s2], oacc[dt], 0, 0, 0);
      }
    // S(it+1) is complete: its row maxima now, beside the trailing P V MFMAs (in the last iteration sn is stale and unused)
    if (PMAX) mt_carry = mask_and_max(sn, kv0 + 64);
  };
  for (int it = 0; it < nkv; it += 2) {
    body(it, std::integral_constant<int, 0>{}, scur, snext);
    if (it + 1 < nkv) body(it + 1, std::integral_constant<int, 1>{}, snext, scur);
  }

  // ---- epilogue: lane holds O[query l&31][d = 32dt + 8(r>>2) + 4hh + (r&3)] ----
  // (this kernel's own copy of store_out_row, attention_kernels.h: through the function every instantiation takes one or two VGPRs more)
  const float lt = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / lt;
  const int qrow = q0 + (l & 31);
  if (p.tune & 2) {
    // T21: lanes l and l + 32 hold the two 8-byte halves of each 16-byte output chunk.  One v_permlane32_swap per dword
    // regroups a pair of chunks (g, g + 1) so that the lower half-wave stores chunk g and the upper one chunk g + 1 as
    // whole 16-byte pieces: 8 store instructions per lane instead of 16 (the tail is store-ISSUE bound).
    bf16_t* op = p.out + (long long)b * p.o_bs + (long long)qrow * p.ld_o + h * 128 + 8 * hh;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; g += 2) {
        uint32_t a0 = pack2bf(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv);
        uint32_t a1 = pack2bf(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
        uint32_t b0 = pack2bf(oacc[dt][4 * g + 4] * inv, oacc[dt][4 * g + 5] * inv);
        uint32_t b1 = pack2bf(oacc[dt][4 * g + 6] * inv, oacc[dt][4 * g + 7] * inv);
        const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        // lower lanes: (r[0], r[1]) = (own chunk-g half, upper lane's chunk-g half); upper lanes: (lower's chunk g+1 half, own)
        const u32x4_t o = {r0[0], r1[0], r0[1], r1[1]};
        if (qrow < p.S) *(u32x4_t*)(op + 32 * dt + 8 * g) = o;
      }
  } else if (qrow < p.S) {
    bf16_t* op = p.out + (long long)b * p.o_bs + (long long)qrow * p.ld_o + h * 128 + 4 * hh;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x2_t o;
        o[0] = pack2bf(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv);
        o[1] = pack2bf(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
        *(u32x2_t*)(op + 32 * dt + 8 * g) = o;
      }
  }
  if (!has_next) break;
  // ---- next item: its K(0), V^T(0), K(1) tiles are already in LDS / in flight (issued by the last two KV iterations) ----
  loc += lstep;
  item_offsets(loc, b, h, soK, soV);
  q0 = (loc - (loc / nqb) * nqb) * QB + w * 32;
  }                                    // items
  }
}

}  // namespace drag_attn
