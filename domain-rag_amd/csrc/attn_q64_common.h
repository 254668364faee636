// attn_q64_common.h — what the two 64-query kernels (attention_q64.hip: hand-placed stream; attention_q64g.hip: generated stream) do alike
// outside their KV loops: the item walk, the K / V^T / q descriptors, the staging offsets, the request of an item's q rows, the seam's waits.
// A helper is used by a kernel only where that kernel's assembly kept its opcode histogram and register counts with it; elsewhere the
// kernel keeps a written-out copy, marked by a comment, and a fix has to be made in both places:
//   q64_decode, q64_k_descr, q64_v_descr      used by q64g only; attention_q64_kernel keeps its own
//   q64_stage_offsets, q64_lane_now           used by q64 only; attention_q64g_kernel keeps its own (the offsets twice: lane_consts, stage_first)
//   q64_q_descr, q64_request, q64_wait_older_than_stores (and q_norm_rope, store_out_row of attention_kernels.h)      used by both
#pragma once
#include "attention_kernels.h"

namespace drag_attn {

// An ITEM is a (batch, head) and a block of 256 queries: item & 7 = the XCD (heads 8 g + xcd share an L2), item >> 3 = (group, query block).
// A grid of p.items workgroups runs one item each; a smaller grid (a multiple of 8: one workgroup per CU) walks items i, i + grid, ... —
// all on the workgroup's XCD.  (grids smaller than p.items are launched only when B * H is a multiple of 8: every item exists)
struct Q64Item { int b, h, q0; };
__device__ __forceinline__ bool q64_decode(const AttnArgs& p, const int w, const int item, Q64Item& t) {
  constexpr int QB = 256;
  const int nqb = (p.S + QB - 1) / QB;
  const int xcd = item & 7, loc = item >> 3;
  const int bh = (loc / nqb) * 8 + xcd;
  t.b = bh / p.H;
  t.h = bh - t.b * p.H;
  t.q0 = (loc - (loc / nqb) * nqb) * QB + w * 64;              // group qg: queries q0 + 32 qg + (l & 31)
  return bh < p.B * p.H;
}

// descriptors based at the item's (batch, head), spanning that (batch, head) only
__device__ __forceinline__ __amdgpu_buffer_rsrc_t q64_k_descr(const AttnArgs& p, const Q64Item& t) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + (long long)t.b * p.qk_bs + t.h * 128), 0, p.k_bytes, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t q64_v_descr(const AttnArgs& p, const Q64Item& t) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p.vt + ((long long)(t.b * p.H + t.h) * 128) * p.s_pad), 0, p.vt_bytes, 0x00020000);
}
// (the K descriptor's span fits q: same row stride, same batch stride, same 128 columns of a head)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t q64_q_descr(const AttnArgs& p, const Q64Item& t) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p.q + (long long)t.b * p.qk_bs + t.h * 128), 0, p.k_bytes, 0x00020000);
}

// K / V^T staging offsets of wave w's piece i (of 4) for lane ll: the lane's row of the piece inside a tile and its swizzled 16-byte slot as
// ONE loop-invariant byte offset; a piece's address is that plus the tile's (uniform) byte offset — one v_add_u32 per piece (the clamp
// min(row, S - 1) and its 64-bit multiply-add cost three VALU instructions per piece in a loop bound by its issue slots).  Rows past S fall
// outside the (batch, head) descriptor: the LDS-DMA writes zeros for them, and their scores are masked by the ragged-tile path like the
// clamped copies of row S - 1 were.
__device__ __forceinline__ void q64_stage_offsets(const AttnArgs& p, const int w, const int ll, const int i, unsigned& koff, unsigned& voff) {
  const int c = w * 4 + i;
  const int krow = c * 4 + (ll >> 4);
  koff = (unsigned)krow * (unsigned)(p.ld_qk * 2) + (unsigned)(((ll & 15) ^ (krow & 15)) * 16);
  const int vrow = c * 8 + (ll >> 3);
  const int vslot = (ll & 7) ^ ((vrow >> 1) & 7);
  voff = (unsigned)(((long long)vrow * p.s_pad + vslot * 8) * 2);
}

// The q rows of item t are REQUESTED here (LDS-DMA, 16 bytes x 8 per lane and query group, every lane's pieces at lane-private LDS addresses
// — qlds: the wave's 16 KiB beside the tiles, no registers) — for the next item before this item's output is stored, so the round trip runs
// under the epilogue — and turned into fragments later (the kernels' q_fragments: read back, + RMSNorm / RoPE when QPREP, whose weight and
// table rows are L2-resident).  (Requested into registers, the 64 VGPRs were spilled around the epilogue and the spill stores waited for
// the loads they were meant to hide.)
__device__ __forceinline__ void q64_request(const AttnArgs& p, DRAG_LDS char* const qlds, const Q64Item& t, const int ll) {
  __amdgpu_buffer_rsrc_t rsQ = q64_q_descr(p, t);
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const int qr = min(t.q0 + 32 * qg + (ll & 31), p.S - 1);
    const unsigned vo = (unsigned)qr * (unsigned)(p.ld_qk * 2) + (unsigned)((ll >> 5) * 16);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (DRAG_LDS void*)(qlds + (qg * 8 + ks) * 1024), 16, vo, ks * 32, 0, 0);   // (the column offset as the
                                                                     // scalar offset: an instruction offset would move the LDS address as well)
  }
}

// (what an item's seam derives from the lane id is recomputed per item from a laundered copy: hoisted out of the item loop it would sit
//  in VGPRs across the KV stream, which has 38 to spare — the first build of this loop spilled 1.3 KB to scratch, inside the stream too)
__device__ __forceinline__ int q64_lane_now(const int l) {
  int v = l;
  asm volatile("" : "+v"(v));
  return v;
}

// The previous item's output stores are the YOUNGEST vector-memory operations when the next item begins: its q rows and first tiles were
// requested before them, and a wave's vector-memory operations retire in issue order — so the waits of the seam leave exactly that many
// operations in flight instead of draining the stores (their acknowledgements take microseconds).  0 = count unknown (a ragged query
// block skips stores): wait for everything
__device__ __forceinline__ void q64_wait_older_than_stores(const int stores_behind) {
  if (stores_behind == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (stores_behind == 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace drag_attn
