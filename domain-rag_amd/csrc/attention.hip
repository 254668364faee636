// attention.hip — the host side of the attention kernels: which kernel a call takes, the launches, the C ABI.  The kernels and what they share
// are described in attention_kernels.h; each is compiled from its own source.
#include "attention_kernels.h"
#include "drag_launch.h"

using namespace drag_attn;

static void fill_prep(PrepArgs& p, void* qkv, void* vt, const void* wq_txt, const void* wk_txt, const void* wq_img, const void* wk_img,
                      const float* rope_cos, const float* rope_sin, int32_t B, int32_t S, int32_t H, int32_t ld, int32_t s_txt, float eps,
                      int skip_q) {
  p.qkv = (bf16_t*)qkv; p.vt = (bf16_t*)vt;
  p.wq_txt = (const bf16_t*)wq_txt; p.wk_txt = (const bf16_t*)wk_txt;
  p.wq_img = (const bf16_t*)wq_img; p.wk_img = (const bf16_t*)wk_img;
  p.cosT = rope_cos; p.sinT = rope_sin;
  p.B = B; p.S = S; p.H = H; p.ld = ld; p.s_txt = s_txt; p.s_pad = (S + 63) / 64 * 64; p.eps = eps;
  p.skip_q = skip_q;
}

extern "C" int drag_qk_norm_rope_vt_bf16(void* qkv, void* vt, const void* wq_txt, const void* wk_txt,
                                         const void* wq_img, const void* wk_img, const float* rope_cos,
                                         const float* rope_sin, int32_t B, int32_t S, int32_t H, int32_t ld,
                                         int32_t s_txt, float eps, void* stream) {
  DRAG_CHECK(qkv && vt, "drag_qk_norm_rope_vt_bf16: null pointer");
  DRAG_CHECK((wq_txt && wk_txt && wq_img && wk_img) || (!wq_txt && !wk_txt && !wq_img && !wk_img),
             "drag_qk_norm_rope_vt_bf16: norm weights are all-or-none");
  DRAG_CHECK((rope_cos == nullptr) == (rope_sin == nullptr), "drag_qk_norm_rope_vt_bf16: cos/sin come in pairs");
  DRAG_CHECK(B > 0 && S > 0 && H > 0 && ld >= 3 * H * 128 && ld % 8 == 0, "drag_qk_norm_rope_vt_bf16: bad shape");
  PrepArgs p;
  fill_prep(p, qkv, vt, wq_txt, wk_txt, wq_img, wk_img, rope_cos, rope_sin, B, S, H, ld, s_txt, eps, 0);
  hipLaunchKernelGGL(qk_norm_rope_vt_kernel, dim3((S + 63) / 64, H, B), dim3(256), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}

// k and v only: the q third of the pass (a read + a write of M x D) moves into the attention kernel's fragment load
extern "C" int drag_k_norm_rope_vt_bf16(void* qkv, void* vt, const void* wk_txt, const void* wk_img, const float* rope_cos,
                                        const float* rope_sin, int32_t B, int32_t S, int32_t H, int32_t ld, int32_t s_txt,
                                        float eps, void* stream) {
  DRAG_CHECK(qkv, "drag_k_norm_rope_vt_bf16: null pointer");      // vt == null: k only (drag_attention_v_bf16 reads v as it is)
  DRAG_CHECK((wk_txt == nullptr) == (wk_img == nullptr), "drag_k_norm_rope_vt_bf16: norm weights come in pairs");
  DRAG_CHECK((rope_cos == nullptr) == (rope_sin == nullptr), "drag_k_norm_rope_vt_bf16: cos/sin come in pairs");
  DRAG_CHECK(B > 0 && S > 0 && H > 0 && ld >= 3 * H * 128 && ld % 8 == 0, "drag_k_norm_rope_vt_bf16: bad shape");
  PrepArgs p;
  fill_prep(p, qkv, vt, wk_txt, wk_txt, wk_img, wk_img, rope_cos, rope_sin, B, S, H, ld, s_txt, eps, 1);      // wq_* only flags "normalise" in the kernel
  hipLaunchKernelGGL(qk_norm_rope_vt_kernel, dim3((S + 63) / 64, H, B), dim3(256), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}

static int attention_launch(const void* q, const void* k, const void* vt, void* out, int32_t B, int32_t S, int32_t H,
                            int32_t ld_qk, int64_t qk_batch_stride, int32_t ld_o, int64_t o_batch_stride, float scale,
                            const void* wq_txt, const void* wq_img, const float* rope_cos, const float* rope_sin, int32_t s_txt,
                            float eps, void* stream, bool vrow = false);

// which kernel family a call of S keys takes (one policy for the launch and for drag_attention_bf16_choice)
static void attention_family(int32_t S, bool vrow, bool& w8, bool& q64) {
  w8 = !drag_opt(DRAG_OPT_ATTN_W4) && S >= 4096;     // 8-wave blocks halve the DMA issue per wave; below ~4k keys 128-query blocks balance better (S=1753: 945 vs 843 TFLOP/s)
  // "attn_q64": 0 = policy (the 4-wave x 64-query kernel for S >= 4096, where it is 4-5 % ahead; below that its 256-query blocks fill
  // the chip worse: S = 1753 911 vs 982 TFLOP/s), 1 = whenever S >= 1024, 2 = never (the 8-wave / 4-wave x 32-query family: measurements, tests)
  const int q64opt = drag_opt(DRAG_OPT_ATTN_Q64);
  q64 = !vrow && q64opt != 2 && ((q64opt == 1 && S >= 1024) || (q64opt == 0 && w8 && (!DRAG_EXP || drag_opt(DRAG_OPT_ATTN_PERSIST) == 0)));
}

// does a 64-query launch over S keys take the generated stream (attention_q64g_kernel)?  Its last two tiles stage the next item's first
// tiles: an even number >= 4 of KV tiles; "attn_gen" = 1 switches it off
static bool attention_generated(int32_t S) {
  const int nkv = (S + 63) / 64;
  return drag_opt(DRAG_OPT_ATTN_GEN) != 1 && nkv % 2 == 0 && nkv >= 4;
}

// 64 = attention_q64_kernel, 640 = attention_q64g_kernel without the fold, 641 = with it (fused q preparation only), 8 / 4 =
// attention_d128_kernel<8 | 4 waves, ...> — for callers that account launches per kernel (bench.py)
extern "C" int drag_attention_bf16_choice(int32_t S, int32_t v_row_major, int32_t q_prep) {
  bool w8, q64;
  attention_family(S, v_row_major != 0, w8, q64);
  if (q64 && attention_generated(S)) return q_prep && drag_opt(DRAG_OPT_ATTN_GEN) != 2 ? 641 : 640;
  return q64 ? 64 : (w8 ? 8 : 4);
}

extern "C" int drag_attention_bf16(const void* q, const void* k, const void* vt, void* out, int32_t B, int32_t S,
                                   int32_t H, int32_t ld_qk, int64_t qk_batch_stride, int32_t ld_o,
                                   int64_t o_batch_stride, float scale, void* stream) {
  return attention_launch(q, k, vt, out, B, S, H, ld_qk, qk_batch_stride, ld_o, o_batch_stride, scale, nullptr, nullptr, nullptr,
                          nullptr, 0, 0.f, stream);
}

// attention whose Q operand is the RAW q projection: per-head RMSNorm (weights wq_txt for rows < s_txt, wq_img after) and
// RoPE are applied while the Q fragments are loaded (FluxAttnProcessor2_0: norm_q / norm_added_q + apply_rotary_emb)
extern "C" int drag_attention_qprep_bf16(const void* q, const void* k, const void* vt, void* out, int32_t B, int32_t S,
                                         int32_t H, int32_t ld_qk, int64_t qk_batch_stride, int32_t ld_o,
                                         int64_t o_batch_stride, float scale, const void* wq_txt, const void* wq_img,
                                         const float* rope_cos, const float* rope_sin, int32_t s_txt, float eps, void* stream) {
  DRAG_CHECK(wq_txt && wq_img && rope_cos && rope_sin,
             "drag_attention_qprep_bf16: the fused q preparation needs both norm weights and both RoPE tables "
             "(drag_attention_bf16 takes an already prepared q)");
  DRAG_CHECK(s_txt >= 0 && s_txt <= S, "drag_attention_qprep_bf16: 0 <= s_txt <= S");
  return attention_launch(q, k, vt, out, B, S, H, ld_qk, qk_batch_stride, ld_o, o_batch_stride, scale, wq_txt, wq_img, rope_cos,
                          rope_sin, s_txt, eps, stream);
}

// attention over q | k | v AS THE LINEARS WROTE THEM: v is read row-major from the projection buffer (same row stride and batch
// stride as q / k) — no V^T pass, no V^T buffer.  The q preparation is optional: all four of wq_txt / wq_img / rope_cos /
// rope_sin, or none of them (then q is used as stored, like drag_attention_bf16).
extern "C" int drag_attention_v_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t S, int32_t H,
                                     int32_t ld_qk, int64_t qk_batch_stride, int32_t ld_o, int64_t o_batch_stride, float scale,
                                     const void* wq_txt, const void* wq_img, const float* rope_cos, const float* rope_sin,
                                     int32_t s_txt, float eps, void* stream) {
  const int given = (wq_txt != nullptr) + (wq_img != nullptr) + (rope_cos != nullptr) + (rope_sin != nullptr);
  DRAG_CHECK(given == 0 || given == 4, "drag_attention_v_bf16: the fused q preparation takes both norm weights and both RoPE tables, or none");
  DRAG_CHECK(given == 0 || (s_txt >= 0 && s_txt <= S), "drag_attention_v_bf16: 0 <= s_txt <= S");
  return attention_launch(q, k, v, out, B, S, H, ld_qk, qk_batch_stride, ld_o, o_batch_stride, scale, wq_txt, wq_img, rope_cos,
                          rope_sin, s_txt, eps, stream, true);
}

#if DRAG_EXP
// workgroups per XCD of the persistent attention kernel
static int persist_slots() {
  const int opt = drag_opt(DRAG_OPT_ATTN_PERSIST);
  if (opt >= 3) return opt;           // (1 = one per CU)
  const int ncu8 = drag_cu_count() / 8;
  return ncu8 > 0 ? ncu8 : 1;
}
#endif

// ---- the launches: attention_launch picks one of these; every instantiation is named once, below ----
using LaunchFn = int (*)(dim3 grid, int block, int lds, hipStream_t st, const AttnArgs& p);

// attention_d128_kernel<NW, ..., QP, ...> by schedule: "attn_sched" 0 | 1 | 2 (and above) = schedule 1 + pipelined row maxima, the product's |
// 3 in experiment builds = V^T fragments read a step ahead | row-major V (the product schedule only)
enum { D128_S0, D128_S1, D128_S1_PMAX, D128_S3, D128_VROW, D128_FORMS };
template <int NW, bool QP>
constexpr LaunchFn d128_forms[D128_FORMS] = {
    drag_launch<attention_d128_kernel<NW, 0, QP, false>>, drag_launch<attention_d128_kernel<NW, 1, QP, false>>, drag_launch<attention_d128_kernel<NW, 1, QP, true>>,
    drag_launch<attention_d128_kernel<NW, DRAG_EXP ? 2 : 1, QP, true>>,      // (product builds: the D128_S1_PMAX entry again; never looked up there)
    drag_launch<attention_d128_kernel<NW, 1, QP, true, true>>};
static const LaunchFn* d128_form(bool w8, bool qprep) {
  return w8 ? (qprep ? d128_forms<8, true> : d128_forms<8, false>) : (qprep ? d128_forms<4, true> : d128_forms<4, false>);
}
// (what bench.py's roofline prints for this family: block size and q preparation only)
static const char* d128_name(bool w8, bool qprep) {
  return w8 ? (qprep ? "attention_d128_kernel<8, ..., true, ...>" : "attention_d128_kernel<8, ..., false, ...>")
            : (qprep ? "attention_d128_kernel<4, ..., true, ...>" : "attention_d128_kernel<4, ..., false, ...>");
}

// a 64-query kernel: its launch and its name, written once
struct Q64Kernel { LaunchFn launch; const char* name; };
#define DRAG_Q64(...) Q64Kernel{drag_launch<__VA_ARGS__>, #__VA_ARGS__}
#if DRAG_EXP
// "attn_gen" = 11 .. 29: schedule variants 1 .. 19 of the fold form
#define DRAG_AQV_LAUNCH(V_) DRAG_Q64(attention_q64g_kernel<true, true, V_>),
static const Q64Kernel q64g_variants[19] = {DRAG_ATTN_Q64G_VARIANTS(DRAG_AQV_LAUNCH)};
#undef DRAG_AQV_LAUNCH
#endif
// the 64-query kernel a call over S keys takes.  "attn_gen": 0 = policy — the generated stream (attention_q64g_kernel) whenever the tiles
// pair up, FOLD with the fused q preparation; 1 = never (attention_q64_kernel); 2 = the generated stream WITHOUT the fold (same bits as
// attention_q64_kernel: tests, A/B)
static Q64Kernel q64_kernel(int32_t S, bool qprep) {
  const int gen = drag_opt(DRAG_OPT_ATTN_GEN);
  if (!attention_generated(S)) return qprep ? DRAG_Q64(attention_q64_kernel<true>) : DRAG_Q64(attention_q64_kernel<false>);
  if (!qprep) return DRAG_Q64(attention_q64g_kernel<false, false>);
#if DRAG_EXP
  if (gen >= 11 && gen <= 29) return q64g_variants[gen - 11];
#endif
  return gen != 2 ? DRAG_Q64(attention_q64g_kernel<true, true>) : DRAG_Q64(attention_q64g_kernel<true, false>);
}
#undef DRAG_Q64

// the kernel the next launch of that shape takes under the current switches, as a profiler prints it — for callers that account launches
// per kernel (asked BEFORE the launch: what the launch is about to read is what gets reported)
extern "C" const char* drag_attention_bf16_kernel_name(int32_t S, int32_t v_row_major, int32_t q_prep) {
  bool w8, q64;
  attention_family(S, v_row_major != 0, w8, q64);
  return q64 ? q64_kernel(S, q_prep != 0).name : d128_name(w8, q_prep != 0);
}

static int attention_launch(const void* q, const void* k, const void* vt, void* out, int32_t B, int32_t S, int32_t H,
                            int32_t ld_qk, int64_t qk_batch_stride, int32_t ld_o, int64_t o_batch_stride, float scale,
                            const void* wq_txt, const void* wq_img, const float* rope_cos, const float* rope_sin, int32_t s_txt,
                            float eps, void* stream, bool vrow) {
  DRAG_CHECK(q && k && vt && out, "drag_attention_bf16: null pointer");
  DRAG_CHECK(B > 0 && S > 0 && H > 0, "drag_attention_bf16: bad shape");
  DRAG_CHECK(ld_qk % 8 == 0 && ld_o % 4 == 0, "drag_attention_bf16: ld_qk %% 8, ld_o %% 4 required");
  // (the prep entry points' analogue is ld >= 3 H 128: a row holds every head; shorter output rows would overlap)
  DRAG_CHECK(ld_qk >= H * 128, "drag_attention_bf16: ld_qk >= H * 128 required");
  DRAG_CHECK(ld_o >= H * 128, "drag_attention_bf16: ld_o >= H * 128 required");
  AttnArgs p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.vt = (const bf16_t*)vt; p.v = (const bf16_t*)vt; p.out = (bf16_t*)out;
  p.B = B; p.S = S; p.H = H; p.ld_qk = ld_qk; p.ld_o = ld_o; p.s_pad = (S + 63) / 64 * 64;
  p.qk_bs = qk_batch_stride; p.o_bs = o_batch_stride;
  p.c = scale * 1.4426950408889634f;
  p.wq_txt = (const bf16_t*)wq_txt; p.wq_img = (const bf16_t*)wq_img; p.cosT = rope_cos; p.sinT = rope_sin;
  p.s_txt = s_txt; p.eps = eps;
  const long long kspan = ((long long)(S - 1) * ld_qk + 128) * 2;
  const long long vspan = (long long)128 * p.s_pad * 2;
  DRAG_CHECK(kspan < (1ll << 31), "drag_attention_bf16: K span must be < 2 GiB per (batch, head)");
  p.k_bytes = (unsigned)kspan; p.vt_bytes = (unsigned)vspan;
  const long long kall = ((long long)(B - 1) * qk_batch_stride + (H - 1) * 128) * 2 + kspan, vall = (long long)B * H * vspan;
  // (whole-tensor spans: only the persistent experiment addresses through them — its launch condition below checks they fit 32 bits)
  const bool fits32 = kall < (1ll << 32) && vall < (1ll << 32);
  p.k_bytes_all = fits32 ? (unsigned)kall : 0u; p.vt_bytes_all = fits32 ? (unsigned)vall : 0u;
  const int groups = (B * H + 7) / 8;
  bool w8, q64;
  attention_family(S, vrow, w8, q64);
  const int QB = (w8 || q64) ? 256 : 128;
  const int nqb2 = (S + QB - 1) / QB;
  const dim3 grid(8 * groups * nqb2);
  const int sched = drag_opt(DRAG_OPT_ATTN_SCHED);          // 0, 1, or 2 = schedule 1 + pipelined row maxima
  const bool qprep = wq_txt != nullptr;
  p.tune = drag_opt(DRAG_OPT_ATTN_TUNE);
  if (ld_o % 8 != 0 || ((uintptr_t)out & 15) != 0 || o_batch_stride % 8 != 0) p.tune &= ~2;     // 16-byte stores need 16-byte aligned rows
  const hipStream_t st = (hipStream_t)stream;
  LaunchFn fn;
  dim3 lgrid = grid;
  int block = w8 ? 512 : 256, lds = 0;
  if (vrow) {                   // row-major V: the product schedule only (SCHED 1 + PMAX)
    fn = d128_form(w8, qprep)[D128_VROW];
  } else if (q64) {
    // 64 KiB of tiles + 64 KiB for the q rows of the next item (LDS-DMA).  One workgroup per CU walks the items (persistent) when every
    // item exists (B * H a multiple of 8) and the tiles pair up (an even number, >= 4: the stream's last two tiles stage for the next item);
    // otherwise, and under "attn_walk" = 2, one item per workgroup
    const int ncu64 = (drag_cu_count() & ~7) ? (drag_cu_count() & ~7) : 8;
    p.items = (int)grid.x;
    const int nkv64 = p.s_pad / 64;
    const int popt = drag_opt(DRAG_OPT_ATTN_WALK);             // 0 policy | 2 one item per workgroup | n >= 8 (a multiple of 8): n workgroups (tests: many items each)
    const int pgrid = popt >= 8 && popt % 8 == 0 ? popt : ncu64;
    // (a forced grid also walks items whose tiles do not pair up: each item then stages its own first tiles behind a barrier — tests)
    const bool walk = popt != 2 && (B * H) % 8 == 0 && (popt >= 8 || (nkv64 % 2 == 0 && nkv64 >= 4)) && p.items > pgrid;
    lgrid = dim3(walk ? (unsigned)pgrid : grid.x);
    block = 256;
    lds = 2 * KT_BYTES + 2 * VT_BYTES + 4 * 16384;
    fn = q64_kernel(S, qprep).launch;
#if DRAG_EXP
  } else if (w8 && sched == 2 && drag_opt(DRAG_OPT_ATTN_PERSIST) != 0 && fits32 && (B * H) % 8 == 0 && (p.s_pad / 64) % 2 == 0 &&
             nqb2 * groups > persist_slots()) {
    // EXPERIMENT, off by default ("attn_persist": 0 = off, 1 = one workgroup per CU, n >= 3 = n workgroups per XCD — tests: many items
    // per workgroup): the persistent form, whose K / V^T stream runs on across a workgroup's items (the KV loop is unrolled by two: an
    // even number of tiles keeps the buffer parity across items).  Same bits either way.  Measured same-box, interleaved
    // (scripts/ab_attn_persist.py, B=8 S=5337): 2592 vs 2571 us with the q preparation, 2523 vs 2499 us without — 1 % SLOWER: what a
    // workgroup pays outside its KV loop (6 us plain, 11-12 us with the q preparation) is the round trip + ingest of its Q rows and
    // RoPE table rows (256 KiB per workgroup through one CU's ~100 GB/s global-load path), not the first K / V^T tiles nor the
    // dispatch; and the hardware already overlaps the seams of one-item workgroups (a CU holds two of them by LDS and registers, so
    // the next workgroup's waves start on SIMDs as the old one's retire), which a single persistent workgroup cannot do.
    lgrid = dim3(8 * persist_slots());
    fn = qprep ? drag_launch<attention_d128_kernel<8, 1, true, true, false, true>> : drag_launch<attention_d128_kernel<8, 1, false, true, false, true>>;
#endif  // DRAG_EXP
  } else {
    fn = d128_form(w8, qprep)[DRAG_EXP && sched == 3 ? D128_S3 : sched >= 2 ? D128_S1_PMAX : sched == 1 ? D128_S1 : D128_S0];
  }
  return fn(lgrid, block, lds, st, p);
}
