"""The five kernels of csrc/textenc.hip, each through its ops wrapper, against the float64 restatements of tests/helpers/textenc_ref.py
(themselves held to the upstream modules by tests/test_textenc_restatements_host.py): every argument combination the attention accepts,
strided sources and destinations with a sentinel around what is written, the sequence lengths at which the kernel's structure changes,
inputs whose answer is known bit for bit, adversarial inputs, every bf16 value through the activations, second trips of the grid-stride
loops, and the refusals.  Numeric comparisons use bf16_bar.bar / bar_rows as they stand; structural ones are torch.equal."""
import itertools
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import textenc_ref as ref  # noqa: E402
from bf16_bar import bar, bar_rows  # noqa: E402

SENTINEL = 777.0
FORMS = {"eager_t5": dict(eager=True, causal=False, bias=True, scale=1.0), "sdpa_clip": dict(eager=False, causal=True, bias=False, scale=0.125)}


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


def _rel_table(H, S, g):
    return torch.randn(H, 2 * S - 1, generator=g).bfloat16()


def _attend(gpu, qkv, B, S, H, rel, causal, eager, scale):
    """dense fused [B, S, 3 * H * 64] rows through the kernel -> [B, S, H * 64] on the host"""
    from domain_rag_amd import ops
    D = H * 64
    d = qkv.to(gpu)
    out = torch.full((B, S, D), SENTINEL, dtype=torch.bfloat16, device=gpu)
    ops.textenc_attention(d, d[..., D:], d[..., 2 * D:], out, B, S, H, ld=3 * D, batch_stride=S * 3 * D, scale=scale,
                          rel_bias=None if rel is None else rel.to(gpu), causal=causal, eager=eager)
    return out.cpu()


# ------------------------------------------------------------------ attention: every combination, strided
@pytest.mark.parametrize("eager,causal,bias,scale", list(itertools.product([True, False], [True, False], [True, False], [1.0, 0.125])),
                         ids=lambda v: str(v))
def test_attention_every_combination_strided_with_sentinel(gpu, eager, causal, bias, scale):
    """q / k / v inside a fused buffer with ld = 3 D + 64 and eight rows between the batches (NaN wherever no operand lies: a read outside
    the operands shows in the output), the output into a wider, taller destination whose every other element must keep its sentinel"""
    from domain_rag_amd import ops
    g = torch.Generator().manual_seed(100 + 8 * eager + 4 * causal + 2 * bias + (scale == 1.0))
    eqs = []
    for S, B, H in ((33, 2, 3), (129, 1, 2)):
        D = H * 64
        ld = 3 * D + 64
        bs = S * ld + 8 * ld
        ld_o, obs = D + 24, (S + 2) * (D + 24)
        buf = torch.full((B, S + 8, ld), math.nan).bfloat16()
        buf[:, :S, :3 * D] = (torch.randn(B, S, 3 * D, generator=g) * (0.35 if eager or scale == 1.0 else 1.0)).bfloat16()
        buf = buf.view(-1)
        rel = _rel_table(H, S, g) if bias else None
        out0 = torch.full((B * obs,), SENTINEL).bfloat16()
        dbuf, out = buf.to(gpu), out0.to(gpu)
        ops.textenc_attention(dbuf, dbuf[D:], dbuf[2 * D:], out, B, S, H, ld=ld, batch_stride=bs, scale=scale,
                              rel_bias=None if rel is None else rel.to(gpu), causal=causal, eager=eager, ld_o=ld_o, o_batch_stride=obs)
        full, rows = ref.attention_strided(buf, 0, D, 2 * D, B, S, H, ld, bs, rel, causal, eager, scale, out0, ld_o, obs)
        got = out.cpu()
        got_rows = got[ref.row_index(B, S, D, ld_o, obs)]
        assert bool(torch.isfinite(got_rows.float()).all())
        eqs.append(bar(got_rows, rows, f"attention eager={eager} causal={causal} bias={bias} scale={scale} S={S}"))
        outside = torch.ones(B * obs, dtype=torch.bool)
        outside[ref.row_index(B, S, D, ld_o, obs).reshape(-1)] = False
        assert torch.equal(got[outside], full[outside]) and bool((got[outside] == SENTINEL).all()), "the kernel wrote outside its [S, D] blocks"
    print("equal fractions", eqs)


@pytest.mark.parametrize("causal,bias", [(False, True), (True, False)], ids=["bias", "causal"])
def test_attention_eager_rounds_the_scaled_logit(gpu, causal, bias):
    """eager's bf16(bf16(q.k) * scale): with scale 0.125, a power of two, that second rounding changes nothing and a kernel without it
    passes every other test here.  scale = float32(0.3) makes it count: the restatement without it is equal on 30 % of these outputs"""
    S, B, H = 77, 2, 2
    scale = float(torch.tensor(0.3, dtype=torch.float32))
    g = torch.Generator().manual_seed(71 + causal)
    qkv = torch.randn(B, S, 3 * H * 64, generator=g).bfloat16()
    rel = _rel_table(H, S, g) if bias else None
    got = _attend(gpu, qkv, B, S, H, rel, causal, True, scale)
    want = ref.attention_f64(qkv, B, S, H, rel, causal, True, scale)
    print("equal fractions", [bar(got, want, f"eager scale 0.3 causal={causal} bias={bias}")])


# ------------------------------------------------------------------ attention: sequence edges
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("S", [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 129, 512])
def test_attention_sequence_edges(gpu, S, form):
    """16 queries per wave, 64 per workgroup, 16-key tiles in pass 1, 32-key steps in pass 2, the causal kend = min(S, q0 + 16)"""
    f = FORMS[form]
    B, H = 2, 2
    g = torch.Generator().manual_seed(1000 + S + (500 if f["eager"] else 0))
    qkv = (torch.randn(B, S, 3 * H * 64, generator=g) * (0.35 if f["eager"] else 1.0)).bfloat16()
    rel = _rel_table(H, S, g) if f["bias"] else None
    got = _attend(gpu, qkv, B, S, H, rel, f["causal"], f["eager"], f["scale"])
    want = ref.attention_f64(qkv, B, S, H, rel, f["causal"], f["eager"], f["scale"])
    print("equal fractions", [bar(got, want, f"attention {form} S={S}")])


# ------------------------------------------------------------------ attention: exact answers
@pytest.mark.parametrize("eager,causal", [(True, False), (True, True), (False, True), (False, False)],
                         ids=["eager_full", "eager_causal", "sdpa_causal", "sdpa_full"])
@pytest.mark.parametrize("S", [17, 64, 77, 512])
def test_attention_one_hot_keys_exact(gpu, S, eager, causal):
    """query i's logits are largest at key pi(i) by 128: every other weight is expf(-128) = 0 and the output is v[pi(i)], bit for bit.  A V
    operand gathered in another key order than P's, at any of a step's 32 positions, gives another row of v"""
    scale = 1.0 if eager else 0.125
    B, H = 2, 2
    for name, pi in ref.onehot_perms(S, causal, S).items():
        qkv, expected = ref.onehot_inputs(S, B, H, pi, scale, S + 1)
        rel = torch.zeros(H, 2 * S - 1).bfloat16() if eager else None
        got = _attend(gpu, qkv, B, S, H, rel, causal, eager, scale)
        wrong = (_bits(got) != _bits(expected)).any(-1)
        assert torch.equal(_bits(got), _bits(expected)), (f"S={S} eager={eager} causal={causal} pi={name}: {int(wrong.sum())} rows are not v[pi(i)], "
                                                          f"first (batch, query) {wrong.nonzero()[:4].tolist()}")


@pytest.mark.parametrize("eager", [True, False], ids=["eager", "sdpa_bias"])
@pytest.mark.parametrize("S", [16, 77, 512])
def test_attention_toeplitz_index_exact(gpu, S, eager):
    """q = 0 and a table that is 0 at one offset d_h and -128 elsewhere: row i is v[i + d_h] exactly wherever that key exists (d_h =
    -(S-1), -1, 0, +1, S-1 across the heads: both ends of rel[key - query + S - 1]); the other rows see all keys alike and meet the bar"""
    B = 2
    scale = 1.0 if eager else 0.125
    qkv, rel, expected, exact = ref.toeplitz_inputs(S, B, S)
    H = rel.shape[0]
    got = _attend(gpu, qkv, B, S, H, rel, False, eager, scale).view(B, S, H, 64)
    mask = exact.t()[None].expand(B, S, H)
    assert torch.equal(_bits(got[mask]), _bits(expected.view(B, S, H, 64)[mask])), f"S={S} eager={eager}: a row with one visible key is not that v row"
    want = ref.attention_f64(qkv, B, S, H, rel, False, eager, scale).view(B, S, H, 64)
    if bool((~mask).any()):
        print("equal fractions", [bar(got[~mask], want[~mask], f"uniform rows S={S} eager={eager}")])


# ------------------------------------------------------------------ attention: adversarial
def _finite_bar(got, want, what):
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    return bar(got, want, what)


@pytest.mark.parametrize("form", list(FORMS))
def test_attention_hot_key_at_each_position_of_a_step(gpu, form):
    """S = 96: the middle 32-key step of three; batch b's key 32 + b outweighs all others by e^64.  Inputs on a dyadic grid (ref.dyadic)"""
    f = FORMS[form]
    S, B, H = 96, 32, 1
    g = torch.Generator().manual_seed(31 + f["eager"])
    x = ref.dyadic(torch.randn(B, S, 3, 64, generator=g)).float()
    q0, k0 = (2.0, 32.0) if f["eager"] else (8.0, 64.0)                       # q0 * k0 * scale = 64
    x[:, :, 0, 0] = q0
    x[torch.arange(B), 32 + torch.arange(B), 1, 0] = k0
    qkv = x.bfloat16().view(B, S, 192)
    rel = _rel_table(H, S, g) if f["bias"] else None
    got = _attend(gpu, qkv, B, S, H, rel, f["causal"], f["eager"], f["scale"])
    want = ref.attention_f64(qkv, B, S, H, rel, f["causal"], f["eager"], f["scale"])
    v = qkv.view(B, S, 3, 64)[torch.arange(B), 32 + torch.arange(B), 2]                        # the hot keys' v rows
    assert bool(((want[:, -1].float() - v.float()).abs().max(-1).values < 0.05).all())         # the last query does see little else
    print("equal fractions", [_finite_bar(got, want, f"hot key, {form}")])


@pytest.mark.parametrize("eager,causal", [(True, False), (True, True), (False, True), (False, False)],
                         ids=["eager_full", "eager_causal", "sdpa_causal", "sdpa_full"])
def test_attention_all_scores_equal(gpu, eager, causal):
    """q = 0.5 and k = 0.25 everywhere: every logit is 8 and the output is the mean of the visible v rows"""
    S, B, H = 77, 2, 2
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, S, 3, H, 64, generator=g)
    x[:, :, 0], x[:, :, 1] = 0.5, 0.25
    qkv = x.bfloat16().view(B, S, 3 * H * 64)
    scale = 1.0 if eager else 0.125
    got = _attend(gpu, qkv, B, S, H, None, causal, eager, scale)
    want = ref.attention_f64(qkv, B, S, H, None, causal, eager, scale)
    if not eager:                                        # SDPA's weights are exactly 1: the restatement IS the mean, rounded once
        v = qkv.view(B, S, 3, H, 64)[:, :, 2].double()
        mean = v.cumsum(1) / torch.arange(1, S + 1)[None, :, None, None] if causal else v.mean(1, keepdim=True).expand(B, S, H, 64)
        bar(want, ref.to_bf16(mean).view(B, S, H * 64), "restatement vs the mean of the visible rows")
    print("equal fractions", [_finite_bar(got, want, f"equal scores eager={eager} causal={causal}")])


@pytest.mark.parametrize("causal,bias,scale", [(False, True, 1.0), (True, False, 0.125)], ids=["bias", "causal_scaled"])
def test_attention_eager_logits_in_the_thousands(gpu, causal, bias, scale):
    """integer q and k up to +-31: q.k reaches a few thousand, is exact in float32 and is rounded to bf16 (16 to the ulp) before anything else"""
    S, B, H = 77, 2, 2
    g = torch.Generator().manual_seed(51)
    x = torch.randn(B, S, 3, H, 64, generator=g)
    x[:, :, :2] = ref.dyadic(x[:, :, :2] * 12, 1.0, 31.0).float()
    qkv = x.bfloat16().view(B, S, 3 * H * 64)
    s = torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0].double(), x[:, :, 1].double())
    assert 2000 < s.abs().max().item() < 2 ** 24 / 64
    rel = _rel_table(H, S, g) if bias else None
    got = _attend(gpu, qkv, B, S, H, rel, causal, True, scale)
    want = ref.attention_f64(qkv, B, S, H, rel, causal, True, scale)
    print("equal fractions", [_finite_bar(got, want, f"large logits causal={causal} bias={bias} scale={scale}")])


@pytest.mark.parametrize("form", list(FORMS))
def test_attention_outlier_channel(gpu, form):
    """one head dim of q and k at 100 x the others (on the dyadic grid: its products reach 40 000 and still sum exactly in float32)"""
    f = FORMS[form]
    S, B, H = 77, 2, 2
    g = torch.Generator().manual_seed(61 + f["eager"])
    x = torch.randn(B, S, 3, H, 64, generator=g)
    x[:, :, :2] = ref.dyadic(x[:, :, :2]).float()
    x[:, :, :2, :, 5] *= 100.0
    qkv = x.bfloat16().view(B, S, 3 * H * 64)
    rel = _rel_table(H, S, g) if f["bias"] else None
    got = _attend(gpu, qkv, B, S, H, rel, f["causal"], f["eager"], f["scale"])
    want = ref.attention_f64(qkv, B, S, H, rel, f["causal"], f["eager"], f["scale"])
    print("equal fractions", [_finite_bar(got, want, f"outlier channel, {form}")])


# ------------------------------------------------------------------ attention: refusals
def test_attention_refusals(gpu):
    from domain_rag_amd import ops
    B, S, H = 2, 8, 2
    D = H * 64
    ld = 3 * D
    bf = dict(dtype=torch.bfloat16, device=gpu)
    buf = torch.zeros(B * S * ld + 16, **bf)
    out = torch.full((B * S * D,), SENTINEL, **bf)
    rel = torch.zeros(H, 2 * S - 1, **bf)

    def call(q=buf, k=buf[D:], v=buf[2 * D:], o=out, S=S, ld=ld, bs=None, rel_bias=None):
        ops.textenc_attention(q, k, v, o, B, S, H, ld=ld, batch_stride=S * ld if bs is None else bs, scale=1.0, rel_bias=rel_bias, eager=True)

    call(rel_bias=rel)                                    # the arguments the refusals below depart from are accepted
    out.fill_(SENTINEL)
    with pytest.raises(RuntimeError, match=r"S must be in \[1, 512\]"):
        call(S=0, bs=0)
    big = torch.zeros(B * 513 * ld, **bf)
    with pytest.raises(RuntimeError, match=r"S must be in \[1, 512\]"):
        call(q=big, k=big[D:], v=big[2 * D:], o=torch.empty(B * 513 * D, **bf), S=513)
    wide = torch.zeros(B * S * (ld + 4), **bf)
    with pytest.raises(RuntimeError, match=r"ld % 8 == 0"):
        call(q=wide, k=wide[D:], v=wide[2 * D:], ld=ld + 4)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(q=buf[4:])
    span = (B - 1) * S * ld + (S - 1) * ld + D
    for name in ("q", "k", "v"):
        with pytest.raises(ValueError, match=rf"textenc_attention\.{name}: .* do not fit the buffer"):
            call(**{name: torch.zeros(span - 1, **bf)})
    call(q=torch.zeros(span, **bf), k=torch.zeros(span, **bf), v=torch.zeros(span, **bf))          # exactly span elements is enough
    out.fill_(SENTINEL)
    with pytest.raises(ValueError, match="output rows do not fit"):
        call(o=torch.empty(B * S * D - 1, **bf))
    with pytest.raises(ValueError, match=r"rel_bias: expected a contiguous \[2, 15\] table"):
        call(rel_bias=torch.zeros(H, 2 * S, **bf))
    with pytest.raises(ValueError, match=r"rel_bias: expected a contiguous \[2, 15\] table"):
        call(rel_bias=torch.zeros(2 * S - 1, H, **bf).t())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------ T5 RMSNorm
def _rmsnorm(gpu, x, w, tail=4):
    """x [M, D] through the kernel into the head of a taller destination: (rows [M, D], the tail rows) on the host"""
    from domain_rag_amd import ops
    M, D = x.shape
    full = torch.full((M + tail, D), SENTINEL, dtype=torch.bfloat16, device=gpu)
    ops.t5_rmsnorm(x.to(gpu), w.to(gpu), full[:M], 1e-6)
    return full[:M].cpu(), full[M:].cpu()


@pytest.mark.parametrize("D", [8, 64, 520, 768, 4088, 4096])
def test_rmsnorm_widths_and_row_counts(gpu, D):
    """D = 8: one lane; 520 / 4088: a 512-wide iteration that a few lanes fill; M = 1, 5: a workgroup with idle waves"""
    g = torch.Generator().manual_seed(70 + D)
    w = ref.rms_weight(D, D + 1)
    eqs = []
    for M in (1, 4, 5, 37):
        x = (3.0 * torch.randn(M, D, generator=g)).bfloat16()
        got, tail = _rmsnorm(gpu, x, w)
        eqs.append(bar_rows(got, ref.t5_layernorm(x, w, 1e-6), f"T5 RMSNorm D={D} M={M}"))
        assert bool((tail == SENTINEL).all()), f"D={D} M={M}: rows behind the last one were written"
    print("equal fractions", eqs)


def test_rmsnorm_no_rows_and_refusals(gpu):
    from domain_rag_amd import ops
    bf = dict(dtype=torch.bfloat16, device=gpu)
    full = torch.full((4, 768), SENTINEL, **bf)
    ops.t5_rmsnorm(torch.empty(0, 768, **bf), torch.ones(768, **bf), full[:0], 1e-6)       # M = 0: accepted, nothing written
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all())
    for D in (4104, 12):
        with pytest.raises(RuntimeError, match=r"need D % 8 == 0 and 8 <= D <= 4096"):
            ops.t5_rmsnorm(torch.zeros(4, D, **bf), torch.ones(D, **bf), torch.empty(4, D, **bf), 1e-6)
        with pytest.raises(RuntimeError, match=r"need D % 8 == 0 and 8 <= D <= 4096"):        # ... with no rows as well
            ops.t5_rmsnorm(torch.zeros(0, D, **bf), torch.ones(D, **bf), torch.empty(0, D, **bf), 1e-6)


def test_rmsnorm_rows_of_a_workgroup_stay_separate(gpu):
    """twelve rows, three workgroups of four waves: zero, subnormal, one-hot, overflowing, NaN and inf rows between Gaussian ones.  A
    statistic that leaked from a neighbour would turn a finite row non-finite, or move it past the bar"""
    D = 768
    x, kinds = ref.rms_block(D, 7)
    w = ref.rms_weight(D, D + 1)
    assert bool((w == 0).any()) and bool((w < 0).any())
    got, tail = _rmsnorm(gpu, x, w)
    want = ref.t5_layernorm(x, w, 1e-6)
    assert bool((tail == SENTINEL).all())
    eqs = {}
    for r, kind in enumerate(kinds):
        finite_row = bool(torch.isfinite(want[r].float()).all())
        assert finite_row == (kind not in ("nan at column 0", "+inf at the last column"))
        if finite_row:
            assert bool(torch.isfinite(got[r].float()).all()), f"row {r} ({kind}) holds a NaN or inf that is not its own"
        eqs[f"{r} {kind}"] = bar_rows(got[r:r + 1], want[r:r + 1], f"row {r} ({kind})")     # specials: value for value
    print("equal fractions", eqs)


# ------------------------------------------------------------------ gated NewGELU
def _gated(gpu, h):
    from domain_rag_amd import ops
    M, F = h.shape[0], h.shape[1] // 2
    out = torch.full((M, F), SENTINEL, dtype=torch.bfloat16, device=gpu)
    ops.gated_new_gelu(h.to(gpu), out)
    return out.cpu()


def test_gated_new_gelu_every_bf16_value(gpu):
    """every bf16 value through the eight roundings of the chain, against the gates 1, -1, 0.3, 3e38 and 0; then the same values in rows
    of two binades each, where the allowance is of that row's largest output"""
    h = ref.gated_all_values()
    eqs = [bar_rows(_gated(gpu, h), ref.gated_new_gelu(h), "gated NewGELU, all bf16 values x 5 gates")]
    a = ref.patterns_by_high_byte()
    for gate in (1.0, 0.3):
        hb = torch.cat([a, torch.full_like(a, gate)], dim=1).contiguous()
        eqs.append(bar_rows(_gated(gpu, hb), ref.gated_new_gelu(hb), f"gated NewGELU by binade rows, gate {gate}"))
    print("equal fractions", eqs)


def test_gated_new_gelu_shapes(gpu):
    """F = 8: one vector per row (row = i / 1); F8 = 3 with a thousand rows; F8 = 1281"""
    g = torch.Generator().manual_seed(81)
    eqs = []
    for M, F in ((3, 8), (1000, 24), (5, 10248)):
        h = (4.0 * torch.randn(M, 2 * F, generator=g)).bfloat16()
        eqs.append(bar_rows(_gated(gpu, h), ref.gated_new_gelu(h), f"gated NewGELU M={M} F={F}"))
    print("equal fractions", eqs)
    assert _gated(gpu, torch.empty(0, 16, dtype=torch.bfloat16)).shape == (0, 8)           # no rows: accepted
    with pytest.raises(RuntimeError, match=r"need F % 8 == 0"):
        _gated(gpu, torch.zeros(4, 24, dtype=torch.bfloat16))


def test_gated_new_gelu_second_trip(gpu):
    """M * F / 8 = 2049 * 1025 = 2 100 225 vectors, 3073 more than 8192 workgroups of 256 lanes take in one trip: the loop's second trip,
    with F8 = 1025 no power of two and a last workgroup of one lane"""
    M, F = 2049, 8200
    assert ref.N8_FIRST_TRIP < M * F // 8 < ref.N8_FIRST_TRIP + 256 * 16 and (M * F // 8) % 256 == 1
    g = torch.Generator().manual_seed(82)
    h = (2.0 * torch.randn(M, 2 * F, generator=g)).bfloat16()
    got = _gated(gpu, h)
    want = ref.gated_new_gelu(h, lut=True)
    eq = bar(got, want, "gated NewGELU, second trip")
    first_row = ref.N8_FIRST_TRIP * 8 // F                                    # the row in which the second trip begins
    eq_tail = bar_rows(got[first_row:], want[first_row:], "gated NewGELU, the rows of the second trip")
    eq_last = bar_rows(got[-1:], want[-1:], "gated NewGELU, the last row")
    print("equal fractions", [eq, eq_tail, eq_last])


# ------------------------------------------------------------------ QuickGELU
def test_quick_gelu_every_bf16_value_in_place_and_not(gpu):
    from domain_rag_amd import ops
    x = ref.all_bf16_patterns()
    want = ref.quick_gelu(x)
    d = x.to(gpu)
    out = ops.quick_gelu(d)
    assert torch.equal(_bits(d), _bits(x)), "the allocating form changed its input"
    eq = bar_rows(out.cpu()[None], want[None], "QuickGELU, all bf16 values")
    xb = ref.patterns_by_high_byte()
    eqb = bar_rows(ops.quick_gelu(xb.to(gpu)).cpu(), ref.quick_gelu(xb), "QuickGELU by binade rows")
    same = ops.quick_gelu(d, d)                          # in place, as ClipTextHIP calls it
    assert same is d and torch.equal(_bits(d), _bits(out)), "in place differs from out of place"
    other = torch.full((65536,), SENTINEL, dtype=torch.bfloat16, device=gpu)
    assert ops.quick_gelu(x.to(gpu), other) is other and torch.equal(_bits(other), _bits(out))
    print("equal fractions", [eq, eqb])


def test_quick_gelu_second_trip_and_sizes(gpu):
    from domain_rag_amd import ops
    n8 = ref.N8_FIRST_TRIP + 301
    g = torch.Generator().manual_seed(91)
    x = (2.0 * torch.randn(n8 * 8, generator=g)).bfloat16()
    want = ref.quick_gelu(x, lut=True)
    full = torch.full((n8 * 8 + 64,), SENTINEL, dtype=torch.bfloat16, device=gpu)
    ops.quick_gelu(x.to(gpu), full[:n8 * 8])
    got = full.cpu()
    eq = bar(got[:n8 * 8], want, "QuickGELU, second trip")
    eq_tail = bar(got[ref.N8_FIRST_TRIP * 8:n8 * 8], want[ref.N8_FIRST_TRIP * 8:], "QuickGELU, the 301 vectors of the second trip")
    assert bool((got[n8 * 8:] == SENTINEL).all())
    print("equal fractions", [eq, eq_tail])
    d = x[:n8 * 8].to(gpu)                               # in place on the second trip as well
    ops.quick_gelu(d, d)
    assert torch.equal(_bits(d), _bits(got[:n8 * 8]))
    empty = torch.empty(0, dtype=torch.bfloat16, device=gpu)
    assert ops.quick_gelu(empty).numel() == 0             # n = 0: accepted
    with pytest.raises(RuntimeError, match=r"need n % 8 == 0"):
        ops.quick_gelu(torch.zeros(12, dtype=torch.bfloat16, device=gpu))


# ------------------------------------------------------------------ embedding gather
@pytest.mark.parametrize("D", [8, 768])
def test_embed_gather_edge_ids(gpu, D):
    """ids 0 and V - 1, and -1, V, 2^40, int64 min among valid ones: a zero row (pos[s] with pos), never a read outside the table"""
    from domain_rag_amd import ops
    V, B, S = 1000, 3, 77
    g = torch.Generator().manual_seed(D)
    table = torch.randn(V, D, generator=g).bfloat16()
    pos = torch.randn(S, D, generator=g).bfloat16()
    ids, bad = ref.gather_ids(B, S, V, 3)
    full = torch.full((B * S + 3, D), SENTINEL, dtype=torch.bfloat16, device=gpu)
    out = full[:B * S]
    ops.embed_gather(ids.to(gpu), table.to(gpu), out)
    got = out.cpu()
    assert torch.equal(got, ref.embed_gather(ids, table))
    assert bool((got.view(B, S, D)[bad] == 0).all()) and torch.equal(got.view(B, S, D)[~bad], table[ids[~bad]])
    ops.embed_gather(ids.to(gpu), table.to(gpu), out, pos=pos.to(gpu))
    got = out.cpu()
    assert torch.equal(got, ref.embed_gather(ids, table, pos))
    assert torch.equal(got.view(B, S, D)[bad], pos[None].expand(B, S, D)[bad])
    assert bool((full[B * S:] == SENTINEL).all())
    with pytest.raises(ValueError, match=rf"embed_gather\.pos: expected contiguous rows of {D} covering {S} positions"):
        ops.embed_gather(ids.to(gpu), table.to(gpu), out, pos=pos[:S - 1].to(gpu))
    ops.embed_gather(ids[:0].to(gpu), table.to(gpu), full[:0])                # no prompts: accepted, nothing written
    assert bool((full[B * S:] == SENTINEL).all())


def test_embed_gather_second_trip(gpu):
    """D = 8: one vector per row, B * S = 2 097 453 rows: 301 of them on the loop's second trip"""
    from domain_rag_amd import ops
    V, D, B = 1000, 8, 3
    S = (ref.N8_FIRST_TRIP + 301) // B
    assert B * S == ref.N8_FIRST_TRIP + 301
    g = torch.Generator().manual_seed(95)
    table = torch.randn(V, D, generator=g).bfloat16()
    ids = torch.randint(0, V, (B, S), generator=g)
    full = torch.full((B * S + 8, D), SENTINEL, dtype=torch.bfloat16, device=gpu)
    ops.embed_gather(ids.to(gpu), table.to(gpu), full[:B * S])
    got = full.cpu()
    assert torch.equal(got[:B * S], table[ids].view(-1, D))
    assert torch.equal(got[ref.N8_FIRST_TRIP:B * S], table[ids.view(-1)[ref.N8_FIRST_TRIP:]])       # the second trip's rows on their own
    assert bool((got[B * S:] == SENTINEL).all())
