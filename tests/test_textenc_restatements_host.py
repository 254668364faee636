"""tests/helpers/textenc_ref.py without a GPU: the float64 restatements that tests/test_gpu_textenc_kernels.py holds the kernels of
csrc/textenc.hip to are themselves held, at the same bar, to the upstream modules run on CPU bf16 tensors, on every bf16 value and on the
extreme rows the GPU tests use; and the exact-answer attention inputs give, through the restatement, exactly the V rows they promise."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import textenc_ref as ref  # noqa: E402
from bf16_bar import bar, bar_rows  # noqa: E402


def _upstream_ln(x, w, eps):
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    ln = T5LayerNorm(w.numel(), eps=eps)
    ln.weight.data = w.float()
    return ln.bfloat16()(x)


# ------------------------------------------------------------------ T5LayerNorm
def test_t5_layernorm_restatement_vs_upstream_on_every_bf16_value():
    x = ref.patterns_by_high_byte()
    w = ref.rms_weight(256, 1)
    want = ref.t5_layernorm(x, w, 1e-6)
    eq = bar_rows(_upstream_ln(x, w, 1e-6), want, "T5LayerNorm on CPU bf16 vs restatement, all bf16 values")
    # rows whose squares leave float32's range (exponent 2^64 and up) come out as zeros; the rows with inf / NaN as NaN
    assert bool((want[0x60:0x7F].float() == 0).all()) and bool(torch.isnan(want[0x7F].float()).all())
    print(f"T5LayerNorm, CPU bf16 vs restatement on all bf16 values: {eq:.4%} equal")


@pytest.mark.parametrize("D", [8, 64, 520, 768, 4088, 4096])
def test_t5_layernorm_restatement_vs_upstream_gaussian_and_extreme_rows(D):
    g = torch.Generator().manual_seed(D)
    w = ref.rms_weight(D, D + 1)
    x = (3.0 * torch.randn(37, D, generator=g)).bfloat16()
    eq = bar_rows(_upstream_ln(x, w, 1e-6), ref.t5_layernorm(x, w, 1e-6), f"T5LayerNorm CPU vs restatement, D={D}")
    xb, kinds = ref.rms_block(D, 7)
    want = ref.t5_layernorm(xb, w, 1e-6)
    eqb = bar_rows(_upstream_ln(xb, w, 1e-6), want, f"T5LayerNorm CPU vs restatement, extreme rows, D={D}")
    for r, kind in enumerate(kinds):
        row = want[r].float()
        if kind == "gaussian":
            assert bool(torch.isfinite(row).all()) and row.abs().max().item() > 0.5, (r, kind)
        elif kind in ("zero", "all 3e38"):
            assert bool((row == 0).all()), (r, kind)
        elif kind == "nan at column 0":
            assert bool(torch.isnan(row).all()), (r, kind)
        elif kind == "+inf at the last column":
            assert bool(torch.isnan(row[-1])) and bool((row[:-1] == 0).all()), (r, kind)
        elif kind == "subnormal":                          # rsqrt(eps) = 1000 lifts 2^-133 into the normal numbers
            nz = row[w.float() != 0].abs()
            assert bool((nz > 0).all()) and bool((nz < 2.0 ** -121).all()) and nz.max().item() > 2.0 ** -124, (r, kind)
        elif kind == "one hot 3e4":
            assert int((row != 0).sum()) == int(w[D // 3] != 0), (r, kind)
    print(f"T5LayerNorm D={D}: CPU bf16 vs restatement {eq:.4%} equal on Gaussian rows, {eqb:.4%} on the extreme block")


# ------------------------------------------------------------------ activations
def test_gated_new_gelu_restatement_vs_upstream_on_every_bf16_value():
    from transformers.activations import NewGELUActivation
    h = ref.gated_all_values()
    F = 65536
    want = ref.gated_new_gelu(h)
    up = NewGELUActivation()(h[:, :F]) * h[:, F:]
    eq = bar_rows(up, want, "NewGELU * gate on CPU bf16 vs restatement, all bf16 values")
    lut = ref.gated_new_gelu(h, lut=True)                  # the table form is the same function (a NaN's sign and payload aside)
    assert torch.equal(torch.isnan(lut), torch.isnan(want)) and torch.equal(lut[~torch.isnan(lut)].view(torch.int16), want[~torch.isnan(want)].view(torch.int16))
    # rows of two binades each: the allowance is of that row's largest output, not of 3e38
    a = ref.patterns_by_high_byte()
    eqs = [eq]
    for gate in (1.0, 0.3):
        hb = torch.cat([a, torch.full_like(a, gate)], dim=1)
        eqs.append(bar_rows(NewGELUActivation()(a) * hb[:, 256:], ref.gated_new_gelu(hb), f"NewGELU * {gate} by binade rows"))
    print("gated NewGELU, CPU bf16 vs restatement: equal shares", [f"{e:.4%}" for e in eqs])


def test_gated_new_gelu_restatement_vs_upstream_gaussian():
    from transformers.activations import NewGELUActivation
    g = torch.Generator().manual_seed(5)
    for M, F in ((3, 8), (1000, 24), (5, 10248)):
        h = (4.0 * torch.randn(M, 2 * F, generator=g)).bfloat16()
        bar_rows(NewGELUActivation()(h[:, :F]) * h[:, F:], ref.gated_new_gelu(h), f"NewGELU * gate CPU vs restatement M={M} F={F}")


def test_quick_gelu_restatement_vs_upstream_on_every_bf16_value():
    x = ref.all_bf16_patterns()
    want = ref.quick_gelu(x)
    eq = bar_rows((x * torch.sigmoid(1.702 * x))[None], want[None], "QuickGELU on CPU bf16 vs restatement, all bf16 values")
    xb = ref.patterns_by_high_byte()
    eqb = bar_rows(xb * torch.sigmoid(1.702 * xb), ref.quick_gelu(xb), "QuickGELU by binade rows")
    assert torch.equal(ref.quick_gelu(x, lut=True).view(torch.int16), want.view(torch.int16))
    f = want.float()
    assert bool(torch.isnan(f[x.float() == -math.inf]).all()) and bool((f[x.float() == math.inf] == math.inf).all())
    print(f"QuickGELU, CPU bf16 vs restatement: {eq:.4%} equal in one row, {eqb:.4%} by binade rows")


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("D", [8, 768])
def test_gather_restatement_vs_indexing(D):
    V, B, S = 1000, 3, 77
    g = torch.Generator().manual_seed(D)
    table = torch.randn(V, D, generator=g).bfloat16()
    pos = torch.randn(S, D, generator=g).bfloat16()
    ids, bad = ref.gather_ids(B, S, V, 3)
    assert int(bad.sum()) >= 8 and bool((ids == 0).any()) and bool((ids == V - 1).any())
    assert {-1, V, 2 ** 40, -2 ** 63} <= set(ids[bad].tolist())
    good = torch.where(bad, torch.zeros_like(ids), ids)
    want = torch.where(bad[..., None], torch.zeros((), dtype=torch.bfloat16), table[good])
    assert torch.equal(ref.embed_gather(ids, table), want.view(-1, D))
    assert torch.equal(ref.embed_gather(ids, table, pos), (want + pos[None]).view(-1, D))           # table[ids] + pos, torch's own bf16 sum
    assert torch.equal(ref.embed_gather(ids, table, pos).view(B, S, D)[bad], pos[None].expand(B, S, D)[bad])


# ------------------------------------------------------------------ attention: the exact-answer inputs
ONEHOT_S = (17, 64, 77, 512)
TOEPLITZ_S = (16, 77, 512)
MODES = {"eager": dict(eager=True, scale=1.0), "sdpa": dict(eager=False, scale=0.125)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("S", ONEHOT_S)
def test_one_hot_inputs_give_exactly_v_of_pi(S, causal, mode):
    m = MODES[mode]
    assert ref.onehot_alpha(1.0) == 64 and ref.onehot_alpha(0.125) == 512
    perms = ref.onehot_perms(S, causal, S)
    assert set(perms) == ({"identity", "lower"} if causal else {"identity", "lower", "reversal"})
    for name, pi in perms.items():
        qkv, expected = ref.onehot_inputs(S, 1, 2, pi, m["scale"], S + 1)
        rel = torch.zeros(2, 2 * S - 1).bfloat16() if m["eager"] else None
        got = ref.attention_f64(qkv, 1, S, 2, rel, causal, m["eager"], m["scale"])
        assert torch.equal(got, expected), f"S={S} {mode} causal={causal} pi={name}"
        # the margin, in the kernel's own float32 terms: the runner-up's weight is expf(-128) = 0
        x = qkv.double().view(1, S, 3, 2, 64)
        s = torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) * m["scale"]
        top = s.topk(2, dim=-1).values if S > 1 else None
        assert bool(((top[..., 0] - top[..., 1]) >= 128).all()) and bool((s.argmax(-1) == pi).all())
        assert bool((s == s.float().bfloat16().double()).all())                                    # every logit is a bf16 value: eager rounds nothing
    assert float(torch.exp(torch.tensor(-128.0, dtype=torch.float32))) == 0.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("S", TOEPLITZ_S)
def test_toeplitz_inputs_give_exactly_v_at_the_offset(S, mode):
    m = MODES[mode]
    qkv, rel, expected, exact = ref.toeplitz_inputs(S, 2, S)
    H = len(ref.toeplitz_offsets(S))
    assert exact.sum(1).tolist() == [1, S - 1, S, S - 1, 1]
    got = ref.attention_f64(qkv, 2, S, H, rel, False, m["eager"], m["scale"]).view(2, S, H, 64)
    mask = exact.t()[None].expand(2, S, H)
    assert torch.equal(got[mask], expected.view(2, S, H, 64)[mask]), f"S={S} {mode}"
    # a row without a key at its offset sees every key alike: the mean of V
    v = qkv.view(2, S, 3, H, 64)[:, :, 2].double()
    mean = ref.to_bf16(v.mean(1, keepdim=True).expand(2, S, H, 64))
    if not m["eager"] or S & (S - 1) == 0:               # eager rounds 1 / S to bf16 first: the mean only where that is exact
        bar(got[~mask], mean[~mask], f"uniform rows S={S} {mode}")


def test_strided_restatement_is_plain_indexing():
    B, S, H = 2, 5, 2
    D, g = H * 64, torch.Generator().manual_seed(1)
    ld = 3 * D + 64
    bs = S * ld + 8 * ld
    buf = torch.full((B * bs,), math.nan).bfloat16()
    qkv = torch.randn(B, S, 3 * D, generator=g).bfloat16()
    buf.view(B, S + 8, ld)[:, :S, :3 * D] = qkv
    out = torch.full((B * (S + 2) * (D + 24),), 777.0).bfloat16()
    full, rows = ref.attention_strided(buf, 0, D, 2 * D, B, S, H, ld, bs, None, True, False, 0.125, out, D + 24, (S + 2) * (D + 24))
    assert torch.equal(rows, ref.attention_f64(qkv, B, S, H, None, True, False, 0.125))
    f = full.view(B, S + 2, D + 24)
    assert torch.equal(f[:, :S, :D], rows) and bool((f[:, S:] == 777).all()) and bool((f[:, :, D:] == 777).all())


def test_dyadic_logits_are_exact_in_float32():
    g = torch.Generator().manual_seed(2)
    q, k = ref.dyadic(torch.randn(64, 64, generator=g) * 100, 1.0, 31.0), ref.dyadic(torch.randn(64, 64, generator=g) * 100, 1.0, 31.0)
    s64 = q.double() @ k.double().t()
    assert torch.equal((q.float() @ k.float().t()).double(), s64) and s64.abs().max().item() > 2000
    assert bool((s64.abs() * 64 < 2 ** 24).all())


def test_scale_that_is_no_power_of_two_shows_the_eager_rounding(monkeypatch):
    """eager's bf16(bf16(q.k) * scale): at scale 0.125 the second rounding is the identity, at float32(0.3) leaving it out moves most outputs,
    which is why tests/test_gpu_textenc_kernels.py runs eager attention at that scale too"""
    S, B, H = 77, 2, 2
    qkv = torch.randn(B, S, 3 * H * 64, generator=torch.Generator().manual_seed(71)).bfloat16()
    for scale, visible in ((0.125, False), (float(torch.tensor(0.3, dtype=torch.float32)), True)):
        want = ref.attention_f64(qkv, B, S, H, None, False, True, scale)
        calls = []
        monkeypatch.setattr(ref, "_bf", lambda x: (calls.append(1), x if len(calls) == 2 else x.float().bfloat16())[1])
        without = ref.attention_f64(qkv, B, S, H, None, False, True, scale)
        monkeypatch.undo()
        eq = (without.view(torch.int16) == want.view(torch.int16)).float().mean().item()
        assert (eq < 0.9) if visible else (eq == 1.0), (scale, eq)
