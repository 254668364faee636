"""tests/helpers/elementwise_ref.py without a GPU: the float64 restatements that tests/test_gpu_elementwise_exact.py holds the kernels of
csrc/elementwise.hip to.  Three things: each restatement agrees with torch's own CPU operator (and, where a definition cancels, with
mpmath); the same restatement evaluated in float32 meets the caps on the very inputs the GPU tests use, so that a float32 kernel can; and
the case lists hold what they are meant to hold."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import elementwise_ref as ref  # noqa: E402
from bf16_bar import bar_rows, ulps  # noqa: E402


@pytest.fixture(scope="module")
def ln_tensors():
    return [ref.ln_case_tensors(c) for c in ref.ln_cases()]


def _same_bits_or_nan(a, b):
    return bool(((a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------ rounding
def test_round_bf16_is_one_rounding_to_nearest_even():
    f = ref.cast_f32_inputs()
    assert _same_bits_or_nan(ref.to_bf16(f), f.bfloat16())                  # every rounding decision of float32 -> bf16, torch's cast as the judge
    up = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 + 2.0 ** -40)], dtype=torch.float64)     # a hair past a tie: float32 lands ON it
    assert ref.round_bf16(up).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    edge = torch.tensor([3.0 * 2.0 ** -134, 2.0 ** -134, ref.BF16_MAX * (1 + 2.0 ** -10), ref.FLT_MAX], dtype=torch.float64)
    assert ref.round_bf16(edge).tolist() == [2.0 ** -132, 0.0, ref.BF16_MAX, math.inf]          # subnormal ties to even; the last tie goes to inf
    p = ref.all_bf16_patterns()
    assert p.view(torch.int16).to(torch.int32).remainder(65536).tolist() == list(range(65536))
    assert _same_bits_or_nan(ref.to_bf16(p), p)


# ------------------------------------------------------------------ LayerNorm
def test_layernorm_cases_cover_what_they_should():
    cs = ref.ln_cases()
    assert {c.D for c in cs} == set(ref.LN_WIDTHS) == {8, 64, 504, 512, 520, 768, 1152, 3072, 4088, 4096}
    assert all({(c.D, f) for c in cs if c.form == f} >= {(D, f) for D in ref.LN_WIDTHS} for f in ref.LN_FORMS)
    assert {c.M for c in cs} >= {1, 3, 5, 37} and any(c.M % 4 for c in cs)
    assert any(c.rpb and c.x_bs > c.rpb * c.ldx for c in cs) and any(c.ldx == 7 * c.D and c.rpb == 0 for c in cs)
    assert any(c.ldy > c.D for c in cs) and {c.ld_mod // c.D for c in cs if c.form == "mod"} == {2, 6}
    assert {c.kind for c in cs} == {"normal", "offset", "outlier", "constant", "small", "extreme"}
    assert {c.eps for c in cs if c.kind == "small"} == {1e-6, 1e-5}
    assert all(v % 8 == 0 for c in cs for v in (c.D, c.ldx, c.x_bs, c.ldy, c.ld_mod))         # 16-byte loads: nothing here may be misaligned


def test_layernorm_restatement_vs_torch_cpu(ln_tensors):
    """F.layer_norm, then the modulation as diffusers writes it on bf16 tensors: n * (1 + scale) + shift rounds where the restatement says.
    Twice: on the bf16 rows themselves, where torch's CPU kernel keeps its statistics in float32 its own way (held to the bar; on the
    mean = 100 x spread rows it is equal on 96 % only, less than the plain float32 evaluation below, so there it is held to the bar without
    the cap and its share is printed; on the constant rows it finds a mean that is not the constant and is left out), and with F.layer_norm on the float64 image of the rows, rounded once (held to the bar everywhere).  The rows whose
    squares leave float32's range are a statement about float32 and no business of torch's float64 kernel."""
    shares, offset, shares64 = [], [], []
    for t in ln_tensors:
        c = t["case"]
        if c.kind == "extreme":
            continue
        x = t["rows"]
        gb = (t["gamma"], t["beta"]) if c.form == "affine" else (None, None)
        got = F.layer_norm(x, (c.D,), *gb, c.eps)
        eps32 = float(torch.tensor(c.eps, dtype=torch.float32))
        got64 = ref.to_bf16(F.layer_norm(x.double(), (c.D,), *(None if v is None else v.double() for v in gb), eps32))
        if c.form == "mod":
            got, got64 = (n * (1 + t["kw"]["scale"]) + t["kw"]["shift"] for n in (got, got64))
        loose = c.kind == "offset"
        if c.kind != "constant":
            (offset if loose else shares).append(bar_rows(got, t["want"], f"torch CPU bf16 vs restatement, {c}", frac=0.0 if loose else 0.99))
        shares64.append(bar_rows(got64, t["want"], f"torch CPU float64 vs restatement, {c}"))
    print(f"layernorm, torch CPU bf16 vs restatement: {len(shares)} cases, equal share min {min(shares):.4%}; the {len(offset)} offset cases "
          f"min {min(offset):.4%}; torch CPU float64, rounded once: {len(shares64)} cases, min {min(shares64):.4%}")


def test_layernorm_float32_evaluation_meets_the_cap(ln_tensors):
    """the restatement in float32, the kernel's precision: what a correct float32 kernel may differ by.  The 99 % of the bar is a cap that
    float32 alone must meet on every input the GPU test uses, or the input is wrong for the test"""
    shares = {}
    for t in ln_tensors:
        c = t["case"]
        got = ref.layernorm(t["rows"], c.form, eps=c.eps, dtype=torch.float32, **t["kw"])
        eq = bar_rows(got, t["want"], f"float32 vs float64, {c}")
        shares[c.kind] = min(eq, shares.get(c.kind, 1.0))
    print("layernorm, float32 evaluation vs restatement, equal share min per input kind:", {k: f"{v:.4%}" for k, v in shares.items()})


def test_layernorm_inputs_show_what_they_are_for(ln_tensors):
    """eps 1e-6 against 1e-5 on the spread-1e-3 rows parts the outputs by about 2 x; a modulation row of the wrong batch moves nearly every
    element; the bf16-max rows come out as zeros (plain) and the subnormal rows as normal numbers"""
    by = {(t["case"].kind, t["case"].eps, t["case"].form, t["case"].D): t for t in ln_tensors if t["case"].group == "inputs"}
    a, b = by[("small", 1e-6, "plain", 520)], by[("small", 1e-5, "plain", 520)]
    wa = ref.layernorm(a["rows"], "plain", eps=1e-6).float()
    wb = ref.layernorm(a["rows"], "plain", eps=1e-5).float()
    assert 1.8 < (wa.abs().mean() / wb.abs().mean()).item() < 3.0 and torch.equal(b["want"], ref.layernorm(b["rows"], "plain", eps=1e-5))
    for t in ln_tensors:
        c = t["case"]
        if c.form == "mod" and c.kind == "normal" and c.M > (c.rpb or c.M):
            wrong = (t["batch"] + 1) % (int(t["batch"].max()) + 1)
            so, ho = t["scale_off"], t["shift_off"]
            other = ref.layernorm(t["rows"], "mod", eps=c.eps, scale=t["modbuf"][wrong, so:so + c.D], shift=t["modbuf"][wrong, ho:ho + c.D])
            assert (ulps(other, t["want"]) > 1).float().mean().item() > 0.9, c
    e = by[("extreme", 1e-6, "plain", 520)]
    assert bool((e["want"][1::3] == 0).all() and (e["want"][2::3] == 0).all())
    sub = e["want"][0::3].float().abs()
    assert bool((e["rows"][0::3].float().abs() < 2.0 ** -126).all()) and (sub > 2.0 ** -126).float().mean().item() > 0.9
    k = by[("constant", 1e-6, "mod", 520)]
    assert torch.equal(k["want"], k["kw"]["shift"])


# ------------------------------------------------------------------ activations
ACTS = (ref.ACT_SILU, ref.ACT_GELU_TANH, ref.ACT_GELU_ERF, ref.ACT_QUICK_GELU)


def _mp_definition(kind, x, mp):
    x = mp.mpf(x)
    if kind == ref.ACT_SILU:
        return x / (1 + mp.exp(-x))
    if kind == ref.ACT_QUICK_GELU:
        return x / (1 + mp.exp(-mp.mpf("1.702") * x))
    if kind == ref.ACT_GELU_TANH:
        return x / 2 * (1 + mp.tanh(mp.sqrt(2 / mp.pi) * (x + mp.mpf("0.044715") * x ** 3)))
    return x / 2 * (1 + mp.erf(x / mp.sqrt(2)))


@pytest.mark.parametrize("kind", ACTS, ids=[ref.ACT_NAMES[k] for k in ACTS])
def test_act_definitions_vs_mpmath(kind):
    """the definitions as written, 1 + tanh and 1 + erf included, at 400 digits: the float64 forms of elementwise_ref.act are within 1e-12 of
    them (relative: u itself, up to 300 here, is rounded to 2^-53 before e^u sees it), on every 37th finite bf16 value up to |x| = 2^10 and on every value on the way to a vanishing result, -20 < x < -3
    (1 + tanh u is 1e-262 there: hence 400 digits)"""
    mp = pytest.importorskip("mpmath").mp
    mp.dps = 400
    p = ref.all_bf16_patterns()
    xf = p.float()
    pick = torch.isfinite(xf) & (xf.abs() <= 1024)
    pick &= (torch.arange(65536) % 37 == 0) | ((xf < -3) & (xf > -20))
    x = p[pick]
    got = ref.act(x, kind).tolist()
    worst = 0.0
    for xi, gi in zip(x.double().tolist(), got):
        want = _mp_definition(kind, xi, mp)
        if want == 0:
            assert gi == 0
            continue
        if abs(want) < mp.mpf(2) ** -1000:               # under float64's normal range: nothing the bound can see (bf16 ends at 2^-133)
            assert abs(gi) < 2.0 ** -999
            continue
        worst = max(worst, float(abs((mp.mpf(gi) - want) / want)))
    print(f"{ref.ACT_NAMES[kind]}: {len(got)} inputs, float64 form vs 400-digit definition: worst relative error {worst:.2e}")
    assert worst < 1e-12


@pytest.mark.parametrize("kind", ACTS, ids=[ref.ACT_NAMES[k] for k in ACTS])
def test_act_restatement_vs_torch_cpu(kind):
    """torch's CPU operators on every bf16 value from 2^-120 to 2^127, the zeros and every NaN (float32 inside, one rounding to bf16) against the definition.  torch writes both
    GELUs as 0.5 x (1 + ...), whose float32 cancellation is the erf form's floor, |x| * 2^-23; QuickGELU has no operator: its graph
    x * sigmoid(1.702 x) on the float32 image of x.  SiLU stands under the bound the kernel gets."""
    x = ref.all_bf16_patterns()
    # torch's erf GELU forms x * (1 + erf) before it halves (inf from 2^127 on, NaN at +inf) and flushes subnormal results: the kernel test holds those
    a = x.float().abs()
    x = x[torch.isnan(x) | (a == 0) | ((a >= 2.0 ** -120) & (a < 2.0 ** 127))]
    if kind == ref.ACT_SILU:
        got = F.silu(x)
    elif kind == ref.ACT_GELU_TANH:
        got = F.gelu(x, approximate="tanh")
    elif kind == ref.ACT_GELU_ERF:
        got = F.gelu(x)
    else:
        got = (x.float() * torch.sigmoid(1.702 * x.float())).bfloat16()
    r = ref.act(x, kind)
    bound = 2.0 ** -8 * torch.clamp(r.abs(), min=2.0 ** -126) + ref.act_floor(x, kind if kind in (ref.ACT_SILU, ref.ACT_QUICK_GELU) else ref.ACT_GELU_ERF)
    worst, worst_normal = ref.act_check(x, got, kind, f"torch CPU {ref.ACT_NAMES[kind]}", bound=bound, normal_too=True)
    print(f"torch CPU {ref.ACT_NAMES[kind]} vs definition: max err / bound {worst:.3f} (results of 2^-126 and more: {worst_normal:.3f})")


@pytest.mark.parametrize("kind", ACTS + (ref.ACT_NONE,), ids=[ref.ACT_NAMES[k] for k in ACTS + (ref.ACT_NONE,)])
def test_act_bound_admits_the_correctly_rounded_result_and_little_else(kind):
    """bf16(definition) passes act_check on all 65 536 inputs with err / bound <= 1; the same moved by two bf16 ulps does not.  And the reason
    the bound's first term stops shrinking under 2^-126: there the correctly rounded result itself misses 2^-8 |ref|."""
    x = ref.all_bf16_patterns()
    r = ref.act(x, kind)
    best = ref.to_bf16(r)
    assert ref.act_check(x, best, kind, "the correctly rounded definition") <= 1.0
    if kind == ref.ACT_NONE:
        return
    sub = torch.isfinite(r) & (r.abs() < 2.0 ** -126) & (r != 0)
    missed = (best.double() - r).abs() > 2.0 ** -8 * r.abs() + ref.act_floor(x, kind)
    assert int((missed & sub).sum()) > 0 and int((missed & ~sub & torch.isfinite(r)).sum()) == 0
    off = (best.view(torch.int16) + 2).view(torch.bfloat16)
    with pytest.raises(AssertionError):
        ref.act_check(x, off, kind, "two ulps off")


# ------------------------------------------------------------------ timestep embedding
def test_timestep_embedding_float32_evaluation_meets_the_bound():
    """the kernel's float32 steps on the host (torch's float32 exp / cos / sin in place of the device's) against the float64 restatement,
    under the bound the kernel gets; t = 0 gives exactly ones and zeros; and the oracle's timestep_proj agrees with the restatement"""
    from oracle import flux as oflux
    t = torch.tensor(ref.TIMESTEPS, dtype=torch.float32)
    for dim in ref.TIMESTEP_DIMS:
        half = dim // 2
        want, angle = ref.timestep_embedding(t, dim)
        f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * torch.arange(half, dtype=torch.float32) / float(half))
        a = t[:, None] * f[None, :]
        got = torch.cat([torch.cos(a), torch.sin(a)], dim=1).bfloat16()
        ratio = (got.double() - want).abs() / ref.timestep_bound(want, angle).clamp(min=1e-300)
        ratio[(got.double() == want)] = 0.0
        print(f"timestep embedding dim {dim}: float32 evaluation, max err / bound {ratio.max().item():.3f}")
        assert ratio.max().item() <= 1.0
        assert torch.equal(got[0], torch.cat([torch.ones(half), torch.zeros(half)]).bfloat16())
    want, _ = ref.timestep_embedding(t, 256)
    assert torch.allclose(oflux.timestep_proj(t).double(), want, atol=2e-4, rtol=0)


# ------------------------------------------------------------------ Euler step
def test_euler_float32_evaluation_meets_the_cap():
    """x + dt * v in float32 with two roundings, the kernel's other possible self, against the one-rounding restatement on the second-trip
    inputs of the GPU test: within 1 ulp everywhere, equal on far more than the 99 % of the cap"""
    x, v = ref.second_trip_inputs(ref.N_SECOND_TRIP_8, 21)
    dt = -0.0371
    want = ref.euler(x, v, dt)
    got = ref.euler_f32(x, v, dt)
    d = ulps(got, want)
    eq = (d == 0).float().mean().item()
    print(f"euler, float32 two-rounding evaluation vs restatement: {eq:.5%} equal, max {int(d.max())} ulp")
    assert eq >= 0.99 and int(d.max()) <= 1
    assert torch.equal(ref.to_bf16(x.double() + v.double()), x + v)         # add: torch's bf16 sum IS the once-rounded sum


def test_second_trip_sizes():
    assert ref.N_SECOND_TRIP_8 == 4196707 and ref.N_SECOND_TRIP_8 // 8 > 2048 * 256 and ref.N_SECOND_TRIP_8 % 8 == 3
    assert ref.N_SECOND_TRIP_1 == 524588
    for n, per in ((ref.N_SECOND_TRIP_8, 8), (ref.N_SECOND_TRIP_1, 1)):
        for lo, hi in ref.second_trip_spots(n, per).values():
            assert 0 <= lo < hi <= n
