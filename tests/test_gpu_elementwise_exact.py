"""The oldest kernels of the library (csrc/elementwise.hip: LayerNorm in its three forms, the activations, the timestep embedding, add,
the Euler step, the two casts) against float64 restatements with the kernels' own rounding points (tests/helpers/elementwise_ref.py,
checked without a GPU by tests/test_elementwise_restatements_host.py), at about one bf16 ulp: every width at which the LayerNorm kernel
takes another path, every addressing mode its callers use, all 65 536 bf16 values through every activation, the second trip of the
grid-stride loops, every rounding decision of the casts, and the refusals of the ops.py wrappers."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import elementwise_ref as ref  # noqa: E402
from bf16_bar import bar_rows, ulps  # noqa: E402

SENTINEL = 7.0


# ------------------------------------------------------------------ LayerNorm
def _layernorm_case(gpu, t):
    """one launch of ops.layernorm as the case says; the columns behind each output row must keep the sentinel"""
    from domain_rag_amd import ops
    c = t["case"]
    y = torch.full((c.M, c.ldy), SENTINEL, dtype=torch.bfloat16, device=gpu)
    kw = {}
    if c.form == "mod":
        md = t["modbuf"].to(gpu).view(-1)
        kw = dict(scale=md[t["scale_off"]:], shift=md[t["shift_off"]:], ld_mod=c.ld_mod)
    elif c.form == "affine":
        kw = dict(gamma=t["gamma"].to(gpu), beta=t["beta"].to(gpu))
    ops.layernorm(t["xbuf"].to(gpu), y, c.M, c.D, ldx=c.ldx, rows_per_batch=c.rpb, x_batch_stride=c.x_bs, ldy=c.ldy, eps=c.eps, **kw)
    out = y.cpu()
    assert bool((out[:, c.D:] == SENTINEL).all()), f"{c}: columns past D were written"
    return out[:, :c.D].contiguous()


@pytest.mark.parametrize("group", ["widths", "rows", "inputs"])
def test_layernorm_vs_f64_restatement(gpu, group):
    """every case of elementwise_ref.ln_cases(): D in {8, 64, 504, 512, 520, 768, 1152, 3072, 4088, 4096} in all three forms; M in
    {1, 3, 5, 37}; batched rows in a wider buffer, the pooled form (ldx = T D, M = B), ldy > D, ld_mod = 2 D and 6 D with a modulation of its
    own per batch; unit-normal, mean = 100 x spread, one-outlier, constant, spread-1e-3 (eps 1e-6 and 1e-5), bf16-max and subnormal rows.
    Bar (bf16_bar.bar_rows): bit-equal on >= 99 % of a case's elements, the others within 1 bf16 ulp or within 2^-8 of their row's largest
    output.  The 99 % is a cap: the host test shows that the float32 evaluation of the restatement meets it on these inputs (99.75 % on the
    mean = 100 x spread rows, 99.97 % and more elsewhere).  D = 3072 with a modulation runs under ln_generic 0 and 1: equal bits, and each
    held to the restatement."""
    from domain_rag_amd import ops
    shares = {}
    for c in ref.ln_cases():
        if c.group != group:
            continue
        t = ref.ln_case_tensors(c)
        if c.D == 3072 and c.form == "mod":
            outs = []
            for generic in (0, 1):
                with ops.options(ln_generic=generic):
                    outs.append(_layernorm_case(gpu, t))
                eq = bar_rows(outs[-1], t["want"], f"ln_generic={generic} {c}")
            assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{c}: the fixed-width kernel and the generic one differ"
        else:
            eq = bar_rows(_layernorm_case(gpu, t), t["want"], str(c))
        key = (c.kind, c.form)
        shares[key] = min(eq, shares.get(key, 1.0))
    print(f"layernorm [{group}] equal share, min per (input kind, form):", {f"{k[0]}/{k[1]}": f"{v:.4%}" for k, v in shares.items()})


def test_layernorm_refusals(gpu):
    """shapes and operand sets the library refuses, before any launch: the output keeps its fill"""
    from domain_rag_amd import ops
    x = torch.zeros(4, 4104, dtype=torch.bfloat16, device=gpu)
    y = torch.full((4, 4104), SENTINEL, dtype=torch.bfloat16, device=gpu)
    v = torch.zeros(4104, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError, match="D <= 4096"):
        ops.layernorm(x, y, 4, 4104)
    with pytest.raises(RuntimeError, match="D % 8 == 0"):
        ops.layernorm(x, y, 4, 12)
    for kw in (dict(ldx=516), dict(ldy=516), dict(ld_mod=516, scale=v, shift=v)):
        with pytest.raises(RuntimeError, match="multiples of 8"):
            ops.layernorm(x, y, 4, 512, **kw)
    with pytest.raises(RuntimeError, match="come in pairs"):
        ops.layernorm(x, y, 4, 512, scale=v)
    with pytest.raises(RuntimeError, match="come in pairs"):
        ops.layernorm(x, y, 4, 512, gamma=v)
    with pytest.raises(RuntimeError, match="exclude each other"):         # it used to take gamma / beta and drop the modulation
        ops.layernorm(x, y, 4, 512, scale=v, shift=v, gamma=v, beta=v)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ------------------------------------------------------------------ activations
ACTS = (ref.ACT_SILU, ref.ACT_GELU_TANH, ref.ACT_GELU_ERF, ref.ACT_QUICK_GELU, ref.ACT_NONE)


def test_act_codes_are_the_librarys():
    from domain_rag_amd import ops
    assert (ops.ACT_NONE, ops.ACT_GELU_TANH, ops.ACT_SILU, ops.ACT_QUICK_GELU, ops.ACT_GELU_ERF) == \
        (ref.ACT_NONE, ref.ACT_GELU_TANH, ref.ACT_SILU, ref.ACT_QUICK_GELU, ref.ACT_GELU_ERF)


@pytest.mark.parametrize("kind", ACTS, ids=[ref.ACT_NAMES[k] for k in ACTS])
def test_act_every_bf16_value_vs_f64_definition(gpu, kind):
    """all 65 536 bf16 bit patterns through one launch, once more with 5 further elements (the scalar tail), and n = 1, 7 and 0.

    Against the activation's definition in float64 (elementwise_ref.act): |err| <= 2^-8 max(|ref|, 2^-126) + floor(x).
    First term: the output's rounding, half a bf16 ulp (2^-9 |ref| to 2^-8 |ref|), doubled.  Under 2^-126 the outputs are bf16 subnormals
    with a fixed ulp of 2^-133, where even the correctly rounded result misses 2^-8 |ref| (host test): the term stays at 2^-8 * 2^-126.
    floor, sigmoid forms (SiLU, QuickGELU, tanh-GELU written as x * sigmoid(2u)): fast_sigmoid is v_rcp_f32(1 + v_exp_f32(.)) on the raw
    instructions.  They flush a subnormal result to zero, and 2^(.) past 2^128 is inf with rcp(inf) = 0: a sigmoid below 2^-126 comes out as
    0, an absolute error under 2^-126, which the product with x makes |x| * 2^-126.  (SiLU's true value at x = -88 is still a
    normal number, -5e-37, where sigmoid may already be 0.)  floor, erf form: erff is within 2 ulp of a number in [0.5, 1], 2 * 2^-24; 1 + erff adds no rounding (both terms are multiples
    of 2^-24), so 1 + erff is off by at most 2^-23 in absolute terms, which 0.5 x turns into |x| * 2^-24; |x| * 2^-23 leaves the two roundings of
    the products room.  The identity code must return every value unchanged.

    Special values as the definition has them, and the definition says NaN at -inf: x * sigmoid(x) = -inf * 0, 0.5 x (1 + tanh) = -inf * 0,
    0.5 x (1 + erf) = -inf * 0 (torch's operators agree; only the identity returns -inf).  NaN in gives NaN out, +inf gives +inf, -0 gives
    -0, and the subnormal inputs give x / 2 (x for the identity), rounded to the subnormal grid."""
    from domain_rag_amd import ops
    name = ref.ACT_NAMES[kind]
    x = ref.all_bf16_patterns()
    worst, worst_normal = ref.act_check(x, ops.act(x.to(gpu), kind), kind, f"{name}, all bf16 values", normal_too=True)
    x5 = torch.cat([x, ref.act_special_inputs()[:5]])
    out = torch.full((x5.numel() + 3,), SENTINEL, dtype=torch.bfloat16, device=gpu)
    ops.act(x5.to(gpu), kind, out=out[:x5.numel()])
    worst = max(worst, ref.act_check(x5, out[:x5.numel()], kind, f"{name}, 65 536 + 5 elements"))
    assert bool((out[x5.numel():] == SENTINEL).all())
    for n in (1, 7):
        xs = ref.act_special_inputs()[:n] if n == 7 else torch.tensor([-3.0]).bfloat16()
        out = torch.full((16,), SENTINEL, dtype=torch.bfloat16, device=gpu)
        ops.act(xs.to(gpu), kind, out=out[:n])
        ref.act_check(xs, out[:n], kind, f"{name}, n = {n}")
        assert bool((out[n:] == SENTINEL).all()), f"{name}, n = {n}: wrote past n"
    assert ops.act(torch.empty(0, dtype=torch.bfloat16, device=gpu), kind).numel() == 0
    print(f"act {name}: max err / bound {worst:.3f} (results of 2^-126 and more: {worst_normal:.3f})")


# ------------------------------------------------------------------ timestep embedding
def test_timestep_embedding_vs_f64(gpu):
    """dim in {2, 6, 256, 258} for the times {0, 1e-3, 1, 356.25, 999.9, 1000, -7} (B = 7: B dim / 2 is no multiple of the 256-lane
    workgroup, and 903 pairs at dim 258 take four of them).  t = 0 gives exactly ones, then exactly zeros.  Elsewhere, against
    [cos(t f_j) | sin(t f_j)], f_j = 10000^(-j / half), in float64:  |err| <= 2^-9 |ref| * 2 + k |t f_j| 2^-23, k = 12.
    k from the kernel's float32 steps, f = expf(-9.210340371976184f * j / half), a = t * f: the exponent's argument is at most ln 10000 = 9.21
    and takes two roundings of 2^-24 each, 9.21 * 2^-23 absolute; the constant as a float32 is 0.117 * 2^-23 off relatively, 1.08 * 2^-23 more;
    expf is within 1 ulp, 2^-23 relative; t * f rounds once, 0.5 * 2^-23: 11.8 units of 2^-23 relative to a, which cos and sin pass on as
    at most that absolute error (elementwise_ref.timestep_bound)."""
    from domain_rag_amd import ops
    t = torch.tensor(ref.TIMESTEPS, dtype=torch.float32)
    for dim in ref.TIMESTEP_DIMS:
        half = dim // 2
        assert (t.numel() * half) % 256 != 0
        got = ops.timestep_embedding(t.to(gpu), dim).cpu()
        assert got.shape == (t.numel(), dim) and got.dtype == torch.bfloat16
        assert torch.equal(got[0], torch.cat([torch.ones(half), torch.zeros(half)]).bfloat16()), f"dim {dim}: t = 0 is not [1.. | 0..]"
        want, angle = ref.timestep_embedding(t, dim)
        err = (got.double() - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ref.timestep_bound(want, angle).clamp(min=1e-300))
        i = int(ratio.argmax())
        print(f"timestep embedding dim {dim}: max err / bound {ratio.max().item():.3f}")
        assert ratio.max().item() <= 1.0, f"dim {dim}: t = {t[i // dim].item()}, column {i % dim}: got {got.view(-1)[i].item()}, want {want.view(-1)[i].item()}"


# ------------------------------------------------------------------ add, Euler step, casts: the second trip of the grid-stride loop
@pytest.fixture(scope="module")
def second_trip():
    return ref.second_trip_inputs(ref.N_SECOND_TRIP_8, 21)


def _spots_equal(got, want, n, per_lane, what):
    for where, (lo, hi) in ref.second_trip_spots(n, per_lane).items():
        assert torch.equal(got[lo:hi], want[lo:hi]), f"{what}: {where} [{lo}, {hi}): {got[lo:hi].tolist()} != {want[lo:hi].tolist()}"


def _equal_or_both_nan(got, want):
    return bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())


def test_add_exact_and_second_trip(gpu, second_trip):
    """ops.add is one float32 sum rounded once, which is torch's bf16 sum: torch.equal.  n = 2048 * 256 * 8 + 8 * 300 + 3 sends 300 lanes on a
    second trip of the grid-stride loop and 3 elements to the scalar tail; n < 8 is a tail alone; special values sum as IEEE says"""
    from domain_rag_amd import ops
    a, b = second_trip
    n = a.numel()
    out = torch.full((n + 8,), math.nan, dtype=torch.bfloat16, device=gpu)
    ops.add(a.to(gpu), b.to(gpu), out=out[:n])
    got, want = out.cpu(), a + b
    _spots_equal(got[:n], want, n, 8, "add")
    assert torch.equal(got[:n], want) and bool(torch.isnan(got[n:]).all())
    sp = torch.tensor([math.inf, -math.inf, math.inf, math.nan, -0.0, 0.0, 2.0 ** -130, ref.BF16_MAX, 1.0, 2.0 ** -133, 3.0]).bfloat16()
    sq = torch.tensor([math.inf, -math.inf, -math.inf, 1.0, -0.0, -0.0, 2.0 ** -131, ref.BF16_MAX, 2.0 ** -8, 2.0 ** -133, -3.0]).bfloat16()
    got, want = ops.add(sp.to(gpu), sq.to(gpu)).cpu(), sp + sq
    fin = ~torch.isnan(want)
    assert _equal_or_both_nan(got, want) and torch.equal(got[fin].view(torch.int16), want[fin].view(torch.int16))       # inf - inf = NaN; -0 + 0 = +0
    for m in (1, 7):
        assert torch.equal(ops.add(a[:m].to(gpu), b[:m].to(gpu)).cpu(), a[:m] + b[:m])
    assert ops.add(torch.empty(0, dtype=torch.bfloat16, device=gpu), torch.empty(0, dtype=torch.bfloat16, device=gpu)).numel() == 0


def test_flow_euler_step_second_trip_vs_f64(gpu, second_trip):
    """x + dt * v in float32 may or may not be contracted to an fma, so at 4.2 M elements it parts from a two-rounding graph on a few
    elements: held to the float64 restatement bf16(x + dt v), within 1 ulp everywhere and equal on >= 99 % (a cap: the two-rounding float32
    evaluation is equal on 99.9999 % in the host test)"""
    from domain_rag_amd import ops
    x, v = second_trip
    n, dt = x.numel(), -0.0371
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.bfloat16, device=gpu)
    buf[:n] = x.to(gpu)
    ops.flow_euler_step(buf[:n], v.to(gpu), dt)
    got, want = buf.cpu(), ref.euler(x, v, dt)
    assert bool((got[n:] == SENTINEL).all())
    d = ulps(got[:n], want)
    eq = (d == 0).float().mean().item()
    print(f"flow_euler_step, {n} elements: {eq:.5%} equal to the float64 restatement, max {int(d.max())} ulp")
    for where, (lo, hi) in ref.second_trip_spots(n, 8).items():
        assert int(d[lo:hi].max()) <= 1, f"euler: {where} [{lo}, {hi}): {got[lo:hi].tolist()} vs {want[lo:hi].tolist()}"
    assert int(d.max()) <= 1 and eq >= 0.99
    for m in (1, 7):
        xs = x[:m].to(gpu).clone()
        ops.flow_euler_step(xs, v[:m].to(gpu), dt)
        assert int(ulps(xs.cpu(), want[:m]).max()) <= 1
    ops.flow_euler_step(torch.empty(0, dtype=torch.bfloat16, device=gpu), torch.empty(0, dtype=torch.bfloat16, device=gpu), dt)


def test_act_second_trip(gpu, second_trip):
    """SiLU on n = 2048 * 256 * 8 + 8 * 300 + 3 elements: the second trip and the tail under the bound of the all-values test"""
    from domain_rag_amd import ops
    x, _ = second_trip
    n = x.numel()
    out = torch.full((n + 8,), math.nan, dtype=torch.bfloat16, device=gpu)
    ops.act(x.to(gpu), ops.ACT_SILU, out=out[:n])
    got = out.cpu()
    for where, (lo, hi) in ref.second_trip_spots(n, 8).items():
        ref.act_check(x[lo:hi], got[lo:hi], ref.ACT_SILU, f"silu, {where} [{lo}, {hi})")
    print(f"act silu, {n} elements: max err / bound {ref.act_check(x, got[:n], ref.ACT_SILU, 'silu, second trip'):.3f}")
    assert bool(torch.isnan(got[n:]).all())


def test_to_bf16_every_rounding_decision_and_second_trip(gpu):
    """for every bf16 value b: b, the tie halfway to the next pattern, and the tie's float32 neighbours on both sides; so also overflow to
    inf past bf16 max, both infs, NaNs, and the float32 subnormals.  Exact against torch's cast (NaN by isnan).  n = 2048 * 256 + 300 sends
    300 lanes on a second trip."""
    from domain_rag_amd import ops
    f = ref.cast_f32_inputs()
    got, want = ops.to_bf16(f.to(gpu)).cpu(), f.bfloat16()
    assert got.dtype == torch.bfloat16 and _equal_or_both_nan(got, want)
    fin = ~torch.isnan(want)
    assert torch.equal(got[fin].view(torch.int16), want[fin].view(torch.int16))           # the sign of a zero too
    n = ref.N_SECOND_TRIP_1
    g = torch.randn(n, generator=torch.Generator().manual_seed(22))
    got, want = ops.to_bf16(g.to(gpu)).cpu(), g.bfloat16()
    _spots_equal(got, want, n, 1, "to_bf16")
    assert torch.equal(got, want)
    assert ops.to_bf16(torch.empty(0, device=gpu)).numel() == 0


def test_to_f32_every_bf16_value_and_second_trip(gpu, second_trip):
    from domain_rag_amd import ops
    p = ref.all_bf16_patterns()
    got, want = ops.to_f32(p.to(gpu)).cpu(), p.float()
    assert got.dtype == torch.float32 and _equal_or_both_nan(got, want)
    fin = ~torch.isnan(want)
    assert torch.equal(got[fin].view(torch.int32), want[fin].view(torch.int32))
    n = ref.N_SECOND_TRIP_1
    x = second_trip[0][:n]
    got = ops.to_f32(x.to(gpu)).cpu()
    _spots_equal(got, x.float(), n, 1, "to_f32")
    assert torch.equal(got, x.float())
    assert ops.to_f32(torch.empty(0, dtype=torch.bfloat16, device=gpu)).numel() == 0


# ------------------------------------------------------------------ the wrappers refuse what the kernels would walk off
def test_elementwise_wrappers_refuse_bad_operands(gpu):
    """a second operand of the wrong dtype or too small, an out of another size: ValueError that names the operand, before any library call
    (nothing here is ever launched on a tensor that is too small)"""
    from domain_rag_amd import ops
    bf = dict(dtype=torch.bfloat16, device=gpu)
    a, small, f32 = torch.zeros(100, **bf), torch.zeros(99, **bf), torch.zeros(100, device=gpu)
    with pytest.raises(ValueError, match=r"add\.b.*bfloat16"):
        ops.add(a, f32)
    with pytest.raises(ValueError, match=r"add\.b.*at least 100"):
        ops.add(a, small)
    with pytest.raises(ValueError, match=r"add\.b"):
        ops.add(a, torch.zeros(1, **bf).expand(100))                       # 100 elements by shape, one in memory
    with pytest.raises(ValueError, match=r"add\.out.*of 100"):
        ops.add(a, a, out=torch.zeros(101, **bf))
    with pytest.raises(ValueError, match=r"add\.out"):
        ops.add(a, a, out=f32)
    with pytest.raises(ValueError, match=r"add\.a"):
        ops.add(torch.zeros(1, **bf).expand(100), a)
    with pytest.raises(ValueError, match=r"act\.out.*of 100"):
        ops.act(a, ops.ACT_SILU, out=small)
    with pytest.raises(ValueError, match=r"act\.out.*bfloat16"):
        ops.act(a, ops.ACT_SILU, out=f32)
    with pytest.raises(ValueError, match=r"flow_euler_step\.v.*bfloat16"):
        ops.flow_euler_step(a, f32, 0.1)
    with pytest.raises(ValueError, match=r"flow_euler_step\.v.*at least 100"):
        ops.flow_euler_step(a, small, 0.1)
    with pytest.raises(ValueError, match=r"flow_euler_step\.x"):
        ops.flow_euler_step(torch.zeros(1, **bf).expand(100), a, 0.1)
    assert bool((a == 0).all())


def test_layernorm_wrapper_refuses_rows_outside_its_tensors(gpu):
    """M, ldx, ldy, rows_per_batch, x_batch_stride and ld_mod address rows; one that leaves x, y, scale / shift or gamma / beta is a
    ValueError that names the operand, before any library call.  The same call with every operand just large enough runs."""
    from domain_rag_amd import ops
    bf = dict(dtype=torch.bfloat16, device=gpu)
    D, M, rpb, ldx, x_bs, ldy, ld_mod = 64, 7, 3, 72, 256, 80, 128             # three batches, the last of one row
    nx, ny, nm = 2 * x_bs + D, (M - 1) * ldy + D, 2 * ld_mod + D                # the last element each addressing reaches, + 1
    x, y, sc, sh = torch.randn(nx, device=gpu).bfloat16(), torch.full((ny,), SENTINEL, **bf), torch.zeros(nm, **bf), torch.zeros(nm, **bf)
    g = torch.ones(D, **bf)
    kw = dict(ldx=ldx, rows_per_batch=rpb, x_batch_stride=x_bs, ldy=ldy)
    ops.layernorm(x, y, M, D, scale=sc, shift=sh, ld_mod=ld_mod, **kw)          # exactly enough of everything
    ops.layernorm(x, y, M, D, gamma=g, beta=g, **kw)
    nx_full = x_bs + 2 * ldx + D                                                 # M = 6: two full batches, the last row of the second reaches furthest
    ops.layernorm(torch.zeros(nx_full, **bf), y, 6, D, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.x"):
        ops.layernorm(torch.zeros(nx_full - 8, **bf), y, 6, D, **kw)
    over = dict(ldx=ldx, rows_per_batch=rpb, x_batch_stride=8, ldy=ldy)         # batches that overlap: the last full one reaches past the short last one
    ops.layernorm(torch.zeros(8 + 2 * ldx + D, **bf), y, M, D, **over)
    with pytest.raises(ValueError, match=r"layernorm\.x"):
        ops.layernorm(torch.zeros(2 * ldx + D, **bf), y, M, D, **over)
    with pytest.raises(ValueError, match=r"layernorm\.x"):
        ops.layernorm(x[8:], y, M, D, scale=sc, shift=sh, ld_mod=ld_mod, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.x"):
        ops.layernorm(x, y, M + 1, D, scale=sc, shift=sh, ld_mod=ld_mod, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.x"):
        ops.layernorm(x, y, M, D, ldx=ldx, rows_per_batch=rpb, x_batch_stride=x_bs + 8, ldy=ldy)
    with pytest.raises(ValueError, match=r"layernorm\.x"):                      # the pooled form with one image too few
        ops.layernorm(torch.zeros(4 * 5 * D, **bf), torch.zeros(5 * D, **bf), 5, D, ldx=5 * D)
    with pytest.raises(ValueError, match=r"layernorm\.y"):
        ops.layernorm(x, y[8:], M, D, scale=sc, shift=sh, ld_mod=ld_mod, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.y"):
        ops.layernorm(x, y, M, D, ldx=ldx, rows_per_batch=rpb, x_batch_stride=x_bs, ldy=ldy + 8)
    with pytest.raises(ValueError, match=r"layernorm\.scale"):
        ops.layernorm(x, y, M, D, scale=sc[8:], shift=sh, ld_mod=ld_mod, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.shift"):
        ops.layernorm(x, y, M, D, scale=sc, shift=sh[8:], ld_mod=ld_mod, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.scale"):
        ops.layernorm(x, y, M, D, scale=sc, shift=sh, ld_mod=ld_mod + 8, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.scale.*bfloat16"):
        ops.layernorm(x, y, M, D, scale=sc.float(), shift=sh, ld_mod=ld_mod, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.gamma"):
        ops.layernorm(x, y, M, D, gamma=g[8:], beta=g, **kw)
    with pytest.raises(ValueError, match=r"layernorm\.beta"):
        ops.layernorm(x, y, M, D, gamma=g, beta=g[8:], **kw)
    with pytest.raises(ValueError, match=r"layernorm\.beta.*bfloat16"):
        ops.layernorm(x, y, M, D, gamma=g, beta=g.float(), **kw)
    with pytest.raises(ValueError, match=r"layernorm\.x_batch_stride"):
        ops.layernorm(x, y, M, D, ldx=ldx, rows_per_batch=rpb, x_batch_stride=-8, ldy=ldy)
