"""The first-block step cache of the Flux DiT (``step_cache.StepCache``, ``FluxTransformerHIP.forward(..., cache=...)``) and its pipeline switch.

What is pinned, and from what:
  * off is untouched: ``cache=None`` and a cache that never fires give equal bits and equal recorded launch sequences;
  * the cache's arithmetic, bit for bit from the HIP forward's own taps (each is one float32 operation and one rounding to bf16);
  * the tail of a reused step against the oracle's own tail (final AdaLayerNormContinuous + proj_out) by the project's rule: HIP may sit
    at most SLACK x further (rms-relative) from the float32 evaluation than the bf16 evaluation does;
  * the decisions on inputs whose ratios were measured on the CPU oracle with a margin of about 10x on each side of the threshold 0.15
    (same timestep: input + 0.01 N(0,1) -> 0.014-0.015, unrelated input -> 1.38-1.48, a repeated input -> exactly 0);
  * launch accounting of a reused step, invalidation, ``forced``, and the two pipelines through ``Engine``.
The configurations and ``_setup`` are those of tests/test_gpu_flux_mxfp8.py (copied: that file may change)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
SLACK = 1.3      # as tests/test_gpu_flux.py: HIP may sit at most this factor further from float32 than the reference evaluation does
CONFIGS = [(1, 24, 6, 8, 1, 1, 64), (2, 77, 12, 10, 2, 2, 384)]
THRESHOLD = 0.15
NEAR, FAR = (0.005, 0.05), (0.5, 3.0)      # where the recorded ratios of a perturbed / an unrelated input must fall


def _rms_rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _setup(B, St, h, w, nl, ns, inch, seed=0):
    from domain_rag_amd.flux import latent_image_ids
    from domain_rag_amd.flux_params import FluxConfig, init_params
    cfg = FluxConfig(in_channels=inch, num_layers=nl, num_single_layers=ns, num_attention_heads=2, joint_attention_dim=128, pooled_projection_dim=64)
    params = init_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    hidden = torch.randn(B, h * w, cfg.in_channels, generator=g).bfloat16()
    enc = torch.randn(B, St, cfg.joint_attention_dim, generator=g).bfloat16()
    pooled = torch.randn(B, cfg.pooled_projection_dim, generator=g).bfloat16()
    return cfg, params, (hidden, enc, pooled, torch.linspace(0.9, 0.3, B), latent_image_ids(h, w), torch.zeros(St, 3), torch.full((B,), 30.0))


_cases = {}


def _case(gpu, cfgt):
    """one configuration's parameters, model and inputs (base, near = base + 0.01 N(0,1), far = an unrelated draw), built once"""
    if cfgt in _cases:
        return _cases[cfgt]
    from domain_rag_amd.flux import FluxTransformerHIP
    cfg, params, inp = _setup(*cfgt)
    hidden = inp[0]
    g = torch.Generator().manual_seed(99)
    near = (hidden.float() + 0.01 * torch.randn(hidden.shape, generator=g)).bfloat16()
    far = torch.randn(hidden.shape, generator=g).bfloat16()
    rest = (inp[1].to(gpu), inp[2].to(gpu)) + tuple(inp[3:])
    c = dict(cfg=cfg, params=params, St=cfgt[1], base=hidden.to(gpu), near=near.to(gpu), far=far.to(gpu), rest=rest,
             model=FluxTransformerHIP(cfg, params, gpu, linear_precision="bf16"))
    _cases[cfgt] = c
    return c


def _fwd(c, hidden, cache=None, taps=None, model=None):
    return (model or c["model"]).forward(hidden, *c["rest"], taps=taps, cache=cache).clone()


def _recorded(fn):
    """(result, [(shape, kernel name)] of the GEMM launches in order, [attention kernel names])"""
    from domain_rag_amd import ops
    rec = ops.GemmRecorder()
    ops.set_recorder(rec)
    try:
        out = fn()
    finally:
        ops.set_recorder(None)
    torch.cuda.synchronize()
    return out, [(s, rec.kernel_of(s, k)) for s, k in zip(rec.shapes, rec.is_conv)], [a[3] for a in rec.attn]


def _ratio64(e, f):
    e, f = e.double().cpu(), f.double().cpu()
    B = e.shape[0]
    return ((e - f).abs().reshape(B, -1).sum(1) / f.abs().reshape(B, -1).sum(1)).tolist()


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_off_is_untouched(gpu, cfgt):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, cfgt)
    plain, gemms0, attn0 = _recorded(lambda: _fwd(c, c["base"]))
    cache = StepCache(0.0)
    for hidden in (c["base"], c["base"], c["near"]):          # a repeated input has ratio exactly 0: still not under a threshold of 0
        want = plain if hidden is c["base"] else _fwd(c, hidden)
        got, gemms, attn = _recorded(lambda: _fwd(c, hidden, cache))
        assert torch.equal(got, want)
        assert gemms == gemms0 and attn == attn0
    assert [d.reused for d in cache.decisions] == [False] * 3
    assert cache.decisions[0].ratios is None and cache.decisions[1].ratios == (0.0,) * cfgt[0]


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_arithmetic_is_pinned_from_the_taps(gpu, cfgt):
    from domain_rag_amd.flux import StepCache
    from oracle import flux as oflux
    c = _case(gpu, cfgt)
    St, nl, ns = c["St"], cfgt[4], cfgt[5]
    last = f"single.{ns - 1}" if ns else f"double.{nl - 1}"
    cache = StepCache(THRESHOLD)
    # a computed step
    t1 = {}
    _fwd(c, c["base"], cache, t1)
    d0_img = t1["double.0"][:, St:]
    delta1 = (d0_img.float() - t1["x_embed"].float()).bfloat16()
    assert torch.equal(t1["cache.delta"], delta1)
    assert "cache.x_img" not in t1 and cache.decisions[-1] == (None, False)
    R = (t1[last][:, St:].float() - d0_img.float()).bfloat16()
    assert torch.equal(cache.R, R)
    assert torch.equal(cache.F, delta1)
    # a reused step
    t2 = {}
    out = _fwd(c, c["near"], cache, t2)
    d0_img = t2["double.0"][:, St:]
    delta2 = (d0_img.float() - t2["x_embed"].float()).bfloat16()
    assert torch.equal(t2["cache.delta"], delta2)
    assert cache.decisions[-1].reused
    assert torch.equal(t2["cache.x_img"], (d0_img.float() + R.float()).bfloat16())
    assert torch.equal(cache.R, R) and torch.equal(cache.F, delta1), "a reused step must leave F and R as they are"
    assert not any(k.startswith("single.") or k == "double.1" for k in t2), "a block ran on a reused step"
    want = _ratio64(delta2, delta1)
    for got, w in zip(cache.decisions[-1].ratios, want):
        print(f"{cfgt}: ratio {got:.17g}, from the taps in float64 {w:.17g}")
        assert abs(got - w) <= 1e-9 * w
    # the tail of the reused step against the oracle's own tail, in bf16 and in float32
    p = {k: v for k, v in c["params"].items()}
    p32 = {k: v.float() for k, v in p.items()}
    x, temb = t2["cache.x_img"].cpu(), t2["temb"].cpu()
    ref_bf16 = oflux._lin(oflux.adaln_continuous(p, "norm_out.linear", temb, x), p, "proj_out")
    ref32 = oflux._lin(oflux.adaln_continuous(p32, "norm_out.linear", temb.float(), x.float()), p32, "proj_out")
    d_hip, d_ref = _rms_rel(out, ref32), _rms_rel(ref_bf16, ref32)
    print(f"{cfgt}: tail of a reused step, rms-relative distance from float32: HIP {d_hip:.4e}, bf16 oracle {d_ref:.4e}, ratio {d_hip / d_ref:.2f}")
    assert d_hip <= SLACK * d_ref, f"HIP vs f32 {d_hip:.4e}, bf16 oracle vs f32 {d_ref:.4e}, ratio {d_hip / d_ref:.2f} (bar {SLACK})"


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_decisions(gpu, cfgt):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, cfgt)
    cache = StepCache(THRESHOLD)
    outs = [_fwd(c, h, cache) for h in (c["base"], c["near"], c["far"], c["far"])]
    d = cache.decisions
    print(f"{cfgt}: ratios {[x.ratios for x in d]}")
    assert [x.reused for x in d] == [False, True, False, True]
    assert d[0].ratios is None
    assert all(NEAR[0] <= r <= NEAR[1] for r in d[1].ratios), d[1]
    assert all(FAR[0] <= r <= FAR[1] for r in d[2].ratios), d[2]
    assert d[3].ratios == (0.0,) * cfgt[0], d[3]          # step 3 replaced F: the repeat compares against itself
    # a computed step with a cache gives the plain forward's bits; a reused one does not (it ran one block of its own input)
    assert torch.equal(outs[0], _fwd(c, c["base"])) and torch.equal(outs[2], _fwd(c, c["far"]))
    assert not torch.equal(outs[1], _fwd(c, c["near"]))


def test_batch_rule_one_unrelated_image_blocks_the_reuse(gpu):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, CONFIGS[1])
    mixed = torch.stack([c["near"][0], c["far"][1]])
    cache = StepCache(THRESHOLD)
    _fwd(c, c["base"], cache)
    out = _fwd(c, mixed, cache)
    r = cache.decisions[-1]
    assert not r.reused and NEAR[0] <= r.ratios[0] <= NEAR[1] and FAR[0] <= r.ratios[1] <= FAR[1], r
    assert torch.equal(out, _fwd(c, mixed))


def test_launch_accounting_of_a_reused_step(gpu):
    """a reused step launches the GEMMs of a model with one double block and nothing else, and one attention.  The models' stacked
    modulation weights differ in their row count (every block's modulation is one GEMM), so that one launch is compared by M and K only."""
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache
    from domain_rag_amd.flux_params import FluxConfig
    c = _case(gpu, CONFIGS[1])
    cfg = c["cfg"]
    one = FluxTransformerHIP(FluxConfig(**{**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}, "num_layers": 1, "num_single_layers": 0}),
                             c["params"], gpu, linear_precision="bf16")
    _, g_one, a_one = _recorded(lambda: _fwd(c, c["base"], model=one))
    cache = StepCache(THRESHOLD)
    _, g_full, a_full = _recorded(lambda: _fwd(c, c["base"], cache))
    _, g_reuse, a_reuse = _recorded(lambda: _fwd(c, c["near"], cache))
    assert cache.decisions[-1].reused

    def shapes(gemms, mod_total):
        return [(M, -1, K) if N == mod_total else (M, N, K) for (M, N, K), _ in gemms]
    assert shapes(g_reuse, c["model"].mod_total) == shapes(g_one, one.mod_total)
    assert len(a_reuse) == 1 and a_reuse == a_one
    assert len(g_full) > len(g_reuse) and len(a_full) == CONFIGS[1][4] + CONFIGS[1][5]


def test_invalidation_and_refusals(gpu):
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache, latent_image_ids
    from domain_rag_amd.flux_params import FluxConfig
    c = _case(gpu, CONFIGS[1])
    hidden, (enc, pooled, t, img_ids, txt_ids, gd) = c["base"], c["rest"]
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16")
    cache = StepCache(math.inf)

    def step(h=hidden, e=enc, p=pooled, tt=t, ids=img_ids, g=gd):
        m.forward(h, e, p, tt, ids, txt_ids, g, cache=cache)
        return cache.decisions[-1].reused
    assert [step(), step()] == [False, True]
    # a changed B
    assert step(hidden[:1].contiguous(), enc[:1].contiguous(), pooled[:1].contiguous(), t[:1], g=gd[:1]) is False
    assert step(hidden[:1].contiguous(), enc[:1].contiguous(), pooled[:1].contiguous(), t[:1], g=gd[:1]) is True
    # a changed Si (12 x 10 -> 12 x 8 latents)
    small = hidden[:1, :96].contiguous()
    assert step(small, enc[:1].contiguous(), pooled[:1].contiguous(), t[:1], latent_image_ids(12, 8), gd[:1]) is False
    assert [step(), step()] == [False, True]
    # a switch of the Linear precision, both ways
    m.linear_precision = "mxfp8"
    assert [step(), step()] == [False, True]
    m.linear_precision = "bf16"
    assert [step(), step()] == [False, True]
    # reset()
    cache.reset()
    assert cache.decisions == [] and [step(), step()] == [False, True] and cache.decisions[0].ratios is None
    with pytest.raises(ValueError, match="step cache"):
        m.forward_graphed(hidden, enc, pooled, t, img_ids, txt_ids, gd, cache=cache)
    cfg = c["cfg"]
    one = FluxTransformerHIP(FluxConfig(**{**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}, "num_layers": 1, "num_single_layers": 0}),
                             c["params"], gpu)
    with pytest.raises(ValueError, match="step cache"):
        one.forward(hidden, enc, pooled, t, img_ids, txt_ids, gd, cache=StepCache(0.1))
    one.forward(hidden, enc, pooled, t, img_ids, txt_ids, gd)            # without a cache it runs
    with pytest.raises(ValueError):
        StepCache(-0.1)
    with pytest.raises(ValueError):
        StepCache(float("nan"))


def test_forced_pattern_is_obeyed(gpu):
    """``forced[i]`` is the value ``reused`` takes: [True, False, True] with a threshold of 0 (never fires by itself) — forward 0 still
    computes (nothing to reuse), forward 1 computes, forward 2 reuses, forward 3 follows the threshold again; and the reverse with inf"""
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, CONFIGS[0])
    cache = StepCache(0.0, forced=[True, False, True])
    for _ in range(4):
        _fwd(c, c["base"], cache)
    assert [d.reused for d in cache.decisions] == [False, False, True, False]
    assert cache.decisions[0].ratios is None and all(d.ratios == (0.0,) for d in cache.decisions[1:])
    cache = StepCache(math.inf, forced=[False, False, True])
    for _ in range(4):
        _fwd(c, c["far"], cache)
    assert [d.reused for d in cache.decisions] == [False, False, True, True]


def _fill_run(eng, gpu, steps=6):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(gpu)
    msk = torch.full((B, H, W), 255, dtype=torch.uint8); msk[:, 8:24, 8:40] = 0
    pe = torch.randn(B, 20, 256, generator=g).bfloat16().to(gpu); pp = torch.randn(B, 64, generator=g).bfloat16().to(gpu)
    en, nz, mn = generator_noise(1, B, H, W, 3)
    out = eng.pipe(img, msk.to(gpu), pe, pp, guidance_scale=30.0, num_inference_steps=steps, strength=1.0, enc_noise=en.to(gpu),
                   masked_enc_noise=mn.to(gpu), noise_tokens=pack_noise(nz).to(gpu))
    return out, (B, H, W, 3)


def _dev_run(eng, gpu, steps=6):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    pe = torch.randn(B, 20, 256, generator=g).bfloat16().to(gpu); pp = torch.randn(B, 64, generator=g).bfloat16().to(gpu)
    out = eng.pipe(pe, pp, height=H, width=W, guidance_scale=3.5, num_inference_steps=steps,
                   noise_tokens=pack_noise(generator_noise(1, B, H, W, 1)[0]).to(gpu))
    return out, (B, H, W, 3)


@pytest.mark.parametrize("kind", ["fill", "dev"])
def test_pipelines(gpu, kind):
    from domain_rag_amd import flux
    from domain_rag_amd.engine import Engine
    run = _fill_run if kind == "fill" else _dev_run
    eng = Engine(kind, synthetic=True, tiny=True, device=gpu, linear_precision="bf16", step_cache=math.inf)
    assert eng.pipe.step_cache == math.inf
    assert type(eng.pipe)(eng.pipe.tr, eng.pipe.vae).step_cache == flux.STEP_CACHE_DEFAULT        # None: $DRAG_STEP_CACHE, else off
    want = [False] + [True] * 5
    on, shape = run(eng, gpu)
    assert [d.reused for d in eng.pipe.last_step_decisions] == want and eng.pipe.last_step_decisions[0].ratios is None
    assert on.dtype == torch.uint8 and tuple(on.shape) == shape and bool(torch.isfinite(on.float()).all())
    again, _ = run(eng, gpu)          # the cache is reset at the start of a call: a computed first step and the same bytes
    assert [d.reused for d in eng.pipe.last_step_decisions] == want and torch.equal(on, again)
    eng.pipe.step_cache = None
    off, _ = run(eng, gpu)
    assert eng.pipe.last_step_decisions is None
    eng.pipe.step_cache = 0.0
    off0, _ = run(eng, gpu)
    assert torch.equal(off, off0) and eng.pipe.last_step_decisions is None
    assert not torch.equal(on, off)
    diff = (on.float() - off.float()).abs().mean().item()
    print(f"tiny {kind} pipeline, 6 steps, 1 computed + 5 reused: mean |level difference| vs off = {diff:.3f} of 255")
    # the same smoke once with MXFP8 Linears
    eng.pipe.tr.linear_precision = "mxfp8"
    eng.pipe.step_cache = math.inf
    mx, _ = run(eng, gpu)
    assert [d.reused for d in eng.pipe.last_step_decisions] == want
    assert mx.dtype == torch.uint8 and tuple(mx.shape) == shape and not torch.equal(mx, on)
