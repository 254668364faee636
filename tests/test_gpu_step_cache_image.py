"""The step cache's scope "image" (``step_cache.StepCache(scope="image")``): every image of a batch decides for itself, and a step on which only
some reuse runs the remaining blocks at the batch size of the others, on the same workspace with those images swapped to its front.

What is pinned, all of it bit for bit (nothing here has a tolerance: the per-image arithmetic of the forward does not depend on the batch
size once split-K is off, which ``ops.options(gemm_splitk=1)`` does for every test of the model — a split launch is the one documented place
where bits depend on M):
  * independence: an image's output and ratios are those of the run in which all images behave as it does, whatever its neighbour does;
  * state: a reusing image's F and R stay, a computing image's are rebuilt from the forward's own taps;
  * every mixed mask at B = 4 against the plain forward (computing images) and the all-reuse run (reusing images), with the launch records;
  * all-reuse and all-compute masks launch what scope "batch" launches;
  * invalidation per image, MXFP8 Linears, and the two pipelines through ``Engine``.
The configuration, inputs and threshold are those of tests/test_gpu_step_cache.py (copied: that file may change)."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
THRESHOLD = 0.15
NEAR, FAR = (0.005, 0.05), (0.5, 3.0)      # where the recorded ratios of a perturbed / an unrelated input must fall
TINY = (77, 12, 10, 2, 2, 384)             # St, latent h, w, double blocks, single blocks, in_channels


@pytest.fixture(autouse=True)
def _no_split_k():
    from domain_rag_amd import ops
    with ops.options(gemm_splitk=1):
        yield


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


def _case(gpu, B):
    """parameters, model and inputs (base, near = base + 0.01 N(0,1), far and other = unrelated draws) at batch B, built once"""
    if B in _cases:
        return _cases[B]
    from domain_rag_amd.flux import FluxTransformerHIP
    from domain_rag_amd.flux_params import FluxConfig
    cfg, params, inp = _setup(B, *TINY)
    hidden = inp[0]
    g = torch.Generator().manual_seed(99)
    near = (hidden.float() + 0.01 * torch.randn(hidden.shape, generator=g)).bfloat16()
    far = torch.randn(hidden.shape, generator=g).bfloat16()
    other = [torch.randn(hidden.shape, generator=g).bfloat16().to(gpu) for _ in range(4)]
    rest = (inp[1].to(gpu), inp[2].to(gpu)) + tuple(inp[3:])
    one_cfg = FluxConfig(**{**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__}, "num_layers": 1, "num_single_layers": 0})
    c = dict(cfg=cfg, one_cfg=one_cfg, params=params, B=B, St=TINY[0], base=hidden.to(gpu), near=near.to(gpu), far=far.to(gpu), other=other, rest=rest,
             model=FluxTransformerHIP(cfg, params, gpu, linear_precision="bf16"))
    _cases[B] = c
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


def _mix(first, second):
    """image 0 of ``first``, every other image of ``second``"""
    return torch.cat([first[:1], second[1:]]).contiguous()


def test_an_image_is_independent_of_its_neighbour(gpu):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, 2)
    mixed = _mix(c["near"], c["far"])
    # scope "batch", every image reuses: base then near
    all_near = StepCache(THRESHOLD)
    _fwd(c, c["base"], all_near)
    out_near = _fwd(c, c["near"], all_near)
    assert all_near.decisions[-1].reused and all_near.reused_images == [(False, False), (True, True)]
    # scope "batch", the mixed batch: nothing reuses (the situation of test_batch_rule_one_unrelated_image_blocks_the_reuse)
    batch = StepCache(THRESHOLD)
    _fwd(c, c["base"], batch)
    _fwd(c, mixed, batch)
    assert not batch.decisions[-1].reused and batch.reused_images[-1] == (False, False)
    plain = _fwd(c, mixed)
    # scope "image"
    cache = StepCache(THRESHOLD, scope="image")
    first = _fwd(c, c["base"], cache)
    out = _fwd(c, mixed, cache)
    d = cache.decisions[-1]
    print(f"ratios {d.ratios}")
    assert cache.reused_images == [(False, False), (True, False)] and d.reused is False and cache.decisions[0] == (None, False)
    assert NEAR[0] <= d.ratios[0] <= NEAR[1] and FAR[0] <= d.ratios[1] <= FAR[1]
    assert d.ratios == batch.decisions[-1].ratios and d.ratios[0] == all_near.decisions[-1].ratios[0]
    assert torch.equal(first, _fwd(c, c["base"]))
    assert torch.equal(out[0], out_near[0]), "the reusing image differs from the run in which every image reuses"
    assert torch.equal(out[1], plain[1]), "the computing image differs from the plain forward"
    assert not torch.equal(out[0], plain[0])


def test_four_forwards_with_another_neighbour(gpu):
    """image 0 sees base, near, near, base; its neighbour either base, far, far, near (computes, computes, reuses with ratio 0, computes)
    or four unrelated draws (computes every time): image 0's outputs and ratios are the same bits"""
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, 2)
    mine = [c["base"], c["near"], c["near"], c["base"]]
    runs = []
    for theirs in ([c["base"], c["far"], c["far"], c["near"]], c["other"]):
        cache = StepCache(THRESHOLD, scope="image")
        outs = [_fwd(c, _mix(a, b), cache) for a, b in zip(mine, theirs)]
        runs.append((cache, outs))
    (ca, oa), (cb, ob) = runs
    print(f"reused: {ca.reused_images} | {cb.reused_images}")
    assert ca.reused_images == [(False, False), (True, False), (True, True), (True, False)]
    assert cb.reused_images == [(False, False), (True, False), (True, False), (True, False)]
    assert ca.decisions[2].ratios[1] == 0.0
    for i in range(4):
        assert torch.equal(oa[i][0], ob[i][0]), f"forward {i}: image 0's output depends on its neighbour"
        if i:
            assert ca.decisions[i].ratios[0] == cb.decisions[i].ratios[0], f"forward {i}: image 0's ratio depends on its neighbour"


def test_state_after_a_mixed_step(gpu):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, 2)
    St = c["St"]
    last = f"single.{TINY[4] - 1}"
    mixed = _mix(c["near"], c["far"])
    cache = StepCache(THRESHOLD, scope="image")
    _fwd(c, c["base"], cache)
    F0, R0 = cache.F.clone(), cache.R.clone()
    t = {}
    _fwd(c, mixed, cache, t)
    assert cache.reused_images[-1] == (True, False) and cache.valid_images == [True, True]
    assert torch.equal(cache.F[0], F0[0]) and torch.equal(cache.R[0], R0[0]), "a reusing image's F and R must stay"
    d0_img = t["double.0"][:, St:]
    delta = (d0_img.float() - t["x_embed"].float()).bfloat16()
    assert torch.equal(t["cache.delta"], delta)
    assert torch.equal(cache.F[1], delta[1]) and not torch.equal(cache.F[1], F0[1])
    assert t["cache.slots"] == (1, 0) and t[last].shape[0] == 1          # image 1 ran alone, in slot 0
    R1 = (t[last][0, St:].float() - d0_img[1].float()).bfloat16()
    assert torch.equal(cache.R[1], R1)
    ratio0 = cache.decisions[-1].ratios[0]
    _fwd(c, mixed, cache)
    assert cache.decisions[-1].ratios == (ratio0, 0.0) and cache.reused_images[-1] == (True, True) and cache.decisions[-1].reused


_refs = {}


def _b4_refs(gpu):
    """at B = 4, once: the plain forward of ``far``, the all-reuse run (base computed, then far reused by every image), and per batch size
    k the launch records of a plain forward, split into [through block 0 | blocks 1... | tail] with a model of one double block"""
    if _refs:
        return _refs
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache
    c = _case(gpu, 4)
    B = 4
    _refs["plain"], g_full, a_full = _recorded(lambda: _fwd(c, c["far"]))
    cache = StepCache(0.0, scope="image", forced_images=[(False,) * B, (True,) * B])
    _fwd(c, c["base"], cache)
    _refs["reuse"], _refs["g_reuse"], _refs["a_reuse"] = _recorded(lambda: _fwd(c, c["far"], cache))
    assert cache.reused_images[-1] == (True,) * B
    full = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16")
    one = FluxTransformerHIP(c["one_cfg"], c["params"], gpu, linear_precision="bf16")
    enc, pooled, t, img_ids, txt_ids, gd = c["rest"]
    parts = {}
    for k in range(1, B + 1):
        args = (c["far"][:k].contiguous(), enc[:k].contiguous(), pooled[:k].contiguous(), t[:k], img_ids, txt_ids, gd[:k])
        _, g, a = _recorded(lambda: full.forward(*args).clone())
        _, g1, _ = _recorded(lambda: one.forward(*args).clone())
        n = len(g1) - 1          # the one-block model's launches but its proj_out: everything through block 0
        parts[k] = dict(head=g[:n], blocks=g[n:-1], tail=g[-1:], attn=a)
    assert parts[B]["head"] + parts[B]["blocks"] + parts[B]["tail"] == g_full and parts[B]["attn"] == a_full
    _refs["parts"] = parts
    return _refs


MIXED_MASKS = [m for m in itertools.product((False, True), repeat=4) if any(m) and not all(m)]


@pytest.mark.parametrize("mask", MIXED_MASKS, ids=lambda m: "".join("r" if v else "c" for v in m))
def test_every_mixed_mask_at_batch_four(gpu, mask):
    from domain_rag_amd.flux import StepCache
    assert len(MIXED_MASKS) == 14
    c, refs = _case(gpu, 4), _b4_refs(gpu)
    B, k = 4, mask.count(False)
    cache = StepCache(0.0, scope="image", forced_images=[(False,) * B, mask])
    _fwd(c, c["base"], cache)
    out, gemms, attn = _recorded(lambda: _fwd(c, c["far"], cache))
    assert cache.reused_images[-1] == mask and cache.decisions[-1].reused is False and cache.valid_images == [True] * B
    for b in range(B):
        want = refs["reuse"] if mask[b] else refs["plain"]
        assert torch.equal(out[b], want[b]), f"image {b} ({'reusing' if mask[b] else 'computing'}) differs"
    p = refs["parts"]
    assert gemms == p[B]["head"] + p[k]["blocks"] + p[B]["tail"]
    assert len(attn) == TINY[3] + TINY[4] and attn == p[B]["attn"][:1] + p[k]["attn"][1:]


def test_uniform_masks_launch_what_scope_batch_launches(gpu):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu, 4)
    B = 4
    for reuse in (True, False):
        runs = []
        for cache in (StepCache(0.0, forced=[False, reuse]), StepCache(0.0, forced=[False, reuse], scope="image"),
                      StepCache(0.0, scope="image", forced_images=[(False,) * B, (reuse,) * B])):
            first = _recorded(lambda: _fwd(c, c["base"], cache))
            second = _recorded(lambda: _fwd(c, c["far"], cache))
            assert cache.reused_images == [(False,) * B, (reuse,) * B] and cache.decisions[-1].reused is reuse
            runs.append((first, second, cache.decisions[-1].ratios))
        for other in runs[1:]:
            for (o0, g0, a0), (o1, g1, a1) in zip(runs[0][:2], other[:2]):
                assert torch.equal(o0, o1) and g0 == g1 and a0 == a1
            assert other[2] == runs[0][2]
    # ... and under the threshold rule: every image far -> all compute, every image repeated -> all reuse
    for scope in ("batch", "image"):
        cache = StepCache(THRESHOLD, scope=scope)
        for hidden in (c["base"], c["far"], c["far"]):
            _fwd(c, hidden, cache)
        assert cache.reused_images == [(False,) * B, (False,) * B, (True,) * B] and cache.decisions[-1].ratios == (0.0,) * B


def test_invalidation_per_image(gpu):
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache, latent_image_ids
    c = _case(gpu, 2)
    hidden, (enc, pooled, t, img_ids, txt_ids, gd) = c["base"], c["rest"]
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16")
    cache = StepCache(math.inf, scope="image")

    def step(h=hidden, e=enc, p=pooled, tt=t, ids=img_ids, g=gd):
        m.forward(h, e, p, tt, ids, txt_ids, g, cache=cache)
        assert cache.valid_images == [True] * h.shape[0]
        return cache.reused_images[-1]
    no2, yes2, no1, yes1 = (False, False), (True, True), (False,), (True,)
    assert [step(), step()] == [no2, yes2]
    one = (hidden[:1].contiguous(), enc[:1].contiguous(), pooled[:1].contiguous(), t[:1])
    assert [step(*one, g=gd[:1]), step(*one, g=gd[:1])] == [no1, yes1]                    # a changed B
    small = hidden[:1, :96].contiguous()                                                  # a changed Si (12 x 10 -> 12 x 8 latents)
    assert step(small, *one[1:], latent_image_ids(12, 8), gd[:1]) == no1
    assert [step(), step()] == [no2, yes2]
    m.linear_precision = "mxfp8"                                                          # a switch of the Linear precision, both ways
    assert [step(), step()] == [no2, yes2]
    m.linear_precision = "bf16"
    assert [step(), step()] == [no2, yes2]
    cache.reset()
    assert cache.decisions == [] and cache.reused_images == [] and not any(cache.valid_images)
    assert [step(), step()] == [no2, yes2] and cache.decisions[0].ratios is None
    # an invalid image computes whatever is forced; forwards beyond the pattern follow the threshold; NaN never reuses
    cache = StepCache(math.inf, scope="image", forced_images=[(True, True), (False, True)])
    assert [step(), step(), step()] == [no2, (False, True), yes2]
    with pytest.raises(ValueError, match="forced_images"):
        cache.configure(math.inf, None, "image", [(True,)])
        cache.reset()
        step()
    cache = StepCache(math.inf, scope="image")
    step()
    bad = hidden.clone()
    bad[1, 5, 7] = float("nan")
    assert step(bad) == (True, False) and math.isnan(cache.decisions[-1].ratios[1])
    with pytest.raises(ValueError, match="step cache"):
        m.forward_graphed(hidden, enc, pooled, t, img_ids, txt_ids, gd, cache=cache)


def test_mixed_mask_with_mxfp8_linears(gpu):
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache
    c = _case(gpu, 4)
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="mxfp8")
    mask = (True, False, True, False)
    cache = StepCache(0.0, scope="image", forced_images=[(False,) * 4, mask, (False, True, True, False)])
    outs = [_fwd(c, h, cache, model=m) for h in (c["base"], c["far"], c["near"])]
    assert cache.reused_images == [(False,) * 4, mask, (False, True, True, False)]
    assert all(bool(torch.isfinite(o.float()).all()) for o in outs)
    assert not torch.equal(outs[1], _fwd(c, c["far"]))


def _fill_run(eng, gpu, alter, steps=6):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    msk = torch.full((B, H, W), 255, dtype=torch.uint8); msk[:, 8:24, 8:40] = 0
    pe = torch.randn(B, 20, 256, generator=g).bfloat16(); pp = torch.randn(B, 64, generator=g).bfloat16()
    en, nz, mn = generator_noise(1, B, H, W, 3)
    nt = pack_noise(nz)
    if alter:          # other inputs for image 1
        img[1] = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        pe[1] = torch.randn(20, 256, generator=g).bfloat16(); pp[1] = torch.randn(64, generator=g).bfloat16()
        nt[1] = torch.randn(nt[1].shape, generator=g).to(nt.dtype)
    return eng.pipe(img.to(gpu), msk.to(gpu), pe.to(gpu), pp.to(gpu), guidance_scale=30.0, num_inference_steps=steps, strength=1.0, enc_noise=en.to(gpu),
                    masked_enc_noise=mn.to(gpu), noise_tokens=nt.to(gpu))


def _dev_run(eng, gpu, alter, steps=6):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    pe = torch.randn(B, 20, 256, generator=g).bfloat16(); pp = torch.randn(B, 64, generator=g).bfloat16()
    nt = pack_noise(generator_noise(1, B, H, W, 1)[0])
    if alter:
        pe[1] = torch.randn(20, 256, generator=g).bfloat16(); pp[1] = torch.randn(64, generator=g).bfloat16()
        nt[1] = torch.randn(nt[1].shape, generator=g).to(nt.dtype)
    return eng.pipe(pe.to(gpu), pp.to(gpu), height=H, width=W, guidance_scale=3.5, num_inference_steps=steps, noise_tokens=nt.to(gpu))


@pytest.mark.parametrize("kind", ["fill", "dev"])
def test_pipelines(gpu, kind):
    from domain_rag_amd import flux
    from domain_rag_amd.engine import Engine
    run = _fill_run if kind == "fill" else _dev_run
    eng = Engine(kind, synthetic=True, tiny=True, device=gpu, linear_precision="bf16", step_cache=math.inf, step_cache_scope="image")
    assert eng.pipe.step_cache_scope == "image"
    assert type(eng.pipe)(eng.pipe.tr, eng.pipe.vae).step_cache_scope == flux.STEP_CACHE_SCOPE_DEFAULT
    with pytest.raises(ValueError, match="scope"):
        type(eng.pipe)(eng.pipe.tr, eng.pipe.vae, step_cache_scope="junk")
    pattern = [(i % 2 == 1, i % 2 == 0) for i in range(6)]          # the two images take turns
    want = [(False, False)] + pattern[1:]                           # ... after a first step that has nothing to reuse
    eng.pipe.step_cache_forced_images = pattern
    on = run(eng, gpu, False)
    assert eng.pipe.last_step_reused_images == want and [d.reused for d in eng.pipe.last_step_decisions] == [False] * 6
    assert on.dtype == torch.uint8 and tuple(on.shape) == (2, 64, 96, 3)
    again = run(eng, gpu, False)
    assert eng.pipe.last_step_reused_images == want and torch.equal(on, again)
    other = run(eng, gpu, True)
    assert eng.pipe.last_step_reused_images == want
    assert torch.equal(on[0], other[0]), "image 0's bytes depend on image 1's inputs"
    assert not torch.equal(on[1], other[1])
    eng.pipe.step_cache = None
    run(eng, gpu, False)
    assert eng.pipe.last_step_decisions is None and eng.pipe.last_step_reused_images is None
