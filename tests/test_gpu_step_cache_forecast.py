"""The step cache's order 1 at the level of the DiT forward (``step_cache.StepCache(order=1)``): a reused step adds the first-order forecast
``R + c (R - P)`` of the remaining-blocks residual instead of R itself.

Everything is bit for bit (split-K is off for every test of the model, as in tests/test_gpu_step_cache_image.py, whose configuration and
inputs are copied here: that file may change):
  * fallback: with fewer than two computed steps behind an image, or two at the same timestep, order 1 IS order 0 — bits, launches, record;
  * the forecast pinned from the cache's own state: P is the R of the step before, and the image rows after the reuse are the float32
    restatement (tests/helpers/stepcache_forecast_ref.py) of the rows after block 0, R, P and the coefficient of the three timesteps;
  * scope "image" at B = 4: a forecasting, an order-0 and two computing images in one step, each equal to its own run at B = 1;
  * invalidation, the two pipelines through ``Engine`` and the stage CLIs' written parameters."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import stepcache_forecast_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
TINY = (77, 12, 10, 2, 2, 384)             # St, latent h, w, double blocks, single blocks, in_channels
C, R = False, True


@pytest.fixture(autouse=True)
def _no_split_k():
    from domain_rag_amd import ops
    with ops.options(gemm_splitk=1):
        yield


_cases = {}


def _case(gpu, B=4):
    """parameters, model and four input draws at batch 4, built once; a smaller batch takes the first images of these"""
    if not _cases:
        from domain_rag_amd.flux import FluxTransformerHIP, latent_image_ids
        from domain_rag_amd.flux_params import FluxConfig, init_params
        St, h, w, nl, ns, inch = TINY
        cfg = FluxConfig(in_channels=inch, num_layers=nl, num_single_layers=ns, num_attention_heads=2, joint_attention_dim=128, pooled_projection_dim=64)
        params = init_params(cfg, seed=0)
        g = torch.Generator().manual_seed(1)
        hidden = [torch.randn(4, h * w, inch, generator=g).bfloat16().to(gpu) for _ in range(4)]
        hidden[1] = (hidden[0].float() + 0.01 * torch.randn(hidden[0].shape, generator=g).to(gpu)).bfloat16()      # a step that barely moved
        enc = torch.randn(4, St, cfg.joint_attention_dim, generator=g).bfloat16().to(gpu)
        pooled = torch.randn(4, cfg.pooled_projection_dim, generator=g).bfloat16().to(gpu)
        _cases.update(cfg=cfg, params=params, St=St, hidden=hidden, enc=enc, pooled=pooled, ids=(latent_image_ids(h, w), torch.zeros(St, 3)),
                      model=FluxTransformerHIP(cfg, params, gpu, linear_precision="bf16"))
    return _cases


def _times(i, B=4):
    """the model timesteps of forward ``i``: another one per image, all distinct over the forwards, as float32"""
    return torch.tensor([0.9 - 0.13 * i - 0.02 * b for b in range(B)], dtype=torch.float32)


def _fwd(c, i, cache=None, taps=None, images=slice(0, 4), times=None, model=None, hidden=None):
    """forward number ``i`` (input draw i, timesteps ``_times(i)``) of the images ``images``"""
    h = (c["hidden"][i] if hidden is None else hidden)[images].contiguous()
    B = h.shape[0]
    t = (_times(i) if times is None else times)[images]
    return (model or c["model"]).forward(h, c["enc"][images].contiguous(), c["pooled"][images].contiguous(), t, *c["ids"], torch.full((B,), 30.0),
                                         taps=taps, cache=cache).clone()


def _coef(i_now, i_last, i_prev, b):
    from domain_rag_amd.step_cache import forecast_coefficient
    return forecast_coefficient(_times(i_now)[b].item(), _times(i_last)[b].item(), _times(i_prev)[b].item())


def _recorded(fn):
    from domain_rag_amd import ops
    rec = ops.GemmRecorder()
    ops.set_recorder(rec)
    try:
        out = fn()
    finally:
        ops.set_recorder(None)
    torch.cuda.synchronize()
    return out, [(s, rec.kernel_of(s, k)) for s, k in zip(rec.shapes, rec.is_conv)], [a[3] for a in rec.attn]


@pytest.mark.parametrize("scope", ["batch", "image"])
def test_one_computed_step_behind_is_order_zero(gpu, scope):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu)
    runs = []
    for order in (0, 1):
        cache = StepCache(0.0, forced=[C, R], scope=scope, order=order)
        runs.append((cache, [_recorded(lambda i=i: _fwd(c, i, cache, images=slice(0, 2))) for i in range(2)]))
    (c0, r0), (c1, r1) = runs
    assert c1.reused_images == c0.reused_images == [(C, C), (R, R)]
    for (o0, g0, a0), (o1, g1, a1) in zip(r0, r1):
        assert torch.equal(o0, o1) and g0 == g1 and a0 == a1
    assert c1.forecasts == c0.forecasts == [(None, None), (None, None)]
    assert c1.has_prev == [False, False] and c0.P is None and c1.P is not None


def test_forecast_pinned_from_the_state(gpu):
    from domain_rag_amd.flux import StepCache
    c = _case(gpu)
    St, B = c["St"], 2
    two = slice(0, B)
    cache = StepCache(0.0, forced=[C, C, R], order=1)
    _fwd(c, 0, cache, images=two)
    R_first = cache.R.clone()
    _fwd(c, 1, cache, images=two)
    R_now, P_now = cache.R.clone(), cache.P.clone()
    assert torch.equal(P_now, R_first), "P must be the R of the computed step before the last one"
    assert not torch.equal(R_now, R_first) and cache.has_prev == [True, True]
    taps = {}
    out = _fwd(c, 2, cache, taps, images=two)
    coefs = tuple(_coef(2, 1, 0, b) for b in range(B))
    assert cache.reused_images[-1] == (R, R) and cache.forecasts == [(None, None), (None, None), coefs]
    assert all(v is not None and abs(v - 1.0) < 1e-5 for v in coefs) and taps["cache.forecast"] == ((0, 1), coefs)
    assert torch.equal(cache.R, R_now) and torch.equal(cache.P, P_now), "a reused step leaves R and P alone"
    x_after_block0 = taps["double.0"][:, St:]
    for b in range(B):
        want = ref.forecast(x_after_block0[b], R_now[b], P_now[b], coefs[b])
        assert torch.equal(taps["cache.x_img"][b].cpu(), want), f"image {b}: the rows after the reuse are not the restated forecast"
    # ... and order 0 gives other bits on the same three forwards
    plain = StepCache(0.0, forced=[C, C, R])
    outs = [_fwd(c, i, plain, images=two) for i in range(3)]
    assert plain.forecasts == [(None, None)] * 3 and not torch.equal(outs[2], out)


def test_equal_timesteps_fall_back(gpu):
    """two computed steps at the same timestep leave nothing to extrapolate along: order-0 bits, None in the record"""
    from domain_rag_amd.flux import StepCache
    c = _case(gpu)
    two, outs = slice(0, 2), []
    for order in (0, 1):
        cache = StepCache(0.0, forced=[C, C, R], order=order)
        outs.append([_fwd(c, i, cache, images=two, times=_times(0) if i < 2 else None) for i in range(3)])
        assert cache.reused_images[-1] == (R, R) and cache.forecasts[-1] == (None, None)
    assert cache.has_prev == [True, True] and cache.t_last == cache.t_prev
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# scope "image" at B = 4, four forwards; image 1 is invalidated before forward 2.  On forward 3: image 0 forecasts (computed at 0 and 1),
# image 1 reuses at order 0 (one computed step, forward 2, behind it), images 2 and 3 compute
MASKS = [(C, C, C, C), (C, C, C, C), (R, C, C, R), (R, R, C, C)]


def _four_forwards(c, images, before_last=None):
    from domain_rag_amd.flux import StepCache
    n = len(range(*images.indices(4)))
    cache = StepCache(0.0, scope="image", forced_images=[m[images] for m in MASKS], order=1)
    outs = []
    for i in range(4):
        if i == 2:
            lo = images.indices(4)[0]
            if lo <= 1 < lo + n:
                cache.valid_images[1 - lo] = False          # what a per-image invalidation leaves behind
        if i == 3 and before_last is not None:
            before_last(cache)
        outs.append(_fwd(c, i, cache, images=images))
    return cache, outs


def test_scope_image_mixed_step_against_every_image_alone(gpu):
    c = _case(gpu)
    state = {}
    cache, outs = _four_forwards(c, slice(0, 4), lambda k: state.update(R=k.R.clone(), P=k.P.clone()))
    assert cache.reused_images == MASKS
    c0_2, c3_2, c0_3 = _coef(2, 1, 0, 0), _coef(2, 1, 0, 3), _coef(3, 1, 0, 0)
    assert cache.forecasts == [(None,) * 4, (None,) * 4, (c0_2, None, None, c3_2), (c0_3, None, None, None)]
    assert cache.has_prev == [True, False, True, True] and cache.valid_images == [True] * 4
    # the state after the mixed step: a computing image that was valid has its former R in P; a reusing image's R and P are untouched
    for b in (2, 3):
        assert torch.equal(cache.P[b], state["R"][b]) and not torch.equal(cache.R[b], state["R"][b]), f"computing image {b}"
    for b in (0, 1):
        assert torch.equal(cache.R[b], state["R"][b]) and torch.equal(cache.P[b], state["P"][b]), f"reusing image {b}"
    for b in range(4):
        alone, outs1 = _four_forwards(c, slice(b, b + 1))
        assert alone.reused_images == [(m[b],) for m in MASKS] and alone.forecasts == [(f[b],) for f in cache.forecasts], f"image {b}"
        for i in range(4):
            assert torch.equal(outs[i][b], outs1[i][0]), f"forward {i}: image {b} differs from its own run at B = 1"


def test_a_precision_change_clears_the_forecast_state(gpu):
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache
    c = _case(gpu)
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16")
    cache = StepCache(0.0, forced=[C, C, R, R, R, C, R], order=1)
    two = slice(0, 2)
    draws = [0, 1, 1, 2, 2, 3, 3]

    def step(i):
        _fwd(c, i, cache, images=two, model=m, hidden=c["hidden"][draws[i]], times=torch.tensor([0.95 - 0.1 * i, 0.9 - 0.1 * i]))
        return cache.reused_images[-1], cache.forecasts[-1]
    assert [step(i)[0] for i in range(2)] == [(C, C), (C, C)]
    mask, fc = step(2)
    assert mask == (R, R) and all(v is not None for v in fc)
    m.linear_precision = "mxfp8"
    assert step(3) == ((C, C), (None, None)) and cache.has_prev == [False, False]          # forced to reuse, but invalid: computes
    assert step(4) == ((R, R), (None, None))                                              # one computed step behind: order 0
    assert step(5) == ((C, C), (None, None)) and cache.has_prev == [True, True]
    mask, fc = step(6)
    assert mask == (R, R) and all(v is not None for v in fc)
    cache.reset()
    assert cache.forecasts == [] and cache.has_prev == [False, False] and cache.t_last == [None, None]


def _fill_run(eng, gpu, steps=6):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    msk = torch.full((B, H, W), 255, dtype=torch.uint8); msk[:, 8:24, 8:40] = 0
    pe = torch.randn(B, 20, 256, generator=g).bfloat16(); pp = torch.randn(B, 64, generator=g).bfloat16()
    en, nz, mn = generator_noise(1, B, H, W, 3)
    return eng.pipe(img.to(gpu), msk.to(gpu), pe.to(gpu), pp.to(gpu), guidance_scale=30.0, num_inference_steps=steps, strength=1.0, enc_noise=en.to(gpu),
                    masked_enc_noise=mn.to(gpu), noise_tokens=pack_noise(nz).to(gpu))


def _dev_run(eng, gpu, steps=6):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    pe = torch.randn(B, 20, 256, generator=g).bfloat16(); pp = torch.randn(B, 64, generator=g).bfloat16()
    nt = pack_noise(generator_noise(1, B, H, W, 1)[0])
    return eng.pipe(pe.to(gpu), pp.to(gpu), height=H, width=W, guidance_scale=3.5, num_inference_steps=steps, noise_tokens=nt.to(gpu))


@pytest.mark.parametrize("kind", ["fill", "dev"])
def test_pipelines(gpu, kind):
    from domain_rag_amd import flux
    from domain_rag_amd.engine import Engine
    from domain_rag_amd.scheduler import flow_sigmas, model_timestep
    from domain_rag_amd.step_cache import forecast_coefficient
    run = _fill_run if kind == "fill" else _dev_run
    eng = Engine(kind, synthetic=True, tiny=True, device=gpu, linear_precision="bf16", step_cache=math.inf, step_cache_order=1)
    pipe = eng.pipe
    assert (pipe.step_cache_order, pipe.step_cache_max_run, pipe.step_cache_warmup) == (1, 0, 0)
    bare = type(pipe)(pipe.tr, pipe.vae)
    assert (bare.step_cache_order, bare.step_cache_max_run, bare.step_cache_warmup) == (flux.STEP_CACHE_ORDER_DEFAULT, flux.STEP_CACHE_MAX_RUN_DEFAULT,
                                                                                       flux.STEP_CACHE_WARMUP_DEFAULT)
    with pytest.raises(ValueError, match="order"):
        type(pipe)(pipe.tr, pipe.vae, step_cache_order=2)
    pattern = [C, C, R, C, R, R]
    pipe.step_cache_forced = pattern
    on = run(eng, gpu)
    assert [d.reused for d in pipe.last_step_decisions] == pattern
    # the coefficients from the scheduler's own timesteps, as the loop hands them to the model (float32 holds a model timestep exactly)
    _, ts = flow_sigmas(6, (64 // 16) * (96 // 16))
    t = [model_timestep(v) for v in ts]
    want, t_last, t_prev = [], None, None
    for i, reused in enumerate(pattern):
        if reused:
            want.append((forecast_coefficient(t[i], t_last, t_prev),) * 2)
        else:
            want.append((None, None))
            t_last, t_prev = t[i], t_last
    assert pipe.last_step_forecasts == want and [w[0] is not None for w in want] == pattern
    assert want[5][0] > want[4][0] > 0          # |c| grows with the length of a run
    pipe.step_cache_order = 0
    zero = run(eng, gpu)
    assert pipe.last_step_forecasts == [(None, None)] * 6 and [d.reused for d in pipe.last_step_decisions] == pattern
    assert not torch.equal(on, zero), "order 1 and order 0 give the same bytes: the switch was dropped on the way down"
    # the limits reach the cache too: threshold inf, no forced pattern
    pipe.step_cache_forced, pipe.step_cache_order, pipe.step_cache_max_run, pipe.step_cache_warmup = None, 1, 2, 2
    run(eng, gpu)
    assert [d.reused for d in pipe.last_step_decisions] == [C, C, R, R, C, R]
    # off: the three switches do nothing — the bytes of an engine built without them
    pipe.step_cache = None
    off = run(eng, gpu)
    assert pipe.last_step_decisions is None and pipe.last_step_forecasts is None
    plain = Engine(kind, synthetic=True, tiny=True, device=gpu, linear_precision="bf16")
    if plain.pipe.step_cache is None:          # (a process default would turn the cache on)
        assert torch.equal(off, run(plain, gpu))


def test_stage_clis_write_the_switches(gpu, tmp_path, monkeypatch):
    """stages 2 and 3 on a one-sample dataset with ``--step_cache 1e9 --step_cache_order 1 --step_cache_max_run 2`` and without the two new
    flags: the written parameters name a switch exactly when it is not the default"""
    from PIL import Image
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    rng = np.random.default_rng(1)
    root = tmp_path
    ds, name = "DIOR", "plane_7"
    for d in (root / "datasets" / ds / "annotations", root / "datasets" / ds / "train", root / "lamainpaint" / ds / "1_shot", root / "coco", root / "rr"):
        d.mkdir(parents=True)
    Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(root / "datasets" / ds / "train" / f"{name}.jpg")
    Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(root / "lamainpaint" / ds / "1_shot" / f"{name}.jpg")
    Image.fromarray(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)).save(root / "coco" / "000001.jpg")
    json.dump({"images": [{"id": 1, "file_name": f"{name}.jpg", "width": 56, "height": 40}],
               "annotations": [{"id": 1, "image_id": 1, "bbox": [8, 6, 20, 14], "category_id": 1}], "categories": [{"id": 1, "name": "airplane"}]},
              open(root / "datasets" / ds / "annotations" / "1_shot.json", "w"))
    json.dump({}, open(root / "rr" / "all_shots_retrieval_results.json", "w"))          # no entry: the one corpus image is the fallback
    monkeypatch.chdir(root)
    flags = ["--step_cache_order", "1", "--step_cache_max_run", "2"]
    common = ["--synthetic-weights", "--tiny", "--num_inference_steps", "4", "--io_workers", "0", "--step_cache", "1e9"]
    for tag, extra in (("new", flags), ("old", [])):
        monkeypatch.setenv("DRAG_TIMESTAMP", tag)
        assert stage2_generate.main(["--dataset", ds, "--shots", "1", "--retrieval_results_dir", "rr", "--output_dir", "result", "--coco_dir", "coco",
                                     "--fallback-seed", "0"] + common + extra) == 0
        assert stage3_outpaint.main(["--process_id", tag, "--dataset", ds, "--shot", "1", "--seed", "5"] + common + extra) == 0
    base = root / "result" / f"{ds}_1shot_retrieval"
    new_txt, old_txt = (open(base / f"results_coco_0.8_target_1.0_cocotext_1.0_targettext_1.0_{tag}" / name / "params.txt", encoding="utf-8").read()
                        for tag in ("new", "old"))
    assert old_txt == new_txt.replace(stage2_generate.params_txt_step_cache(1e9, "batch", 1, 2), stage2_generate.params_txt_step_cache(1e9))
    assert new_txt.endswith(stage2_generate.params_txt_step_cache(1e9, "batch", 1, 2)) and new_txt.count("\n") == old_txt.count("\n") + 2
    assert [line.rsplit(": ", 1)[1] for line in new_txt.splitlines()[-2:]] == ["1", "2"]
    new_js, old_js = (json.load(open(root / "outpaint_hires" / f"process_{tag}" / ds / "1_shot" / name / f"{ds}_{name}_1shot_params_1.json"))
                      for tag in ("new", "old"))
    assert new_js["step_cache"] == old_js["step_cache"] == 1e9 and new_js["step_cache_order"] == 1 and new_js["step_cache_max_run"] == 2
    assert "step_cache_warmup" not in new_js and "step_cache_scope" not in new_js
    assert not any(k in old_js for k in ("step_cache_order", "step_cache_max_run", "step_cache_warmup"))
    assert set(new_js) - set(old_js) == {"step_cache_order", "step_cache_max_run"}
