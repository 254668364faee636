"""The denoise loop of the two pipelines (``FluxTxt2ImgHIP``, ``FluxFillHIP``) against the same loop spelled out here: the eager
``tr.forward(...)`` and ``ops.flow_euler_rows(...)`` step by step, for Fill between the public calls the pipeline makes before and after
its loop.  Every ``on_step`` latent and the final uint8 image must be equal bit for bit, with the hipGraph replay on and off, with a
sampling recorder (a mix of eager and replayed steps) and with a forced step-cache pattern against ``forward(..., cache=StepCache(...))``.

The tiny model of ``engine.TINY``, B = 2, 64 x 64 pixels (16 image tokens), 16 text tokens.  The hand loops run once per pipeline and
cache pattern and are shared by the cases."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
B, H, W, ST = 2, 64, 64, 16
DEV_STEPS, FILL_STEPS, FILL_STRENGTH = 3, 4, 0.5
DEV_GUIDANCE, FILL_GUIDANCE = 3.5, 30.0
DEV_FORCED, FILL_FORCED = [False, True, False], [False, True]

_engines, _inputs, _hand = {}, {}, {}


def _engine(gpu, kind):
    if kind not in _engines:
        from domain_rag_amd.engine import Engine
        _engines[kind] = Engine(kind, synthetic=True, tiny=True, device=gpu, linear_precision="bf16")
    return _engines[kind]


def _input(gpu):
    if not _inputs:
        from domain_rag_amd.engine import generator_noise, pack_noise
        g = torch.Generator().manual_seed(11)
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        msk = torch.full((B, H, W), 255, dtype=torch.uint8); msk[:, 16:40, 8:48] = 0
        pe, pp = torch.randn(B, ST, 256, generator=g).bfloat16(), torch.randn(B, 64, generator=g).bfloat16()
        en, nz, mn = generator_noise(5, B, H, W, 3)
        _inputs.update(img=img.to(gpu), msk=msk.to(gpu), pe=pe.to(gpu), pp=pp.to(gpu), en=en.to(gpu), mn=mn.to(gpu), noise=pack_noise(nz).to(gpu))
    return _inputs


def _hand_cache(pipe, forced):
    from domain_rag_amd.flux import StepCache
    return None if forced is None else StepCache(math.inf, forced=forced, scope=pipe.step_cache_scope)


def _hand_dev(gpu, forced=None):
    """FluxTxt2ImgHIP's call by hand -> ([latents after each step], uint8 image, the cache's decisions)"""
    if ("dev", forced is not None) in _hand:
        return _hand[("dev", forced is not None)]
    from domain_rag_amd import ops
    from domain_rag_amd.flux import latent_image_ids
    from domain_rag_amd.scheduler import flow_sigmas, model_timestep
    pipe, inp = _engine(gpu, "dev").pipe, _input(gpu)
    tr, cache = pipe.tr, _hand_cache(pipe, forced)
    h, w = H // 16, W // 16
    lat, pe, pp = inp["noise"].clone(), inp["pe"].clone(), inp["pp"].clone()
    sigmas, timesteps = flow_sigmas(DEV_STEPS, h * w)
    img_ids, txt_ids = latent_image_ids(h, w), torch.zeros(ST, 3)
    guidance = torch.full((B,), DEV_GUIDANCE) if tr.cfg.guidance_embeds else None
    lats = []
    for i in range(DEV_STEPS):
        t = torch.full((B,), model_timestep(timesteps[i]))
        v = tr.forward(lat, pe, pp, t, img_ids, txt_ids, guidance, cache=cache)
        ops.flow_euler_rows(lat, v, B * h * w, 64, 64, 64, float(sigmas[i + 1] - sigmas[i]))
        lats.append((i, lat.clone()))
    out = pipe.vae.decode_tokens(lat, B, h, w, ld=64).clone()
    _hand[("dev", forced is not None)] = (lats, out, None if cache is None else list(cache.decisions))
    return _hand[("dev", forced is not None)]


def _hand_fill(gpu, forced=None):
    """FluxFillHIP's call by hand: the two VAE encodes, mask pack and noise scaling, the loop from ``strength_start`` on, the decode"""
    if ("fill", forced is not None) in _hand:
        return _hand[("fill", forced is not None)]
    from domain_rag_amd import ops
    from domain_rag_amd.flux import latent_image_ids
    from domain_rag_amd.scheduler import flow_sigmas, model_timestep, strength_start
    pipe, inp = _engine(gpu, "fill").pipe, _input(gpu)
    tr, cache = pipe.tr, _hand_cache(pipe, forced)
    h, w = H // 16, W // 16
    Si, C = h * w, tr.cfg.in_channels
    hidden = torch.empty((B, Si, C), dtype=torch.bfloat16, device=gpu)
    hv, pe, pp = hidden.view(-1), inp["pe"].clone(), inp["pp"].clone()
    pipe.vae.encode_to_tokens(inp["img"], None, inp["en"], hv, C)
    pipe.vae.encode_to_tokens(inp["img"], inp["msk"], inp["mn"], hv[64:], C)
    ops.mask_pack(inp["msk"], hv[128:], B, H, W, C)
    sigmas, timesteps = flow_sigmas(FILL_STEPS, Si)
    t0 = strength_start(FILL_STEPS, FILL_STRENGTH)
    assert t0 == 2, "the case is meant to begin the loop after step 0"
    ops.scale_noise_rows(hv, inp["noise"], B * Si, 64, C, 64, float(sigmas[t0]))
    img_ids, txt_ids = latent_image_ids(h, w), torch.zeros(ST, 3)
    guidance = torch.full((B,), FILL_GUIDANCE)
    lats = []
    for i in range(t0, FILL_STEPS):
        t = torch.full((B,), model_timestep(timesteps[i]))
        v = tr.forward(hidden, pe, pp, t, img_ids, txt_ids, guidance, cache=cache)
        ops.flow_euler_rows(hv, v, B * Si, 64, C, 64, float(sigmas[i + 1] - sigmas[i]))
        lats.append((i, hidden[:, :, :64].clone()))
    out = pipe.vae.decode_tokens(hv, B, h, w, ld=C).clone()
    _hand[("fill", forced is not None)] = (lats, out, None if cache is None else list(cache.decisions))
    return _hand[("fill", forced is not None)]


def _run_dev(gpu, use_graph, forced=None):
    pipe, inp = _engine(gpu, "dev").pipe, _input(gpu)
    pipe.use_graph, pipe.step_cache, pipe.step_cache_forced = use_graph, (None if forced is None else math.inf), forced
    got = []
    try:
        out = pipe(inp["pe"], inp["pp"], height=H, width=W, guidance_scale=DEV_GUIDANCE, num_inference_steps=DEV_STEPS,
                   noise_tokens=inp["noise"], on_step=lambda i, lat: got.append((i, lat)))
    finally:
        pipe.use_graph, pipe.step_cache, pipe.step_cache_forced = True, None, None
    return got, out, pipe.last_step_decisions


def _run_fill(gpu, use_graph, forced=None, recorder=None):
    pipe, inp = _engine(gpu, "fill").pipe, _input(gpu)
    pipe.use_graph, pipe.step_cache, pipe.step_cache_forced = use_graph, (None if forced is None else math.inf), forced
    got = []
    try:
        out = pipe(inp["img"], inp["msk"], inp["pe"], inp["pp"], guidance_scale=FILL_GUIDANCE, num_inference_steps=FILL_STEPS,
                   strength=FILL_STRENGTH, enc_noise=inp["en"], masked_enc_noise=inp["mn"], noise_tokens=inp["noise"], recorder=recorder,
                   on_step=lambda i, lat: got.append((i, lat)))
    finally:
        pipe.use_graph, pipe.step_cache, pipe.step_cache_forced = True, None, None
    return got, out, pipe.last_step_decisions


def _assert_same(got, want, n_steps):
    (lats, out, _), (wlats, wout, _) = got, want
    assert [i for i, _ in lats] == [i for i, _ in wlats] and len(lats) == n_steps
    for (i, a), (_, b) in zip(lats, wlats):
        assert a.dtype == torch.bfloat16 and tuple(a.shape) == (B, (H // 16) * (W // 16), 64)
        assert torch.equal(a, b), f"latents after step {i} differ"
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, 3)
    assert torch.equal(out, wout), "the final image differs"


@pytest.mark.parametrize("use_graph", [True, False])
def test_txt2img_loop(gpu, use_graph):
    want = _hand_dev(gpu)
    got = _run_dev(gpu, use_graph)
    _assert_same(got, want, DEV_STEPS)
    assert got[2] is None


@pytest.mark.parametrize("use_graph", [True, False])
def test_fill_loop_from_a_later_first_step(gpu, use_graph):
    want = _hand_fill(gpu)
    got = _run_fill(gpu, use_graph)
    _assert_same(got, want, FILL_STEPS - 2)
    assert [i for i, _ in got[0]] == [2, 3] and got[2] is None


def test_fill_loop_with_a_sampling_recorder(gpu):
    """``GemmRecorder(every=2)``: the loop's first step runs eagerly under the recorder, its second replays the graph"""
    from domain_rag_amd import ops
    rec = ops.GemmRecorder(every=2)
    _assert_same(_run_fill(gpu, True, recorder=rec), _hand_fill(gpu), FILL_STEPS - 2)
    assert rec.totals()[2] > 0


def test_txt2img_loop_with_a_forced_step_cache(gpu):
    want = _hand_dev(gpu, DEV_FORCED)
    got = _run_dev(gpu, True, DEV_FORCED)
    _assert_same(got, want, DEV_STEPS)
    assert [d.reused for d in want[2]] == DEV_FORCED == [d.reused for d in got[2]]


def test_fill_loop_with_a_forced_step_cache(gpu):
    want = _hand_fill(gpu, FILL_FORCED)
    got = _run_fill(gpu, True, FILL_FORCED)
    _assert_same(got, want, FILL_STEPS - 2)
    assert [d.reused for d in want[2]] == FILL_FORCED == [d.reused for d in got[2]]
