"""The Flux DiT with ``attention_precision="mxfp8"`` against the CPU oracle whose attention is the host restatement of the format.

The reference for the mode is ``oracle.flux.flux_forward`` in bf16 with ``oracle.flux.sdpa`` patched from here to ``mx.attention_ref`` per batch
and head.  The yardstick is the unpatched float32 oracle: the HIP output may sit at most SLACK x further from it (rms-relative) than the
patched oracle does, on the output and on every block's tap — HIP is a second evaluation of the same graph.  The distances (the mode, the
patched oracle, bf16, and both MX modes together) go to profiles/attn_mxfp8_dit_distance.json."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
SLACK = 1.3      # as tests/test_gpu_flux.py and tests/test_gpu_flux_mxfp8.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "attn_mxfp8_dit_distance.json")
CONFIGS = [(1, 24, 6, 8, 1, 1, 64), (2, 77, 12, 10, 2, 2, 384)]         # the two configurations of tests/test_gpu_flux_mxfp8.py


def _record(key, values):
    try:
        with open(RECORD) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        rec = {}
    rec[key] = values
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


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


def _mx_sdpa(q, k, v):
    """the patched ``oracle.flux.sdpa``: [B, H, S, 128] prepared q, k, v -> ``mx.attention_ref`` per batch and head"""
    from domain_rag_amd import mx
    scale = 1 / math.sqrt(q.shape[-1])
    return torch.stack([torch.stack([mx.attention_ref(q[b, h].bfloat16(), k[b, h].bfloat16(), v[b, h].bfloat16(), scale)
                                     for h in range(q.shape[1])]) for b in range(q.shape[0])]).to(q.dtype)


_cases = {}


def _case(gpu, cfgt, monkeypatch):
    """oracle evaluations and HIP models of one configuration, computed once and shared by the tests below"""
    if cfgt in _cases:
        return _cases[cfgt]
    from domain_rag_amd.flux import FluxTransformerHIP
    from oracle import flux as oflux
    cfg, params, inp = _setup(*cfgt)
    hidden, enc, pooled, t, img_ids, txt_ids, gd = inp
    ocfg = oflux.FluxConfig(**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__})
    taps32, taps_mx = {}, {}
    p32 = {k: v.float() for k, v in params.items()}
    ref32 = oflux.flux_forward(p32, ocfg, hidden.float(), enc.float(), pooled.float(), t, img_ids, txt_ids, gd, taps=taps32, time_dtype=torch.bfloat16)
    with monkeypatch.context() as m:
        m.setattr(oflux, "sdpa", _mx_sdpa)
        ref_mx = oflux.flux_forward(params, ocfg, hidden, enc, pooled, t, img_ids, txt_ids, gd, taps=taps_mx)
    dev_inp = (hidden.to(gpu), enc.to(gpu), pooled.to(gpu), t, img_ids, txt_ids, gd)
    c = dict(cfg=cfg, params=params, inp=dev_inp, ref32=ref32, ref_mx=ref_mx, taps32=taps32, taps_mx=taps_mx,
             mx=FluxTransformerHIP(cfg, params, gpu, linear_precision="bf16", attention_precision="mxfp8"),
             bf16=FluxTransformerHIP(cfg, params, gpu, linear_precision="bf16", attention_precision="bf16"))
    _cases[cfgt] = c
    return c


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_mxfp8_attention_forward_vs_patched_oracle(gpu, cfgt, monkeypatch):
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, cfgt, monkeypatch)
    nl, ns = cfgt[4], cfgt[5]
    taps = {}
    out = c["mx"](*c["inp"], taps=taps).clone()
    out_bf16 = c["bf16"](*c["inp"]).clone()
    both = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="mxfp8", attention_precision="mxfp8")
    out_both = both(*c["inp"]).clone()
    torch.cuda.synchronize()
    d_hip, d_oracle, d_bf16, d_both = (_rms_rel(out, c["ref32"]), _rms_rel(c["ref_mx"], c["ref32"]), _rms_rel(out_bf16, c["ref32"]),
                                       _rms_rel(out_both, c["ref32"]))
    print(f"{cfgt}: rms-relative distance from the float32 oracle: HIP mxfp8 attention {d_hip:.4e}, patched oracle {d_oracle:.4e}, HIP bf16 {d_bf16:.4e}, "
          f"HIP mxfp8 attention + mxfp8 Linears {d_both:.4e}; HIP mxfp8 attention vs patched oracle {_rms_rel(out, c['ref_mx']):.4e}")
    _record("dit_B%d_St%d_%dx%d_L%d_S%d_in%d" % cfgt, dict(hip_mxfp8_attention_vs_f32=d_hip, patched_oracle_vs_f32=d_oracle, hip_bf16_vs_f32=d_bf16,
                                                            hip_mxfp8_attention_and_linears_vs_f32=d_both, ratio=d_hip / d_oracle, bar=SLACK))
    for name in [f"double.{i}" for i in range(nl)] + [f"single.{i}" for i in range(ns)]:
        t_hip, t_or = _rms_rel(taps[name], c["taps32"][name]), _rms_rel(c["taps_mx"][name], c["taps32"][name])
        print(f"  {name}: HIP {t_hip:.4e}, patched oracle {t_or:.4e}, ratio {t_hip / t_or:.3f}")
        assert t_hip <= SLACK * t_or, f"{name}: HIP mxfp8 attention vs f32 {t_hip:.4e}, patched oracle vs f32 {t_or:.4e}, ratio {t_hip / t_or:.2f} (bar {SLACK})"
    assert d_hip <= SLACK * d_oracle, f"HIP mxfp8 attention vs f32 {d_hip:.4e}, patched oracle vs f32 {d_oracle:.4e}, ratio {d_hip / d_oracle:.2f} (bar {SLACK})"
    # the mode is engaged, and independent of the Linears' mode
    assert not torch.equal(out, out_bf16) and not torch.equal(out_both, out)
    assert both.linear_precision == "mxfp8" and both.attention_precision == "mxfp8" and c["mx"].linear_precision == "bf16"


def test_launch_accounting_shows_the_mx_attention(gpu, monkeypatch):
    """in the mode every block launches the MX prep pass and the MX kernel and no bf16 attention or prep pass; bf16 launches neither"""
    from domain_rag_amd import ops
    c = _case(gpu, CONFIGS[1], monkeypatch)
    nl, ns = CONFIGS[1][4], CONFIGS[1][5]
    calls = {}
    for name in ("qkv_prep_mxfp8", "k_norm_rope_vt", "qk_norm_rope_vt"):
        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    seen = {}
    for mode in ("mx", "bf16"):
        calls.clear()
        rec = ops.GemmRecorder()
        ops.set_recorder(rec)
        try:
            c[mode](*c["inp"])
        finally:
            ops.set_recorder(None)
        seen[mode] = ({k: v[0] for k, v in rec.attention_by_kernel().items()}, dict(calls), rec.attention_by_kernel())
    kernels, preps, full = seen["mx"]
    assert list(kernels) == ["attention_mxfp8_kernel<1, 8>"] and kernels["attention_mxfp8_kernel<1, 8>"] == nl + ns, kernels
    assert preps == {"qkv_prep_mxfp8": nl + ns}, preps
    B, S, H = CONFIGS[1][0], CONFIGS[1][1] + CONFIGS[1][2] * CONFIGS[1][3], 2
    assert full["attention_mxfp8_kernel<1, 8>"][2] == (nl + ns) * 4.0 * S * S * 128 * H * B          # the bf16 launches' FLOP count
    kernels, preps, _ = seen["bf16"]
    assert sum(kernels.values()) == nl + ns and not any("mxfp8" in k for k in kernels), kernels
    assert "qkv_prep_mxfp8" not in preps and sum(preps.values()) == nl + ns, preps


def _parent_attention(self, ws, nb, S, St, wq_txt, wk_txt, wq_img, wk_img, cos, sin, out, ld_o, scale):
    """the launches both block kinds made before the mode existed"""
    from domain_rag_amd import ops
    D, H = self.cfg.dim, self.cfg.num_attention_heads
    qkv, vt = ws["qkv"], ws["vt"]
    ops.k_norm_rope_vt(qkv, vt, wk_txt, wk_img, cos, sin, nb, S, H, 3 * D, St)
    ops.attention_qprep(qkv, qkv.view(-1)[D:], vt, out, nb, S, H, 3 * D, S * 3 * D, ld_o, S * ld_o, scale, wq_txt, wq_img, cos, sin, St)


def test_bf16_is_the_default_and_its_bits_do_not_change(gpu, monkeypatch):
    from domain_rag_amd import flux
    c = _case(gpu, CONFIGS[0], monkeypatch)
    default = flux.FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16")          # attention_precision=None
    assert default.attention_precision == (os.environ.get("DRAG_ATTENTION_PRECISION") or "bf16")
    same = c["bf16"] if default.attention_precision == "bf16" else c["mx"]
    want = same(*c["inp"]).clone()
    assert torch.equal(default(*c["inp"]), want)
    # ... and they are the bits of the route as it was before the mode existed
    if not flux._SEPARATE_QPREP:
        fresh = flux.FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16", attention_precision="bf16")
        with monkeypatch.context() as m:
            m.setattr(flux.FluxTransformerHIP, "_attention", _parent_attention)
            assert torch.equal(fresh(*c["inp"]), c["bf16"](*c["inp"]).clone())
    with pytest.raises(ValueError):
        default.attention_precision = "fp8"
    with pytest.raises(ValueError):
        flux.FluxTransformerHIP(c["cfg"], c["params"], gpu, attention_precision="int8")


def test_mxfp8_attention_graph_replay_is_bit_identical(gpu, monkeypatch):
    c = _case(gpu, CONFIGS[1], monkeypatch)
    m = c["mx"]
    hidden, enc, pooled, _, img_ids, txt_ids, gd = c["inp"]
    for tt in (torch.tensor([0.9, 0.9]), torch.tensor([0.4, 0.4]), torch.tensor([0.05, 0.7])):
        eager = m.forward(hidden, enc, pooled, tt, img_ids, txt_ids, gd).clone()
        graphed = m.forward_graphed(hidden, enc, pooled, tt, img_ids, txt_ids, gd).clone()
        assert torch.equal(eager, graphed)
    assert len(m._graphs) == 1


def test_switching_the_attention_precision_reproduces_bits(gpu, monkeypatch):
    """history: bf16 -> mxfp8 -> bf16 -> mxfp8 on ONE model (eager and graphed) gives each mode's bits every time, and they are the bits of
    models that never switched"""
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, CONFIGS[0], monkeypatch)
    want = {"mxfp8": c["mx"](*c["inp"]).clone(), "bf16": c["bf16"](*c["inp"]).clone()}
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16", attention_precision="bf16")
    for mode in ("bf16", "mxfp8", "bf16", "mxfp8"):
        m.attention_precision = mode
        assert torch.equal(m.forward(*c["inp"]), want[mode]), mode
        assert torch.equal(m.forward_graphed(*c["inp"]), want[mode]), mode + " (graphed)"
    assert len(m._graphs) == 2          # one graph per precision: the key holds it


def test_step_cache_with_the_mode(gpu, monkeypatch):
    """the step cache over the mode: a computed step gives the plain forward's bits, a repeated input is reused, and a switch of the
    attention precision invalidates the cache (its residual belongs to the other mode's blocks)"""
    from domain_rag_amd.flux import FluxTransformerHIP, StepCache
    c = _case(gpu, CONFIGS[1], monkeypatch)
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="bf16", attention_precision="mxfp8")
    plain = c["mx"](*c["inp"]).clone()
    cache = StepCache(math.inf)
    first = m.forward(*c["inp"], cache=cache).clone()
    second = m.forward(*c["inp"], cache=cache).clone()
    assert [d.reused for d in cache.decisions] == [False, True]
    assert torch.equal(first, plain)
    assert bool(torch.isfinite(second.float()).all()) and _rms_rel(second, plain) < 1e-2      # the same input: the cached residual is this step's
    m.attention_precision = "bf16"
    third = m.forward(*c["inp"], cache=cache).clone()
    assert cache.decisions[-1].reused is False and torch.equal(third, c["bf16"](*c["inp"]))
    m.attention_precision = "mxfp8"
    m.forward(*c["inp"], cache=cache)
    assert cache.decisions[-1].reused is False


def test_fill_pipeline_smoke_in_mxfp8_attention(gpu):
    """one tiny 2-step Fill pipeline through Engine(attention_precision="mxfp8"): shape, type, and a result that differs from bf16's"""
    from domain_rag_amd.engine import Engine, generator_noise, pack_noise
    eng = Engine("fill", synthetic=True, tiny=True, device=gpu, linear_precision="bf16", attention_precision="mxfp8")
    assert eng.pipe.tr.attention_precision == "mxfp8" and eng.pipe.tr.linear_precision == "bf16"
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 64, 96
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(gpu)
    msk = torch.full((B, H, W), 255, dtype=torch.uint8); msk[:, 8:24, 8:40] = 0
    pe = torch.randn(B, 20, 256, generator=g).bfloat16().to(gpu); pp = torch.randn(B, 64, generator=g).bfloat16().to(gpu)
    en, nz, mn = generator_noise(1, B, H, W, 3)

    def run():
        return eng.pipe(img, msk.to(gpu), pe, pp, guidance_scale=30.0, num_inference_steps=2, strength=0.9, enc_noise=en.to(gpu),
                        masked_enc_noise=mn.to(gpu), noise_tokens=pack_noise(nz).to(gpu))
    out_mx = run()
    eng.pipe.tr.attention_precision = "bf16"
    out_bf16 = run()
    torch.cuda.synchronize()
    assert out_mx.dtype == torch.uint8 and tuple(out_mx.shape) == (B, H, W, 3)
    assert bool(torch.isfinite(out_mx.float()).all())
    assert not torch.equal(out_mx, out_bf16)
    diff = (out_mx.float() - out_bf16.float()).abs().mean().item()
    print(f"tiny Fill pipeline, 2 steps: mean |level difference| mxfp8 attention vs bf16 = {diff:.3f} of 255")
    _record("fill_pipeline_tiny_2_steps", dict(mean_abs_level_difference_vs_bf16=diff))
