"""The Flux DiT with ``linear_precision="mxfp8"`` against the CPU oracle whose block Linears quantise their input and weight the same way.

The reference for the mode is ``oracle.flux.flux_forward`` in bf16 with ``oracle.flux._lin`` patched from here: the Linears that move
(both streams' q|k|v, the attention out-projections, ff up and down, the single blocks' q|k|v, proj_mlp and proj_out) compute
``linear(dequantize_ref(quantize_ref(x)), dequantize_ref(quantize_ref(W)))``.  The yardstick is the unpatched float32 oracle: the HIP output
may sit at most SLACK x further from it (rms-relative) than the patched oracle does — HIP is a second evaluation of the same graph.  No
absolute bar: a per-Linear rms error of about 4 % is the format's own.  The distances are recorded in profiles/mxfp8_dit_distance.json."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
SLACK = 1.3      # as tests/test_gpu_flux.py: HIP may sit at most this factor further from float32 than the reference evaluation does
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "mxfp8_dit_distance.json")
CONFIGS = [(1, 24, 6, 8, 1, 1, 64), (2, 77, 12, 10, 2, 2, 384)]         # the two configurations of test_flux_forward_vs_oracle
MOVES = re.compile(r"^(transformer_blocks\.\d+\.(attn\.(to_q|to_k|to_v|add_q_proj|add_k_proj|add_v_proj|to_out\.0|to_add_out)|ff(_context)?\.net\.(0\.proj|2))"
                   r"|single_transformer_blocks\.\d+\.(attn\.(to_q|to_k|to_v)|proj_mlp|proj_out))$")


def _record(key, values):
    """merge one case's figures into the record (the cases of this file write it one after the other)"""
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


def _mx_lin():
    """the patched ``oracle.flux._lin``: MX-quantised input and weight on the Linears that move, the plain Linear elsewhere"""
    import torch.nn.functional as F
    from domain_rag_amd import mx
    wcache = {}

    def rt(t):             # quantise -> dequantise along the last axis, back in t's dtype (exact: an e4m3 value times a power of two)
        return mx.dequantize_ref(*mx.quantize_ref(t.reshape(-1, t.shape[-1]))).reshape(t.shape).to(t.dtype)

    def lin(x, p, name):
        W, b = p[name + ".weight"], p.get(name + ".bias")
        if not MOVES.match(name):
            return F.linear(x, W, b)
        if name not in wcache:
            wcache[name] = rt(W)
        return F.linear(rt(x), wcache[name], b)
    return lin


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
        m.setattr(oflux, "_lin", _mx_lin())
        ref_mx = oflux.flux_forward(params, ocfg, hidden, enc, pooled, t, img_ids, txt_ids, gd, taps=taps_mx)
    dev_inp = (hidden.to(gpu), enc.to(gpu), pooled.to(gpu), t, img_ids, txt_ids, gd)
    c = dict(cfg=cfg, params=params, inp=dev_inp, ref32=ref32, ref_mx=ref_mx, taps32=taps32, taps_mx=taps_mx,
             mx=FluxTransformerHIP(cfg, params, gpu, linear_precision="mxfp8"), bf16=FluxTransformerHIP(cfg, params, gpu, linear_precision="bf16"))
    _cases[cfgt] = c
    return c


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_mxfp8_forward_vs_patched_oracle(gpu, cfgt, monkeypatch):
    c = _case(gpu, cfgt, monkeypatch)
    nl, ns = cfgt[4], cfgt[5]
    taps = {}
    out = c["mx"](*c["inp"], taps=taps).clone()
    out_bf16 = c["bf16"](*c["inp"]).clone()
    torch.cuda.synchronize()
    d_hip, d_oracle, d_bf16 = _rms_rel(out, c["ref32"]), _rms_rel(c["ref_mx"], c["ref32"]), _rms_rel(out_bf16, c["ref32"])
    print(f"{cfgt}: rms-relative distance from the float32 oracle: HIP mxfp8 {d_hip:.4e}, patched oracle {d_oracle:.4e}, HIP bf16 {d_bf16:.4e}; "
          f"HIP mxfp8 vs patched oracle {_rms_rel(out, c['ref_mx']):.4e}")
    _record("dit_B%d_St%d_%dx%d_L%d_S%d_in%d" % cfgt, dict(hip_mxfp8_vs_f32=d_hip, patched_oracle_vs_f32=d_oracle, hip_bf16_vs_f32=d_bf16,
                                                            ratio=d_hip / d_oracle, bar=SLACK))
    # per-block taps localise a failure: the same rule on every block's output
    for name in [f"double.{i}" for i in range(nl)] + [f"single.{i}" for i in range(ns)]:
        t_hip, t_or = _rms_rel(taps[name], c["taps32"][name]), _rms_rel(c["taps_mx"][name], c["taps32"][name])
        assert t_hip <= SLACK * t_or, f"{name}: HIP mxfp8 vs f32 {t_hip:.4e}, patched oracle vs f32 {t_or:.4e}, ratio {t_hip / t_or:.2f} (bar {SLACK})"
    assert d_hip <= SLACK * d_oracle, f"HIP mxfp8 vs f32 {d_hip:.4e}, patched oracle vs f32 {d_oracle:.4e}, ratio {d_hip / d_oracle:.2f} (bar {SLACK})"
    # the mode is engaged
    assert not torch.equal(out, out_bf16)


def test_launch_accounting_shows_the_mx_gemm(gpu, monkeypatch):
    from domain_rag_amd import ops
    c = _case(gpu, CONFIGS[1], monkeypatch)
    nl, ns = CONFIGS[1][4], CONFIGS[1][5]
    counts = {}
    for mode in ("mx", "bf16"):
        rec = ops.GemmRecorder()
        ops.set_recorder(rec)
        try:
            c[mode](*c["inp"])
        finally:
            ops.set_recorder(None)
        counts[mode] = {k: v[0] for k, v in rec.by_kernel().items()}
    mx_launches = sum(n for k, n in counts["mx"].items() if k.startswith("gemm_mxfp8"))
    # a double block: q|k|v, out-projection, ff up, ff down on both streams; a single block: q|k|v, proj_mlp, proj_out
    assert mx_launches == 8 * nl + 3 * ns, counts
    assert not any(k.startswith("gemm_mxfp8") for k in counts["bf16"]), counts
    # what stays bf16 in the mode: the two embedders, the time / text / guidance embedders, the stacked modulation, the final proj_out
    assert sum(n for k, n in counts["mx"].items() if not k.startswith("gemm_mxfp8")) == 2 + (6 if c["cfg"].guidance_embeds else 4) + 1 + 1, counts


def test_bf16_is_the_default_and_its_bits_do_not_change(gpu, monkeypatch):
    from domain_rag_amd import flux
    c = _case(gpu, CONFIGS[0], monkeypatch)
    default = flux.FluxTransformerHIP(c["cfg"], c["params"], gpu)
    assert default.linear_precision == (os.environ.get("DRAG_LINEAR_PRECISION") or "bf16")
    same = c["bf16"] if default.linear_precision == "bf16" else c["mx"]
    assert torch.equal(default(*c["inp"]), same(*c["inp"]))
    with pytest.raises(ValueError):
        default.linear_precision = "fp8"
    with pytest.raises(ValueError):
        flux.FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="int8")


def test_mxfp8_graph_replay_is_bit_identical(gpu, monkeypatch):
    c = _case(gpu, CONFIGS[1], monkeypatch)
    m = c["mx"]
    hidden, enc, pooled, _, img_ids, txt_ids, gd = c["inp"]
    for tt in (torch.tensor([0.9, 0.9]), torch.tensor([0.4, 0.4]), torch.tensor([0.05, 0.7])):
        eager = m.forward(hidden, enc, pooled, tt, img_ids, txt_ids, gd).clone()
        graphed = m.forward_graphed(hidden, enc, pooled, tt, img_ids, txt_ids, gd).clone()
        assert torch.equal(eager, graphed)
    assert len(m._graphs) == 1


def test_switching_the_precision_reproduces_bits(gpu, monkeypatch):
    """history: mxfp8 -> bf16 -> mxfp8 on ONE model (eager and graphed) gives each mode's bits every time, and they are the bits of
    models that never switched"""
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, CONFIGS[0], monkeypatch)
    want = {"mxfp8": c["mx"](*c["inp"]).clone(), "bf16": c["bf16"](*c["inp"]).clone()}
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="mxfp8")
    for mode in ("mxfp8", "bf16", "mxfp8", "bf16"):
        m.linear_precision = mode
        assert torch.equal(m.forward(*c["inp"]), want[mode]), mode
        assert torch.equal(m.forward_graphed(*c["inp"]), want[mode]), mode + " (graphed)"
    assert len(m._graphs) == 2          # one graph per precision: the key holds it


def test_fill_pipeline_smoke_in_mxfp8(gpu):
    """one tiny 2-step Fill pipeline through Engine(linear_precision="mxfp8"): shape, type, and a result that differs from bf16's"""
    from domain_rag_amd.engine import Engine, generator_noise, pack_noise
    eng = Engine("fill", synthetic=True, tiny=True, device=gpu, linear_precision="mxfp8")
    assert eng.pipe.tr.linear_precision == "mxfp8"
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
    eng.pipe.tr.linear_precision = "bf16"
    out_bf16 = run()
    torch.cuda.synchronize()
    assert out_mx.dtype == torch.uint8 and tuple(out_mx.shape) == (B, H, W, 3)
    assert bool(torch.isfinite(out_mx.float()).all())
    assert not torch.equal(out_mx, out_bf16)
    diff = (out_mx.float() - out_bf16.float()).abs().mean().item()
    print(f"tiny Fill pipeline, 2 steps: mean |level difference| mxfp8 vs bf16 = {diff:.3f} of 255")
    _record("fill_pipeline_tiny_2_steps", dict(mean_abs_level_difference_vs_bf16=diff))
