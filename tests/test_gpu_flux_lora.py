"""LoRA adapters merged into the Flux DiT's resident weights (``FluxTransformerHIP.load_lora``): the merged rows against the written-down
rule, the forward against the CPU oracle on merged weights, exact unload, independence of the load history, captured graphs, the MX
copies, both file spellings, and the public surface (Engine, compat pipelines, stage CLIs).

The adapter touches EVERY Linear of ``flux.linear_locations`` (modulation weights and embedders included), ranks alternating 4 and 16,
``down`` ~ N(0, 1/K), ``up`` ~ N(0, (0.25 std(W))^2 K / r): a delta of a quarter of the weight's std.  Measured with the CPU oracle, that
moves the float32 output by 41 % / 38 % rms-relative on the two configurations; the bf16 oracle sits 0.60 % / 0.65 % from float32 with the
adapter (HIP without it: 0.53 % / 0.59 %).  Forward bar, as tests/test_gpu_flux_mxfp8.py: HIP may sit at most SLACK x the bf16 oracle's
rms-relative distance from the float32 oracle (both on the float64-merged weights; the bf16 run on those weights rounded once).  The
distances are recorded in profiles/lora_dit_distance.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.bf16_bar import bar  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 1.3
MOVE = 0.10      # the adapter must move the float32 output at least this far (rms-relative): no assertion below passes vacuously
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "lora_dit_distance.json")
CONFIGS = [(1, 24, 6, 8, 1, 1, 64), (2, 77, 12, 10, 2, 2, 384)]         # the two configurations of test_flux_forward_vs_oracle


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


def _adapter(cfg, params, seed, names=None):
    """an Adapter over ``names`` (default: every Linear of the DiT), by the recipe of the module docstring"""
    from domain_rag_amd import lora
    from domain_rag_amd.flux import linear_locations
    g = torch.Generator().manual_seed(100 + seed)
    entries = {}
    for j, n in enumerate(sorted(names if names is not None else linear_locations(cfg))):
        N, K = params[n].shape
        r = (4, 16)[j % 2]
        down = (torch.randn(r, K, generator=g) / K ** 0.5).bfloat16()
        up = (torch.randn(N, r, generator=g) * (0.25 * params[n].float().std().item() * (K / r) ** 0.5)).bfloat16()
        entries[n] = (down, up, 1.0)
    return lora.Adapter(entries=entries)


def _write_peft(path, adapter, prefix="transformer."):
    from safetensors.torch import save_file
    sd = {}
    for n, (down, up, _) in adapter.entries.items():
        mod = prefix + n[: -len(".weight")]
        sd[mod + ".lora_A.weight"], sd[mod + ".lora_B.weight"] = down.contiguous(), up.contiguous()
    save_file(sd, str(path))
    return str(path)


def _resident(model) -> dict:
    """every resident tensor of a model by a stable key (an MX copy: its two tensors)"""
    out = {("w", k): v for k, v in model.w.items()}
    out[("mod_w",)], out[("mod_b",)] = model.mod_w, model.mod_b
    for kind, blocks in (("double", model.double), ("single", model.single)):
        for i, blk in enumerate(blocks):
            for k, v in blk.items():
                if isinstance(v, tuple):
                    out[(kind, i, k, "q")], out[(kind, i, k, "s")] = v
                else:
                    out[(kind, i, k)] = v
    return out


def _same_resident(a, b, what):
    ra, rb = _resident(a), _resident(b)
    assert set(ra) == set(rb), what
    diff = [k for k in ra if not torch.equal(ra[k], rb[k])]
    assert not diff, f"{what}: resident tensors differ: {diff[:6]}"


_cases = {}


def _case(gpu, cfgt):
    """the oracle evaluations of one configuration (float32 without the adapter, float32 and bf16 on the merged weights), computed once"""
    if cfgt in _cases:
        return _cases[cfgt]
    from domain_rag_amd import lora
    from oracle import flux as oflux
    cfg, params, inp = _setup(*cfgt)
    hidden, enc, pooled, t, img_ids, txt_ids, gd = inp
    ad = _adapter(cfg, params, 0)
    merged64 = {k: (lora.merge_ref(v, [ad.entries[k]]) if k in ad.entries else v.double()) for k, v in params.items()}
    ocfg = oflux.FluxConfig(**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__})
    f32 = lambda p: oflux.flux_forward({k: v.float() for k, v in p.items()}, ocfg, hidden.float(), enc.float(), pooled.float(), t, img_ids, txt_ids,
                                       gd, time_dtype=torch.bfloat16)
    ref32_plain, ref32 = f32(params), f32(merged64)
    merged_bf16 = {k: v.to(torch.bfloat16) for k, v in merged64.items()}
    ref_bf16 = oflux.flux_forward(merged_bf16, ocfg, hidden, enc, pooled, t, img_ids, txt_ids, gd)
    c = dict(cfg=cfg, params=params, adapter=ad, merged_bf16=merged_bf16, ref32_plain=ref32_plain, ref32=ref32, ref_bf16=ref_bf16,
             inp=(hidden.to(gpu), enc.to(gpu), pooled.to(gpu), t, img_ids, txt_ids, gd))
    _cases[cfgt] = c
    return c


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_resident_weights_follow_the_rule(gpu, cfgt):
    """(a) every target's resident rows against merge_ref; everything that is no target keeps its bits"""
    from domain_rag_amd.flux import FluxTransformerHIP, linear_locations
    c = _case(gpu, cfgt)
    fresh, model = FluxTransformerHIP(c["cfg"], c["params"], gpu), FluxTransformerHIP(c["cfg"], c["params"], gpu)
    ptrs = {k: v.data_ptr() for k, v in _resident(model).items()}
    name = model.load_lora(c["adapter"], name="all")
    torch.cuda.synchronize()
    assert name == "all" and model.loras == [dict(name="all", scale=1.0, ranks=[4, 16], targets=len(c["adapter"].entries))]
    loc = linear_locations(c["cfg"])
    assert set(c["adapter"].entries) == set(loc)
    worst = 1.0
    for n, (holder, row0, rows) in loc.items():
        got = model._holder(holder)[row0: row0 + rows].cpu()
        assert not torch.equal(got, c["params"][n]), f"{n}: not merged"
        worst = min(worst, bar(got, c["merged_bf16"][n], n))
    print(f"{cfgt}: least equal share over {len(loc)} Linears {worst:.4%}")
    holders = {h for h, _, _ in loc.values()}
    ra, rf = _resident(model), _resident(fresh)
    for k in ra:
        assert ra[k].data_ptr() == ptrs[k], f"{k} moved"
        if k not in holders:
            assert torch.equal(ra[k], rf[k]), f"{k} is no target and changed"


@pytest.mark.parametrize("cfgt", CONFIGS)
def test_forward_with_adapter_vs_oracle(gpu, cfgt):
    """(b) the forward on merged weights, and (c) exact unload"""
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, cfgt)
    model = FluxTransformerHIP(c["cfg"], c["params"], gpu)
    before = model(*c["inp"]).clone()
    model.load_lora(c["adapter"])
    out = model(*c["inp"]).clone()
    torch.cuda.synchronize()
    move = _rms_rel(c["ref32"], c["ref32_plain"])
    d_hip, d_or = _rms_rel(out, c["ref32"]), _rms_rel(c["ref_bf16"], c["ref32"])
    print(f"{cfgt}: the adapter moves the float32 output by {move:.4f}; distance from the float32 oracle: HIP {d_hip:.4e}, bf16 oracle {d_or:.4e}, "
          f"ratio {d_hip / d_or:.3f}; HIP without the adapter vs float32 without {_rms_rel(before, c['ref32_plain']):.4e}")
    _record("dit_B%d_St%d_%dx%d_L%d_S%d_in%d" % cfgt, dict(adapter_moves_f32_output=move, hip_vs_f32=d_hip, bf16_oracle_vs_f32=d_or,
                                                            ratio=d_hip / d_or, bar=SLACK))
    assert move >= MOVE, f"the adapter moves the output by only {move:.3f}"
    assert _rms_rel(out, before) >= MOVE
    assert d_hip <= SLACK * d_or, f"HIP vs f32 {d_hip:.4e}, bf16 oracle vs f32 {d_or:.4e}, ratio {d_hip / d_or:.2f} (bar {SLACK})"
    # (c) unload: the weights of a model that never saw the adapter, its forward, and no pristine copy left
    model.unload_lora()
    assert model.loras == [] and not model._pristine
    _same_resident(model, FluxTransformerHIP(c["cfg"], c["params"], gpu), "after unload")
    assert torch.equal(model(*c["inp"]), before)


def test_history_independence(gpu):
    """(d) the resident bits depend on the active adapters and their scales only"""
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, CONFIGS[0])
    cfg, params = c["cfg"], c["params"]
    A, B = c["adapter"], _adapter(cfg, params, 1, names=[n for j, n in enumerate(sorted(c["adapter"].entries)) if j % 3 != 1])
    m = FluxTransformerHIP(cfg, params, gpu)
    m.load_lora(A, name="A"); m.load_lora(B, 0.75, name="B")
    both = {k: v.clone() for k, v in _resident(m).items()}
    m.unload_lora("A")
    only_b = FluxTransformerHIP(cfg, params, gpu)
    only_b.load_lora(B, 0.75, name="B")
    _same_resident(m, only_b, "A, B, unload A vs B alone")
    assert any(not torch.equal(both[k], v) for k, v in _resident(m).items())
    # two adapters on one Linear are one launch over the concatenated ranks: against the rule
    from domain_rag_amd import lora
    from domain_rag_amd.flux import linear_locations
    n = sorted(B.entries)[0]
    holder, row0, rows = linear_locations(cfg)[n]
    d, u, _ = B.entries[n]
    bar(both[holder][row0: row0 + rows].cpu(), lora.merge_ref(params[n], [A.entries[n], (d, u, 0.75)]).to(torch.bfloat16), n + " (A + B)")
    m.set_lora_scale("B", -0.5)
    at_scale = FluxTransformerHIP(cfg, params, gpu)
    at_scale.load_lora(B, -0.5, name="B")
    _same_resident(m, at_scale, "set_lora_scale vs a fresh load at that scale")
    assert m.loras[0]["scale"] == -0.5
    m.unload_lora("B")
    assert not m._pristine
    _same_resident(m, FluxTransformerHIP(cfg, params, gpu), "all unloaded")
    with pytest.raises(KeyError):
        m.unload_lora("B")
    with pytest.raises(KeyError):
        m.set_lora_scale("nobody", 1.0)


def test_captured_graph_replays_the_merged_weights(gpu, monkeypatch):
    """(e) a graph captured before the load replays the new weights: one graph, the eager forward's bits"""
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, CONFIGS[1])
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu)
    pre = m.forward_graphed(*c["inp"]).clone()
    m.load_lora(c["adapter"])
    replay = m.forward_graphed(*c["inp"]).clone()
    eager = m.forward(*c["inp"]).clone()
    assert torch.equal(replay, eager)
    assert not torch.equal(replay, pre) and _rms_rel(replay, pre) >= MOVE
    assert len(m._graphs) == 1
    m.unload_lora()
    assert torch.equal(m.forward_graphed(*c["inp"]), pre) and len(m._graphs) == 1
    # a change while a stream is capturing is refused, by the model and by the wrapper (the query is patched: nothing is captured here)
    from domain_rag_amd import ops
    m.load_lora(c["adapter"], name="kept")
    w = m.w["x_embedder.weight"]
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        for change in (lambda: m.load_lora(c["adapter"]), lambda: m.unload_lora(), lambda: m.set_lora_scale("kept", 2.0)):
            with pytest.raises(RuntimeError, match="capturing"):
                change()
        with pytest.raises(RuntimeError, match="capture"):
            ops.lora_merge(w, w, torch.zeros(w.shape[0], 8, dtype=torch.bfloat16, device=gpu),
                           torch.zeros(8, w.shape[1], dtype=torch.bfloat16, device=gpu), torch.zeros(8, device=gpu))
    assert m.loras == [dict(name="kept", scale=1.0, ranks=[4, 16], targets=len(c["adapter"].entries))]
    assert torch.equal(m.forward(*c["inp"]), eager)


def test_mx_copies_follow(gpu):
    """(f) linear_precision="mxfp8": the MX copy of a touched weight is the quantiser's output on the merged weight, in the same buffers"""
    from domain_rag_amd import ops
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, CONFIGS[1])
    fresh = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="mxfp8")
    m = FluxTransformerHIP(c["cfg"], c["params"], gpu, linear_precision="mxfp8")
    ptrs = {k: v.data_ptr() for k, v in _resident(m).items()}
    before = m(*c["inp"]).clone()
    m.load_lora(c["adapter"])
    seen = 0
    for blocks in (m.double, m.single):
        for blk in blocks:
            for k in [k for k in blk if k.endswith("@mx")]:
                q, s = ops.quantize_mxfp8(blk[k[:-3]])
                assert torch.equal(blk[k][0], q) and torch.equal(blk[k][1], s), k
                seen += 1
    assert seen == 8 * len(m.double) + 2 * len(m.single)
    changed = [k for k, v in _resident(m).items() if k[-1] in ("q", "s") and not torch.equal(v, _resident(fresh)[k])]
    assert len(changed) == 2 * seen
    assert all(v.data_ptr() == ptrs[k] for k, v in _resident(m).items())
    assert _rms_rel(m(*c["inp"]), before) >= MOVE
    m.unload_lora()
    _same_resident(m, fresh, "mxfp8 model after unload")
    assert torch.equal(m(*c["inp"]), before)


def _kohya_pair(tmp_path, cfg, params):
    """one adapter over every name of the kohya table, written in the kohya and in the PEFT spelling (with alpha)"""
    from safetensors.torch import save_file
    from domain_rag_amd import lora
    g = torch.Generator().manual_seed(21)
    kohya, peft = {}, {}
    blocks = [("double", lora.KOHYA_DOUBLE, "transformer_blocks.", cfg.num_layers), ("single", lora.KOHYA_SINGLE, "single_transformer_blocks.", cfg.num_single_layers)]
    j = 0
    for kind, table, pre, count in blocks:
        for i in range(count):
            for kname, targets in table.items():
                r = (4, 16)[j % 2]; j += 1
                ws = [params[f"{pre}{i}.{t}.weight"] for t in targets]
                K = ws[0].shape[1]
                down = (torch.randn(r, K, generator=g) / K ** 0.5).bfloat16()
                up = (torch.randn(sum(w.shape[0] for w in ws), r, generator=g) * (0.25 * ws[0].float().std().item() * (K / r) ** 0.5)).bfloat16()
                base = f"lora_unet_{kind}_blocks_{i}_{kname}"
                kohya[base + ".lora_down.weight"], kohya[base + ".lora_up.weight"], kohya[base + ".alpha"] = down, up, torch.tensor(float(r) / 2)
                row0 = 0
                for t, w in zip(targets, ws):
                    mod = f"transformer.{pre}{i}.{t}"
                    peft[mod + ".lora_A.weight"], peft[mod + ".lora_B.weight"] = down.clone(), up[row0: row0 + w.shape[0]].contiguous()
                    peft[mod + ".alpha"] = torch.tensor(float(r) / 2)
                    row0 += w.shape[0]
    kp, pp = str(tmp_path / "kohya.safetensors"), str(tmp_path / "peft.safetensors")
    save_file(kohya, kp); save_file(peft, pp)
    return kp, pp


def test_file_spellings_give_the_same_bits(gpu, tmp_path):
    """(g) the kohya file and the PEFT file of one adapter"""
    from domain_rag_amd.flux import FluxTransformerHIP
    c = _case(gpu, CONFIGS[1])
    kp, pp = _kohya_pair(tmp_path, c["cfg"], c["params"])
    a, b = FluxTransformerHIP(c["cfg"], c["params"], gpu), FluxTransformerHIP(c["cfg"], c["params"], gpu)
    assert a.load_lora(kp) == "kohya" and b.load_lora(pp, name="kohya") == "kohya"
    _same_resident(a, b, "kohya vs PEFT file")
    assert a.loras == b.loras and a.loras[0]["targets"] == 20 * 2
    fresh = _resident(FluxTransformerHIP(c["cfg"], c["params"], gpu))
    assert sum(not torch.equal(v, fresh[k]) for k, v in _resident(a).items()) == 1 + 8 * 2 + 2 * 2      # mod_w, the blocks' weights


# ---------------------------------------------------------------------------------------------- (h) the public surface
def _tiny_fill_adapter(tmp_path):
    from domain_rag_amd.engine import TINY
    from domain_rag_amd.flux_params import FluxConfig, init_params
    cfg = FluxConfig(in_channels=384, **TINY["flux"])
    return _write_peft(tmp_path / "domain.safetensors", _adapter(cfg, init_params(cfg, seed=0), 5))


def _fill_inputs(gpu, B=1, H=64, W=96):
    from domain_rag_amd.engine import generator_noise, pack_noise
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(gpu)
    msk = torch.full((B, H, W), 255, dtype=torch.uint8); msk[:, 8:24, 8:40] = 0
    pe = torch.randn(B, 20, 256, generator=g).bfloat16().to(gpu); pp = torch.randn(B, 64, generator=g).bfloat16().to(gpu)
    en, nz, mn = generator_noise(1, B, H, W, 3)
    return (img, msk.to(gpu), pe, pp), dict(guidance_scale=30.0, num_inference_steps=2, strength=0.9, enc_noise=en.to(gpu),
                                            masked_enc_noise=mn.to(gpu), noise_tokens=pack_noise(nz).to(gpu))


def test_engine_takes_adapters(gpu, tmp_path):
    from domain_rag_amd.engine import Engine
    path = _tiny_fill_adapter(tmp_path)
    args, kw = _fill_inputs(gpu)
    plain = Engine("fill", synthetic=True, tiny=True, device=gpu)
    out0 = plain.pipe(*args, **kw).clone()
    eng = Engine("fill", synthetic=True, tiny=True, device=gpu, lora=[f"{path}:1.0"])
    assert [a["name"] for a in eng.pipe.tr.loras] == ["domain"]
    out1 = eng.pipe(*args, **kw).clone()
    assert out1.dtype == torch.uint8 and out1.shape == out0.shape and bool(torch.isfinite(out1.float()).all())
    assert not torch.equal(out1, out0)
    # the pass-through methods: the same bits as the constructor's list, and back
    name = plain.load_lora(path)
    assert torch.equal(plain.pipe(*args, **kw), out1)
    plain.set_lora_scale(name, 0.5)
    half = plain.pipe(*args, **kw).clone()
    assert not torch.equal(half, out1) and not torch.equal(half, out0)
    plain.unload_lora()
    assert torch.equal(plain.pipe(*args, **kw), out0)
    half_eng = Engine("fill", synthetic=True, tiny=True, device=gpu, lora=[(path, 0.5)])
    assert torch.equal(half_eng.pipe(*args, **kw), half)


def test_compat_pipeline_lora_methods(gpu, tmp_path, monkeypatch):
    from PIL import Image
    from domain_rag_amd import compat
    monkeypatch.setenv("DRAG_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("DRAG_TINY", "1")
    path = _tiny_fill_adapter(tmp_path)
    rng = np.random.default_rng(0)
    image = Image.fromarray(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8))
    mask = Image.fromarray(np.where(rng.integers(0, 256, (64, 96)) > 100, 255, 0).astype(np.uint8), mode="L")
    g = torch.Generator().manual_seed(2)
    pe, pp = torch.randn(1, 20, 256, generator=g).bfloat16().to(gpu), torch.randn(1, 64, generator=g).bfloat16().to(gpu)

    def run(p):
        return np.asarray(p(image=image, mask_image=mask, height=64, width=96, guidance_scale=30.0, num_inference_steps=2, prompt_embeds=pe,
                            pooled_prompt_embeds=pp, generator=torch.Generator("cpu").manual_seed(7), strength=0.9).images[0])
    pipe = compat.FluxFillPipeline.from_pretrained("./model/FLUX.1-Fill-dev", torch_dtype=torch.bfloat16).to("cuda")
    out0 = run(pipe)
    pipe.load_lora_weights(str(tmp_path), weight_name="domain.safetensors", adapter_name="dom")
    pipe.fuse_lora(); pipe.unfuse_lora()
    out1 = run(pipe)
    assert not np.array_equal(out1, out0)
    pipe.set_adapters(["dom"], adapter_weights=[0.5])
    out_half = run(pipe)
    assert not np.array_equal(out_half, out1) and not np.array_equal(out_half, out0)
    with pytest.raises(ValueError, match="set_adapters"):
        pipe.fuse_lora(lora_scale=0.5)
    with pytest.raises(ValueError, match="not loaded"):
        pipe.set_adapters(["other"])
    pipe.unload_lora_weights()
    assert np.array_equal(run(pipe), out0)
    # calls made before .to("cuda") are queued and applied when the model is built; a directory with one file needs no weight_name
    late = compat.FluxFillPipeline.from_pretrained("./model/FLUX.1-Fill-dev", torch_dtype=torch.bfloat16)
    late.load_lora_weights(str(tmp_path), adapter_name="dom")
    late.set_adapters("dom", 0.5)
    late = late.to("cuda")
    assert [(a["name"], a["scale"]) for a in late.tr.loras] == [("dom", 0.5)]
    assert np.array_equal(run(late), out_half)


def _run_cli(mod, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, DRAG_TIMESTAMP="20260101_000000")
    r = subprocess.run([sys.executable, "-m", mod] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_stage3_cli_lora_flag_and_manifest(gpu, tmp_path):
    from PIL import Image
    path = _tiny_fill_adapter(tmp_path)
    rng = np.random.default_rng(1)
    root, ds, name = tmp_path, "DIOR", "plane_7"
    (root / "datasets" / ds / "annotations").mkdir(parents=True); (root / "datasets" / ds / "train").mkdir(parents=True)
    Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(root / "datasets" / ds / "train" / f"{name}.jpg")
    json.dump({"images": [{"id": 1, "file_name": f"{name}.jpg", "width": 56, "height": 40}],
               "annotations": [{"id": 1, "image_id": 1, "bbox": [8, 6, 20, 14], "category_id": 1}], "categories": [{"id": 1, "name": "airplane"}]},
              open(root / "datasets" / ds / "annotations" / "1_shot.json", "w"))
    sdir = root / "result" / f"{ds}_1shot_retrieval" / "results_x" / name
    sdir.mkdir(parents=True)
    Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(sdir / "generated_image_rank1.png")
    common = ["--dataset", ds, "--shot", "1", "--synthetic-weights", "--tiny", "--num_inference_steps", "2", "--seed", "5", "--io_workers", "0"]
    _run_cli("domain_rag_amd.cli.stage3_outpaint", ["--process_id", "plain"] + common, cwd=root)
    _run_cli("domain_rag_amd.cli.stage3_outpaint", ["--process_id", "lora"] + common + ["--lora", f"{path}:0.5"], cwd=root)
    d0, d1 = (root / "outpaint_hires" / f"process_{p}" / ds / "1_shot" / name for p in ("plain", "lora"))
    pre = f"{ds}_{name}_1shot"
    p0, p1 = json.load(open(d0 / f"{pre}_params_1.json")), json.load(open(d1 / f"{pre}_params_1.json"))
    assert "lora" not in p0 and p1["lora"] == [{"file": "domain.safetensors", "scale": 0.5}]
    assert set(p1) - set(p0) == {"lora"} and all(p1[k] == p0[k] for k in ("strength", "guidance_scale", "seed", "num_bbox"))
    a, b = np.asarray(Image.open(d0 / f"{pre}_hires_result_1.png")), np.asarray(Image.open(d1 / f"{pre}_hires_result_1.png"))
    assert a.shape == b.shape and not np.array_equal(a, b)


def test_stage2_cli_lora_flag_and_params_line(gpu, tmp_path):
    from PIL import Image
    from domain_rag_amd.engine import TINY
    from domain_rag_amd.flux_params import FluxConfig, init_params
    cfg = FluxConfig(in_channels=64, **TINY["flux"])
    path = _write_peft(tmp_path / "dev_domain.safetensors", _adapter(cfg, init_params(cfg, seed=0), 6))
    rng = np.random.default_rng(2)
    root, ds = tmp_path, "ArTaxOr"
    (root / "coco").mkdir(); (root / "lamainpaint" / ds / "1_shot").mkdir(parents=True); (root / "rr").mkdir()
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)).save(root / "coco" / f"{i:06d}.jpg")
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(root / "lamainpaint" / ds / "1_shot" / "beetle_01.jpg")
    json.dump({}, open(root / "rr" / "all_shots_retrieval_results.json", "w"))        # no entry: the seeded random-corpus fallback
    common = ["--dataset", ds, "--shots", "1", "--retrieval_results_dir", "rr", "--coco_dir", "coco", "--synthetic-weights", "--tiny",
              "--num_inference_steps", "2", "--fallback-seed", "0", "--io_workers", "0"]
    _run_cli("domain_rag_amd.cli.stage2_generate", common + ["--output_dir", "plain"], cwd=root)
    _run_cli("domain_rag_amd.cli.stage2_generate", common + ["--output_dir", "lora", "--lora", path, "--lora", f"{path}:0.25"], cwd=root)
    sub = os.path.join(f"{ds}_1shot_retrieval", "results_coco_0.8_target_1.0_cocotext_1.0_targettext_1.0_20260101_000000", "beetle_01")
    t0, t1 = (open(root / o / sub / "params.txt", encoding="utf-8").read() for o in ("plain", "lora"))
    line = "LoRA: dev_domain.safetensors:1.0, dev_domain.safetensors:0.25\n"
    assert "LoRA" not in t0 and t1 == t0 + line
    a, b = (np.asarray(Image.open(root / o / sub / "generated_image_rank1.png")) for o in ("plain", "lora"))
    assert a.shape == b.shape and not np.array_equal(a, b)
