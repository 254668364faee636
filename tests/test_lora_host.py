"""LoRA adapters, host side (no GPU): reading both file spellings into one representation, every refusal, the written-down merge rule,
the ``PATH[:SCALE]`` argument, the table of where the DiT keeps each Linear, and the C ABI's refusals before any launch."""
import ctypes

import pytest
import torch
from safetensors.torch import save_file

from domain_rag_amd import lora
from domain_rag_amd.flux import linear_locations
from domain_rag_amd.flux_params import FluxConfig, param_shapes

CFG = FluxConfig(in_channels=64, num_layers=2, num_single_layers=2, num_attention_heads=2, joint_attention_dim=128, pooled_projection_dim=64)
D, F = CFG.dim, CFG.mlp_ratio * CFG.dim


def _rand(g, *shape):
    return (0.1 * torch.randn(*shape, generator=g)).bfloat16()


def _adapter_files(tmp_path, alpha=True, prefix="transformer."):
    """one adapter in both spellings: block 1 of each kind, every kohya name of the table, the fused ones included (their q / k / v
    [/ proj_mlp] share ``down`` in the PEFT file, which is what a split fused entry is)"""
    g = torch.Generator().manual_seed(11)
    kohya, peft, want = {}, {}, {}
    for kind, table, pre in (("double", lora.KOHYA_DOUBLE, "transformer_blocks.1."), ("single", lora.KOHYA_SINGLE, "single_transformer_blocks.1.")):
        shapes = param_shapes(CFG)
        for j, (kname, targets) in enumerate(table.items()):
            r = (4, 16)[j % 2]
            rows = [shapes[pre + t + ".weight"][0] for t in targets]
            K = shapes[pre + targets[0] + ".weight"][1]
            down, up = _rand(g, r, K), _rand(g, sum(rows), r)
            a = float(r // 2 + j)
            base = f"lora_unet_{kind}_blocks_1_{kname}"
            kohya[base + ".lora_down.weight"], kohya[base + ".lora_up.weight"] = down, up
            if alpha:
                kohya[base + ".alpha"] = torch.tensor(a)
            row0 = 0
            for t, nr in zip(targets, rows):
                peft[f"{prefix}{pre}{t}.lora_A.weight"] = down.clone()
                peft[f"{prefix}{pre}{t}.lora_B.weight"] = up[row0: row0 + nr].clone()
                if alpha:
                    peft[f"{prefix}{pre}{t}.alpha"] = torch.tensor(a)
                want[pre + t + ".weight"] = (down, up[row0: row0 + nr], a / r if alpha else 1.0)
                row0 += nr
    kp, pp = str(tmp_path / f"kohya_{alpha}.safetensors"), str(tmp_path / f"peft_{alpha}_{len(prefix)}.safetensors")
    save_file({k: v.contiguous() for k, v in kohya.items()}, kp)
    save_file({k: v.contiguous() for k, v in peft.items()}, pp)
    return kp, pp, want


@pytest.mark.parametrize("alpha", [True, False])
@pytest.mark.parametrize("prefix", ["transformer.", ""])
def test_both_spellings_give_one_representation(tmp_path, alpha, prefix):
    kp, pp, want = _adapter_files(tmp_path, alpha, prefix)
    a, b = lora.read_adapter(kp, CFG), lora.read_adapter(pp, CFG)
    assert set(a.entries) == set(b.entries) == set(want)
    names2d = {n for n, s in param_shapes(CFG).items() if len(s) == 2}
    assert set(a.entries) <= names2d
    for n, (down, up, f) in want.items():
        for ad in (a, b):
            d, u, fac = ad.entries[n]
            assert d.dtype == u.dtype == torch.bfloat16
            assert torch.equal(d, down) and torch.equal(u, up), n
            assert fac == f, (n, fac, f)
    assert a.ranks == b.ranks == [4, 16]
    assert len(a.entries) == (8 + 2 * 3) + (2 + 4)   # double: 8 plain names + two fused of 3; single: 2 plain + linear1 of 4


def _one(tmp_path, tensors, name="bad.safetensors"):
    p = str(tmp_path / name)
    save_file({k: v.contiguous() for k, v in tensors.items()}, p)
    return p


def _good():
    g = torch.Generator().manual_seed(3)
    m = "transformer.transformer_blocks.0.attn.to_q"
    return {m + ".lora_A.weight": _rand(g, 4, D), m + ".lora_B.weight": _rand(g, D, 4)}


REFUSALS = {
    "unknown module": ({"transformer.transformer_blocks.0.attn.to_z.lora_A.weight": torch.zeros(4, D),
                        "transformer.transformer_blocks.0.attn.to_z.lora_B.weight": torch.zeros(D, 4)}, "attn.to_z"),
    "block that does not exist": ({"transformer.transformer_blocks.7.attn.to_q.lora_A.weight": torch.zeros(4, D),
                                   "transformer.transformer_blocks.7.attn.to_q.lora_B.weight": torch.zeros(D, 4)}, "transformer_blocks.7"),
    "wrong shape": ({"transformer.transformer_blocks.0.attn.to_q.lora_A.weight": torch.zeros(4, D + 8),
                     "transformer.transformer_blocks.0.attn.to_q.lora_B.weight": torch.zeros(D, 4)}, "to_q.lora_A.weight"),
    "wrong shape of up": ({"transformer.transformer_blocks.0.attn.to_q.lora_A.weight": torch.zeros(4, D),
                           "transformer.transformer_blocks.0.attn.to_q.lora_B.weight": torch.zeros(D + 8, 4)}, "to_q.lora_B.weight"),
    "different rank": ({"transformer.transformer_blocks.0.attn.to_q.lora_A.weight": torch.zeros(4, D),
                        "transformer.transformer_blocks.0.attn.to_q.lora_B.weight": torch.zeros(D, 8)}, "to_q.lora_B.weight"),
    "lora_B bias": ({**_good(), "transformer.transformer_blocks.0.attn.to_q.lora_B.bias": torch.zeros(D)}, "to_q.lora_B.bias"),
    "diff_b": ({**_good(), "transformer.transformer_blocks.0.attn.to_q.diff_b": torch.zeros(D)}, "to_q.diff_b"),
    "dora_scale": ({**_good(), "transformer.transformer_blocks.0.attn.to_q.dora_scale": torch.zeros(D)}, "to_q.dora_scale"),
    "lora_magnitude_vector": ({**_good(), "transformer.transformer_blocks.0.attn.to_q.lora_magnitude_vector": torch.zeros(D)},
                              "lora_magnitude_vector"),
    "text_encoder": ({**_good(), "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(4, 8),
                      "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_B.weight": torch.zeros(8, 4)}, "text_encoder.text_model"),
    "text_encoder_2": ({**_good(), "text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_A.weight": torch.zeros(4, 8),
                        "text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_B.weight": torch.zeros(8, 4)}, "text_encoder_2.encoder"),
    "lora_te": ({"lora_unet_double_blocks_0_img_attn_proj.lora_down.weight": torch.zeros(4, D),
                 "lora_unet_double_blocks_0_img_attn_proj.lora_up.weight": torch.zeros(D, 4),
                 "lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8),
                 "lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_up.weight": torch.zeros(8, 4)}, "lora_te1_text_model"),
    "kohya img_in": ({"lora_unet_img_in.lora_down.weight": torch.zeros(4, 64), "lora_unet_img_in.lora_up.weight": torch.zeros(D, 4)}, "lora_unet_img_in"),
    "kohya final_layer": ({"lora_unet_final_layer_linear.lora_down.weight": torch.zeros(4, D),
                           "lora_unet_final_layer_linear.lora_up.weight": torch.zeros(64, 4)}, "lora_unet_final_layer_linear"),
    "kohya time_in": ({"lora_unet_time_in_in_layer.lora_down.weight": torch.zeros(4, 256),
                       "lora_unet_time_in_in_layer.lora_up.weight": torch.zeros(D, 4)}, "lora_unet_time_in_in_layer"),
    "kohya fused of the wrong height": ({"lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight": torch.zeros(4, D),
                                         "lora_unet_double_blocks_0_img_attn_qkv.lora_up.weight": torch.zeros(D, 4)}, "img_attn_qkv.lora_up"),
    "half an entry": ({"transformer.transformer_blocks.0.attn.to_q.lora_A.weight": torch.zeros(4, D)}, "to_q.lora_A.weight"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_name_the_key(tmp_path, case):
    tensors, named = REFUSALS[case]
    with pytest.raises(ValueError) as e:
        lora.read_adapter(_one(tmp_path, tensors), CFG)
    assert named in str(e.value), str(e.value)


def test_good_file_reads(tmp_path):
    ad = lora.read_adapter(_one(tmp_path, _good(), "good.safetensors"), CFG)
    assert list(ad.entries) == ["transformer_blocks.0.attn.to_q.weight"] and ad.entries["transformer_blocks.0.attn.to_q.weight"][2] == 1.0


def test_merge_ref_is_the_formula():
    g = torch.Generator().manual_seed(5)
    N, K = 9, 16
    w0 = _rand(g, N, K)
    e1 = (_rand(g, 3, K), _rand(g, N, 3), 0.5)
    e2 = (_rand(g, 2, K), _rand(g, N, 2), torch.tensor([2.0, -0.25]))
    got = lora.merge_ref(w0, [e1, e2])
    assert got.dtype == torch.float64 and got.shape == (N, K)
    want = torch.zeros(N, K, dtype=torch.float64)
    scales = [[0.5] * 3, [2.0, -0.25]]
    for n in range(N):
        for k in range(K):
            acc = float(w0[n, k])
            for (down, up, _), sc in zip((e1, e2), scales):
                for r in range(down.shape[0]):
                    acc += sc[r] * float(up[n, r]) * float(down[r, k])
            want[n, k] = acc
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-15)
    assert torch.equal(lora.merge_ref(w0, []), w0.double())


def test_parse_lora_arg():
    assert lora.parse_lora_arg("a.safetensors") == ("a.safetensors", 1.0)
    assert lora.parse_lora_arg("a.safetensors:0.5") == ("a.safetensors", 0.5)
    assert lora.parse_lora_arg("dir:with:colons/a.safetensors") == ("dir:with:colons/a.safetensors", 1.0)
    assert lora.parse_lora_arg("x:notanumber") == ("x:notanumber", 1.0)
    assert lora.parse_lora_arg("dir:with:colons/a.safetensors:-2") == ("dir:with:colons/a.safetensors", -2.0)


@pytest.mark.parametrize("cfg", [CFG, FluxConfig(in_channels=64, num_layers=1, num_single_layers=1, num_attention_heads=2, joint_attention_dim=128,
                                                 pooled_projection_dim=64, guidance_embeds=False), FluxConfig.flux_dev(), FluxConfig.flux_fill()],
                         ids=["test-sized", "no-guidance", "flux-dev", "flux-fill"])
def test_linear_locations_cover_every_holder(cfg):
    shapes = param_shapes(cfg)
    loc = linear_locations(cfg)
    assert set(loc) == {n for n, s in shapes.items() if len(s) == 2}
    by_holder: dict = {}
    for n, (holder, row0, rows) in loc.items():
        assert rows == shapes[n][0], n
        by_holder.setdefault(holder, []).append((row0, rows, shapes[n][1]))
    Dm, Fm = cfg.dim, cfg.mlp_ratio * cfg.dim
    mod_rows = cfg.num_layers * 12 * Dm + cfg.num_single_layers * 3 * Dm + 2 * Dm
    for holder, ranges in by_holder.items():
        ranges.sort()
        assert len({k for _, _, k in ranges}) == 1, f"{holder}: Linears of different widths in one tensor"
        end = 0
        for row0, rows, _ in ranges:
            assert row0 == end, f"{holder}: rows {end}..{row0} are covered twice or not at all"
            end = row0 + rows
        total = {"mod_w": mod_rows, "wqkv": 3 * Dm, "cwqkv": 3 * Dm, "wqkvm": 3 * Dm + Fm}.get(holder[-1] if holder[0] != "mod_w" else "mod_w")
        if total is not None:
            assert end == total, f"{holder}: {end} rows covered of {total}"
    assert len([h for h in by_holder if h[0] == "double"]) == 8 * cfg.num_layers and len([h for h in by_holder if h[0] == "single"]) == 2 * cfg.num_single_layers


def test_abi_refusals_before_any_launch(built_lib):
    """every requirement of drag_lora_merge_bf16 is refused with a message and no launch (host memory stands in for the operands)"""
    buf = (ctypes.c_uint16 * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 8)
    sc = ctypes.c_void_p(base + 4096)
    f = built_lib.drag_lora_merge_bf16

    def refused(args, word):
        assert f(*args) != 0, word
        msg = built_lib.drag_last_error().decode()
        assert word in msg, (word, msg)

    #        w0 ldw0 w ldw  N  K   up ldup down lddown scale R stream
    ok = [p, 64, p, 64, 4, 64, p, 8, p, 64, sc, 4, None]

    def with_(**kw):
        names = ["w0", "ldw0", "w", "ldw", "N", "K", "up", "ldup", "down", "lddown", "scale", "R", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for name in ("w0", "w", "up", "down", "scale"):
        refused(with_(**{name: None}), "null")
    refused(with_(N=0), "N >= 1")
    refused(with_(R=0), "R >= 1")
    refused(with_(K=0), "multiple of 8")
    refused(with_(K=4, ldw=8, ldw0=8, lddown=8), "multiple of 8")
    refused(with_(K=60), "multiple of 8")
    for name in ("ldw", "ldw0", "lddown"):
        refused(with_(**{name: 56}), ">= K")
        refused(with_(**{name: 68}), "multiples of 8")
    refused(with_(ldup=0), "ldup")
    refused(with_(ldup=12), "ldup")
    refused(with_(R=9), "ldup")
    for name in ("w0", "w", "up", "down"):
        refused(with_(**{name: odd}), "16-byte aligned")
