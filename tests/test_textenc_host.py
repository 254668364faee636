"""Host-side pieces of the HIP prompt encoders (domain_rag_amd.textenc): relative-position buckets, the transformers-name mapping
of both encoders, the CLIP pooling rule, and the refusals that happen before any launch.  No GPU needed."""
import ctypes

import pytest
import torch


def test_t5_buckets_equal_upstream_for_every_offset():
    from transformers.models.t5.modeling_t5 import T5Attention
    from domain_rag_amd.textenc import t5_relative_buckets
    for S in (1, 16, 77, 300, 512):
        pos = torch.arange(S)
        rel = pos[None, :] - pos[:, None]                                   # memory - context, as compute_bias builds it
        want = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128)
        got = t5_relative_buckets(S)
        assert got.shape == (2 * S - 1,)
        assert torch.equal(got[rel + S - 1], want), f"S={S}"


def _tiny_t5():
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(0)
    return T5EncoderModel(T5Config(vocab_size=96, d_model=128, d_kv=64, d_ff=192, num_layers=2, num_heads=2,
                                   feed_forward_proj="gated-gelu")).eval()


def _tiny_clip(eos_token_id=2):
    from transformers import CLIPTextConfig, CLIPTextModel
    torch.manual_seed(1)
    return CLIPTextModel(CLIPTextConfig(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                                        max_position_embeddings=77, eos_token_id=eos_token_id)).eval()


def test_loaders_consume_every_saved_key(tmp_path):
    """save_pretrained -> safetensors -> from_pretrained: every key is mapped (an unmapped one raises), and the device tensors are the module's"""
    from domain_rag_amd.textenc import ClipTextHIP, T5EncoderHIP
    t5, clip = _tiny_t5(), _tiny_clip()
    t5.save_pretrained(tmp_path / "text_encoder_2", safe_serialization=True)
    clip.save_pretrained(tmp_path / "text_encoder", safe_serialization=True)
    a = T5EncoderHIP.from_pretrained(str(tmp_path / "text_encoder_2"), device="cpu")
    b = ClipTextHIP.from_pretrained(str(tmp_path / "text_encoder"), device="cpu")
    assert a.cfg.num_layers == 2 and a.cfg.num_heads == 2 and b.cfg.num_hidden_layers == 2 and b.cfg.eos_token_id == 2
    L = t5.encoder.block[1].layer
    assert torch.equal(a.layers[1]["wqkv"], torch.cat([L[0].SelfAttention.q.weight, L[0].SelfAttention.k.weight,
                                                       L[0].SelfAttention.v.weight]).bfloat16())
    assert torch.equal(a.layers[1]["wi"][192:], L[1].DenseReluDense.wi_1.weight.bfloat16())
    assert torch.equal(a.rel_bias, t5.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.bfloat16())
    tm = getattr(clip, "text_model", clip)                   # transformers 4.x nests the tower under text_model (the checkpoints' key prefix)
    assert torch.equal(b.layers[0]["bqkv"][128:256], tm.encoder.layers[0].self_attn.k_proj.bias.bfloat16())
    assert torch.equal(b.pos, tm.embeddings.position_embedding.weight.bfloat16())
    # from a live module: same tensors
    c = T5EncoderHIP.from_module(t5, device="cpu")
    assert all(torch.equal(x, y) for x, y in zip(a.parameters(), c.parameters()))


def test_loaders_name_missing_and_unexpected_keys():
    from domain_rag_amd.textenc import ClipTextConfig, ClipTextHIP, T5EncoderConfig, T5EncoderHIP
    t5 = _tiny_t5()
    cfg = T5EncoderConfig.from_dict(t5.config.to_dict())
    sd = dict(t5.state_dict())
    del sd["encoder.block.1.layer.1.DenseReluDense.wo.weight"]
    with pytest.raises(KeyError, match=r"encoder\.block\.1\.layer\.1\.DenseReluDense\.wo\.weight"):
        T5EncoderHIP(cfg, sd, device="cpu")
    sd = dict(t5.state_dict())
    del sd["shared.weight"]                                      # either alias of the tied embedding is enough
    T5EncoderHIP(cfg, sd, device="cpu")
    sd["decoder.block.0.layer.0.layer_norm.weight"] = torch.ones(128)
    with pytest.raises(KeyError, match="unexpected"):
        T5EncoderHIP(cfg, sd, device="cpu")
    clip = _tiny_clip()
    ccfg = ClipTextConfig.from_dict(clip.config.to_dict())
    sd = {k.replace("text_model.", ""): v for k, v in clip.state_dict().items()}
    ClipTextHIP(ccfg, sd, device="cpu")
    ClipTextHIP(ccfg, {"text_model." + k: v for k, v in sd.items()}, device="cpu")      # the checkpoints' prefixed names as well
    del sd["final_layer_norm.bias"]
    with pytest.raises(KeyError, match=r"final_layer_norm\.bias"):
        ClipTextHIP(ccfg, sd, device="cpu")


def test_pool_index_matches_upstream_pooling():
    from domain_rag_amd.textenc import clip_pool_index
    rows = torch.tensor([[94, 5, 7, 95, 95, 95], [94, 95, 3, 3, 3, 3], [94, 8, 9, 10, 11, 95], [94, 9, 9, 9, 9, 9]])
    for eos in (2, 95, 9):
        clip = _tiny_clip(eos)
        with torch.no_grad():
            out = clip(rows)
        idx = clip_pool_index(rows, eos)
        assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(4), idx]), f"eos_token_id={eos}"


def test_unsupported_configs_are_refused():
    from domain_rag_amd.textenc import ClipTextConfig, T5EncoderConfig
    for bad, what in ((dict(d_kv=128), "head_dim"), (dict(feed_forward_proj="relu"), "feed_forward_proj"),
                      (dict(feed_forward_proj="gated-silu"), "feed_forward_proj"), (dict(is_decoder=True), "decoder")):
        with pytest.raises(NotImplementedError, match=what):
            T5EncoderConfig.from_dict(dict(d_model=512, num_heads=8, **bad))
    with pytest.raises(NotImplementedError, match="head_dim"):
        ClipTextConfig.from_dict(dict(hidden_size=768, num_attention_heads=8))
    with pytest.raises(NotImplementedError, match="hidden_act"):
        ClipTextConfig.from_dict(dict(hidden_act="gelu"))
    assert ClipTextConfig.from_dict({"text_config": {"hidden_size": 1024, "num_attention_heads": 16}}).hidden_size == 1024


def test_bad_ids_are_refused_before_any_launch():
    from domain_rag_amd.textenc import T5EncoderHIP
    enc = T5EncoderHIP.from_module(_tiny_t5(), device="cpu")
    with pytest.raises(ValueError, match="token id"):
        enc(torch.tensor([[1, 2, 96]]))
    with pytest.raises(ValueError, match="S <= 512"):
        enc(torch.zeros(1, 513, dtype=torch.long))


def test_abi_refuses_bad_arguments(built_lib):
    buf = (ctypes.c_uint16 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    att = built_lib.drag_textenc_attention_bf16
    assert att(None, p, p, p, 1, 8, 1, 192, 8 * 192, 64, 512, 1.0, None, 0, 1, None) != 0 and b"null" in built_lib.drag_last_error()
    assert att(p, p, p, p, 1, 513, 1, 192, 513 * 192, 64, 513 * 64, 1.0, None, 0, 1, None) != 0 and b"S must be" in built_lib.drag_last_error()
    assert att(p, p, p, p, 1, 8, 4, 192, 8 * 192, 256, 8 * 256, 1.0, None, 0, 1, None) != 0 and b"ld >= 64 H" in built_lib.drag_last_error()
    assert att(p, p, p, p, 1, 8, 1, 196, 8 * 196, 64, 512, 1.0, None, 0, 1, None) != 0 and b"ld % 8" in built_lib.drag_last_error()
    rms = built_lib.drag_t5_rmsnorm_bf16
    assert rms(p, p, p, 4, 4104, 1e-6, None) != 0 and b"D <= 4096" in built_lib.drag_last_error()
    assert rms(p, p, p, 4, 100, 1e-6, None) != 0 and b"D % 8" in built_lib.drag_last_error()
    assert built_lib.drag_gated_new_gelu_bf16(p, p, 4, 12, None) != 0 and b"F % 8" in built_lib.drag_last_error()
    assert built_lib.drag_quick_gelu_bf16(p, p, 12, None) != 0 and b"n % 8" in built_lib.drag_last_error()
    assert built_lib.drag_embed_gather_bf16(None, p, None, p, 4, 4, 64, 10, None) != 0 and b"null" in built_lib.drag_last_error()


def test_abi_accepts_calls_with_nothing_to_do(built_lib):
    """an empty torch tensor has no address (data_ptr() is 0): a call over no rows is accepted before any pointer is looked at, so
    ops.t5_rmsnorm / gated_new_gelu / quick_gelu / embed_gather take empty tensors; a bad width is refused all the same"""
    buf = (ctypes.c_uint16 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert built_lib.drag_t5_rmsnorm_bf16(None, p, None, 0, 768, 1e-6, None) == 0
    assert built_lib.drag_gated_new_gelu_bf16(None, None, 0, 64, None) == 0
    assert built_lib.drag_quick_gelu_bf16(None, None, 0, None) == 0
    assert built_lib.drag_embed_gather_bf16(None, p, None, None, 0, 4, 64, 10, None) == 0
    assert built_lib.drag_t5_rmsnorm_bf16(None, p, None, 0, 4104, 1e-6, None) != 0 and b"D <= 4096" in built_lib.drag_last_error()
    assert built_lib.drag_gated_new_gelu_bf16(None, None, 0, 12, None) != 0 and b"F % 8" in built_lib.drag_last_error()
    assert built_lib.drag_t5_rmsnorm_bf16(None, p, None, 4, 768, 1e-6, None) != 0 and b"null" in built_lib.drag_last_error()
