"""The host side of the MXFP8 attention mode (no GPU, no library): ``mx.attention_ref`` on a case checked by hand, its distance from exact
attention pinned to the figure recorded when the rule was written, and the address arithmetic of the new ``ops._attention_reach`` kinds
against addresses enumerated by brute force."""
import itertools
import math

import pytest
import torch


def _rms_rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def test_attention_ref_on_two_keys_by_hand():
    """S = 2, scale = 1.  q0 = 2 e0, k0 = e0, k1 = 0: row 0 scores (2, 0), p = (1, e^-2 = 0.135335); p 256 = (256, 34.6458) and e4m3 holds
    32 and 36 around the second (step 4 in [32, 64)), so P^ = (1, 36 / 256 = 0.140625): out0 = (v0 + 0.140625 v1) / 1.135335 — the sum of the
    UNROUNDED p.  q1 = 0: row 1 scores (0, 0), P^ = (1, 1), out1 = (v0 + v1) / 2.  v0 = 1 and v1 cycling through 0.5 .. 8 survive the V^T
    quantisation exactly (block amax 8: shared exponent -5, every value times 32 is an e4m3 value)."""
    from domain_rag_amd import mx
    q = torch.zeros(2, 128); k = torch.zeros(2, 128)
    q[0, 0], k[0, 0] = 2.0, 1.0
    v1 = torch.tensor([0.5, 1, 1.5, 2, 3, 4, 6, 8]).repeat(16)
    v = torch.stack([torch.ones(128), v1])
    out = mx.attention_ref(q.bfloat16(), k.bfloat16(), v.bfloat16(), 1.0)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (2, 128)
    want0 = (1.0 + 0.140625 * v1.double()) / (1.0 + math.exp(-2.0))
    want1 = (1.0 + v1.double()) / 2
    assert torch.equal(out[0], want0.float().bfloat16())
    assert torch.equal(out[1], want1.float().bfloat16())
    # the two rules a later "fix" would most likely change, each visible in this case: the unrounded p (0.135335) as the operand, or the
    # rounded P^ in the row sum
    assert not torch.equal(out[0], ((1.0 + math.exp(-2.0) * v1.double()) / (1.0 + math.exp(-2.0))).float().bfloat16())
    assert not torch.equal(out[0], ((1.0 + 0.140625 * v1.double()) / 1.140625).float().bfloat16())
    with pytest.raises(ValueError):
        mx.attention_ref(q, k, v, 1.0)                    # float32: the inputs are prepared bf16


def test_attention_ref_distance_is_the_recorded_one():
    """seeded N(0, 1), S = 512: rms-relative distance from float64 attention on the unquantised inputs within +-20 % of the 5.2e-2 measured
    when the restatement was written, and above a bf16 flash evaluation's (bf16 P, float32 sums: 2.2e-3 then)"""
    from domain_rag_amd import mx
    g = torch.Generator().manual_seed(1)
    S, scale = 512, 1 / math.sqrt(128)
    q, k, v = (torch.randn(S, 128, generator=g).bfloat16() for _ in range(3))
    s = (q.double() @ k.double().t()) * scale
    exact = torch.softmax(s, dim=1) @ v.double()
    d_ref = _rms_rel(mx.attention_ref(q, k, v, scale), exact)
    p = torch.exp(s - s.amax(dim=1, keepdim=True)).float()
    bf16_eval = ((p.bfloat16().float() @ v.float()) / p.sum(dim=1, keepdim=True)).bfloat16()
    d_bf16 = _rms_rel(bf16_eval, exact)
    print(f"mx.attention_ref vs float64: {d_ref:.4e}; bf16 evaluation vs float64: {d_bf16:.4e}")
    assert 0.8 * 5.2e-2 <= d_ref <= 1.2 * 5.2e-2
    assert d_ref > d_bf16


def _reach(*a, **kw):
    from domain_rag_amd import ops
    return ops._attention_reach(*a, **kw)


@pytest.mark.parametrize("S,s_pad", [(1, 128), (17, 128), (127, 128), (128, 128), (129, 256), (333, 384)])
def test_mx_image_reach_rounds_s_up_to_128(S, s_pad):
    """the six dense images: every byte of every row is written, the padding included; (batch b, head h) at (b H + h) * the image of one head"""
    for B, H in itertools.product((1, 2, 3), (1, 2)):
        rows = max(((b * H + h) * s_pad + s) * 128 + d for b in range(B) for h in range(H) for s in (0, s_pad - 1) for d in (0, 127))
        assert _reach("mx_rows", B, S, H) == rows + 1 == B * H * s_pad * 128
        row_scales = max(((b * H + h) * s_pad + s) * 4 + j for b in range(B) for h in range(H) for s in (0, s_pad - 1) for j in (0, 3))
        assert _reach("mx_row_scales", B, S, H) == row_scales + 1
        vt = max(((b * H + h) * 128 + d) * s_pad + pos for b in range(B) for h in range(H) for d in (0, 127) for pos in (0, s_pad - 1))
        assert _reach("mx_vt", B, S, H) == vt + 1
        vt_scales = max(((b * H + h) * 128 + d) * (s_pad // 32) + j for b in range(B) for h in range(H) for d in (0, 127) for j in (0, s_pad // 32 - 1))
        assert _reach("mx_vt_scales", B, S, H) == vt_scales + 1


def test_mx_images_are_refused_on_the_host_and_counted():
    """``ops._attention_room`` looks at the images' device and type before their size: host tensors and a wrong count are refused"""
    from domain_rag_amd import ops
    imgs = tuple(torch.zeros(4, dtype=torch.uint8) for _ in range(6))
    with pytest.raises(ValueError, match="expected a GPU uint8"):
        ops._attention_room("t", 1, 1, 1, mx=imgs)
    with pytest.raises(ValueError, match="six MXFP8 images"):
        ops._attention_room("t", 1, 1, 1, mx=imgs[:5])
