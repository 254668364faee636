"""drag_lora_merge_bf16 on the GPU against ``lora.merge_ref`` (float64, rounded once to bf16) under ``tests/helpers/bf16_bar.bar``:
at least 99 % of the elements equal, the rest within 1 ulp or 2^-8 of the largest output.  A float32 evaluation of the rule meets that
bar with a wide margin on every shape here (three summation orders tried on the host: >= 99.99 % equal for W ~ N(0, 0.02^2) and factors
of std 0.02-0.1); the kernel's scaled factors carry 16 mantissa bits, which moves an element by at most 2^-17 of the delta.

Every operand is a view inside a sentinel-filled buffer with at least 256 guard elements either side: ldw > K with gap columns that must
keep their sentinel, ldup > R with NaN in the padding columns, per-column scales that differ (two adapters concatenated)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.bf16_bar import bar  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 1), (17, 8, 1), (200, 264, 4), (333, 520, 24), (256, 1024, 64), (256, 1024, 128), (130, 72, 200)]
GUARD = 256
SENT = 768.0          # exactly representable in bf16; no weight, factor or merged value comes near it


def _framed(rows: int, cols: int, ld: int, fill: float, dev):
    """(buffer, view): ``view`` [rows, cols] with row stride ``ld`` inside a flat bf16 buffer filled with ``fill``, GUARD elements either
    side (the front guard keeps the view 16-byte aligned)"""
    buf = torch.full((GUARD + rows * ld + GUARD,), fill, dtype=torch.bfloat16, device=dev)
    return buf, buf[GUARD: GUARD + rows * ld].view(rows, ld)[:, :cols]


def _case(N, K, R, dev, seed=0, w_std=0.02):
    g = torch.Generator().manual_seed(1000 * seed + N + K + R)
    w0 = (w_std * torch.randn(N, K, generator=g)).bfloat16()
    up = (0.05 * torch.randn(N, R, generator=g)).bfloat16()
    down = (0.05 * torch.randn(R, K, generator=g)).bfloat16()
    # two adapters' worth of columns: different factors either side of the middle, all exact in float32
    scale = torch.where(torch.arange(R) < (R + 1) // 2, torch.tensor(0.75), torch.tensor(-1.625)).float()
    ldw, ldup, lddown = K + 24, (R + 7) // 8 * 8 + 8, K + 8
    d = dict(N=N, K=K, R=R, w0=w0, up=up, down=down, scale=scale)
    d["w0_buf"], d["w0_v"] = _framed(N, K, ldw, SENT, dev)
    d["w_buf"], d["w_v"] = _framed(N, K, ldw, SENT, dev)
    d["up_buf"], d["up_v"] = _framed(N, R, ldup, float("nan"), dev)
    d["down_buf"], d["down_v"] = _framed(R, K, lddown, SENT, dev)
    d["w0_v"].copy_(w0); d["up_v"].copy_(up); d["down_v"].copy_(down)
    d["scale_d"] = scale.to(dev)
    return d


def _want(d):
    from domain_rag_amd import lora
    return lora.merge_ref(d["w0"], [(d["down"], d["up"], d["scale"])]).to(torch.bfloat16)


def _gaps_keep_sentinel(buf, rows, cols, ld, what, nan=False):
    """everything of ``buf`` outside the framed view still holds its fill value"""
    b = buf.cpu().float()
    body = b[GUARD: GUARD + rows * ld].view(rows, ld)
    outside = torch.cat([b[:GUARD], b[GUARD + rows * ld:], body[:, cols:].reshape(-1)])
    ok = torch.isnan(outside) if nan else outside == SENT
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements outside the view changed"


@pytest.mark.parametrize("N,K,R", SHAPES)
def test_merge_matches_the_rule(gpu, N, K, R):
    from domain_rag_amd import ops
    d = _case(N, K, R, gpu)
    want = _want(d)
    w0_before = d["w0_buf"].clone()
    out = ops.lora_merge(d["w0_v"], d["w_v"], d["up_v"], d["down_v"], d["scale_d"])
    torch.cuda.synchronize()
    assert out.data_ptr() == d["w_v"].data_ptr()
    got = d["w_v"].cpu()
    assert bool(torch.isfinite(got.float()).all()), "NaN padding of up reached the output"
    eq = bar(got, want, f"lora_merge {N}x{K} R={R}")
    moved = (want.float() - d["w0"].float()).abs().max().item()
    print(f"lora_merge N={N} K={K} R={R}: {eq:.4%} equal, largest move {moved:.3e}")
    assert moved > 0, "the case does not move the weight"
    # out of place leaves w0 (and every gap and guard of every operand) as it was
    assert torch.equal(d["w0_buf"], w0_before), "the out-of-place form wrote to w0"
    ldw = K + 24
    _gaps_keep_sentinel(d["w_buf"], N, K, ldw, "w")
    _gaps_keep_sentinel(d["up_buf"], N, R, (R + 7) // 8 * 8 + 8, "up", nan=True)
    _gaps_keep_sentinel(d["down_buf"], R, K, K + 8, "down")
    # in place gives the same bits
    ops.lora_merge(d["w0_v"], d["w0_v"], d["up_v"], d["down_v"], d["scale_d"])
    torch.cuda.synchronize()
    assert torch.equal(d["w0_v"].cpu(), got), "in place and out of place differ"
    _gaps_keep_sentinel(d["w0_buf"], N, K, ldw, "w0 (in place)")


def test_merge_into_a_row_slice_leaves_the_other_rows(gpu):
    """rows [D, 2D) of a stacked [3D, K] weight (to_k inside wqkv): the other rows keep their bits"""
    from domain_rag_amd import lora, ops
    D, K, R = 136, 264, 16
    g = torch.Generator().manual_seed(7)
    stacked = (0.02 * torch.randn(3 * D, K, generator=g)).bfloat16()
    up = (0.05 * torch.randn(D, R, generator=g)).bfloat16()
    down = (0.05 * torch.randn(R, K, generator=g)).bfloat16()
    scale = torch.full((R,), 0.5)
    w = stacked.to(gpu)
    pristine = w.clone()
    ops.lora_merge(pristine[D: 2 * D], w[D: 2 * D], up.to(gpu), down.to(gpu), scale.to(gpu))
    torch.cuda.synchronize()
    got = w.cpu()
    assert torch.equal(got[:D], stacked[:D]) and torch.equal(got[2 * D:], stacked[2 * D:])
    bar(got[D: 2 * D], lora.merge_ref(stacked[D: 2 * D], [(down, up, 0.5)]).to(torch.bfloat16), "row slice")
    assert not torch.equal(got[D: 2 * D], stacked[D: 2 * D])


def test_zero_scale_returns_w0_bits(gpu):
    from domain_rag_amd import ops
    d = _case(200, 264, 4, gpu, seed=3)
    w0 = d["w0"].clone()
    w0[w0 == 0] = 0.0                                     # no -0.0: (-0) + (+0) is +0 in float32
    d["w0_v"].copy_(w0)
    ops.lora_merge(d["w0_v"], d["w_v"], d["up_v"], d["down_v"], torch.zeros(4, device=gpu))
    torch.cuda.synchronize()
    assert torch.equal(d["w_v"].cpu().view(torch.int16), w0.view(torch.int16))


def test_huge_weights_absorb_a_small_delta(gpu):
    from domain_rag_amd import ops
    d = _case(130, 72, 24, gpu, seed=5)
    w0 = torch.where(d["w0"].float() >= 0, torch.tensor(1e30), torch.tensor(-1e30)).bfloat16()
    d["w0_v"].copy_(w0)
    ops.lora_merge(d["w0_v"], d["w_v"], d["up_v"], d["down_v"], d["scale_d"])
    torch.cuda.synchronize()
    assert torch.equal(d["w_v"].cpu().view(torch.int16), w0.view(torch.int16))


def test_wrapper_refusals(gpu):
    from domain_rag_amd import ops
    bf = dict(dtype=torch.bfloat16, device=gpu)
    w = torch.zeros(32, 64, **bf)
    up, down, sc = torch.zeros(32, 8, **bf), torch.zeros(8, 64, **bf), torch.ones(8, device=gpu)
    with pytest.raises(ValueError, match="overlap"):
        ops.lora_merge(w[:16], w[8:24], up[:16], down, sc)
    with pytest.raises(ValueError, match="do not fit"):
        ops.lora_merge(w, w, up[:16], down, sc)
    with pytest.raises(TypeError):
        ops.lora_merge(w.float(), w, up, down, sc)
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.lora_merge(w, w.t().contiguous().t(), up, down, sc)
    with pytest.raises(ValueError, match="R = 8 factors"):
        ops.lora_merge(w, w, up, down, sc[:4])
    with pytest.raises(RuntimeError, match="K a positive multiple of 8"):
        ops.lora_merge(torch.zeros(32, 12, **bf), torch.zeros(32, 12, **bf), up, torch.zeros(8, 12, **bf), sc)
