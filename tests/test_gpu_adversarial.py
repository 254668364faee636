"""Adversarial input distributions for every kernel that had only ever seen N(0, 1).

Round 4's three worst findings (the 64-query attention kernel's row maximum over half the keys, GroupNorm's cancelling sums, the top-k
select's slow path) all came from leaving the comfortable distribution, and nothing but this repo's own oracle checks the generation core.
The value ranges here are the ones FluxTransformer2DModel really sees under batch_generate_flux_kshot.py:467-474 /
outpainting_updown_sampling_redux.py:1246-1257 — hidden states with outlier channels 10^2-10^3 x the median, heavy-tailed weights,
softmax rows owned by one logit — plus the representable extremes (bf16 subnormals, +-max bf16, row norms from 1e-20 to 1e18).

Yardsticks and bars (written where they are used):
  * bf16 GEMM / conv families: float64 over the SAME bf16 operands.  A bf16-in / f32-accumulate / bf16-out product may differ from it by
    the output rounding (2^-8 relative = half an ulp of bf16's 8-bit significand; the gate epilogue rounds three times and gets three
    of them) plus the float32 accumulation error, which is relative to S = sum_k |a_k w_k|, not to the result — BAR_ACC x S with BAR_ACC = 1e-5 (K <= 4096 terms,
    blockwise: measured <= 3e-7).  A kernel that drops an outlier channel, saturates, or sums in bf16 fails by orders of magnitude.
  * softmax / norms / f32 attention: float64 of the same inputs, elementwise, with the output type's rounding as the bar.
  * blocks and the 30-step chain on Student-t (nu = 3) weights: the bf16 oracle's own distance from the float32 oracle x 1.3 (the bar of
    tests/test_gpu_fullsize.py), rms x 1.1 / max x 1.4 per step for the chain (the bars of tests/test_gpu_chained_steps.py).
Every bug this file found is listed in DESIGN.md ("Round 5")."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR_OUT = 2.0 ** -8
BAR_ACC = 1e-5
BF16_MAX = 3.3895313892515355e38
BF16_MIN_NORMAL = 2.0 ** -126


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.to(torch.bfloat16)


def _student_t(shape, nu, gen):
    """Student-t with nu degrees of freedom and unit variance (nu > 2): z / sqrt(chi2_nu / nu) * sqrt((nu - 2) / nu)"""
    z = torch.randn(shape, generator=gen)
    chi = torch.zeros(shape)
    for _ in range(nu):
        chi += torch.randn(shape, generator=gen) ** 2
    return z / (chi / nu).sqrt() * math.sqrt((nu - 2) / nu)


def _gemm_check(out, a, w, *, bias=None, what=""):
    """out against float64 over the same bf16 operands: |out - ref| <= BAR_OUT |ref| + BAR_ACC sum|a||w| (+ one bf16 subnormal step)"""
    a64, w64 = a.double(), w.double()
    ref = a64 @ w64.T
    mag = a64.abs() @ w64.abs().T
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    err = (out.double().cpu() - ref).abs()
    bound = 1.001 * BAR_OUT * ref.abs() + BAR_ACC * mag + 1e-40
    bad = err > bound
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite outputs"
    flat = int((err / bound).argmax())
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} outputs beyond the bar; worst err/bound {(err / bound).max().item():.2f} at "
                           f"(row {flat // err.shape[1]}, column {flat % err.shape[1]}); max err/S {(err / (mag + 1e-300)).max().item():.2e}")
    return (err / (mag + 1e-300)).max().item()


# kernel families by the rows of the launch (policy of csrc/gemm_bf16.hip): t256 persistent, t128, the ring kernels
FAMILIES = [("t256", 2304), ("t128_or_ring", 640), ("ring_small_m", 40)]


def _outlier_operands(M, N, K, seed, factor, frac=1e-3):
    """A ~ N(0, 1) with `frac` of its K channels scaled by `factor` (the massive-activation channels of a DiT's hidden states);
    W ~ N(0, 0.02) with `frac` of its rows' entries scaled by 100 (heavy-tailed weights)"""
    g = _g(seed)
    a = torch.randn(M, K, generator=g)
    nch = max(1, int(round(K * frac)))
    ch = torch.randperm(K, generator=g)[:nch]
    a[:, ch] *= factor
    w = torch.randn(N, K, generator=g) * 0.02
    idx = torch.randint(0, N * K, (max(1, int(N * K * frac)),), generator=g)
    w.view(-1)[idx] *= 100.0
    return _bf(a), _bf(w), ch


@pytest.mark.parametrize("factor", [1e2, 1e3])
@pytest.mark.parametrize("family,M", FAMILIES)
def test_gemm_outlier_channels(gpu, family, M, factor):
    from domain_rag_amd import ops
    N, K = 768, 3072
    a, w, ch = _outlier_operands(M, N, K, 7 + M, factor)
    bias = _bf(torch.randn(N, generator=_g(3)))
    out = ops.gemm(a.to(gpu), w.to(gpu), bias=bias.to(gpu))
    _gemm_check(out, a, w, bias=bias, what=f"{family} outliers x{factor:g}")
    # the outlier channels carry the result: zeroing them must change it (guards the test itself)
    a0 = a.clone(); a0[:, ch] = 0
    assert ((a.double() @ w.double().T) - (a0.double() @ w.double().T)).abs().max() > 10


@pytest.mark.parametrize("family,M", FAMILIES)
def test_gemm_cancelling_rows(gpu, family, M):
    """every output is the difference of two large, nearly equal sums: a = [u, -u], w = [v, v + d] with |d| ~ 2^-7 |v|.  Products of bf16
    pairs are exact in float32, so the result lives or dies with the accumulation: the bar is relative to sum |a w| (~1e3 x the result)"""
    from domain_rag_amd import ops
    N, K = 512, 2048
    g = _g(M)
    u = _bf(torch.randn(M, K // 2, generator=g) * 8)
    v = _bf(torch.randn(N, K // 2, generator=g))
    d = _bf(v.float() * (2.0 ** -7) * torch.sign(torch.randn(N, K // 2, generator=g)))
    a = torch.cat([u, -u], 1).contiguous()
    w = torch.cat([v, _bf(v.float() + d.float())], 1).contiguous()
    out = ops.gemm(a.to(gpu), w.to(gpu))
    ref = a.double() @ w.double().T
    mag = a.double().abs() @ w.double().abs().T
    assert (mag / ref.abs().clamp_min(1e-30)).median() > 50          # really cancelling
    _gemm_check(out, a, w, what=f"{family} cancelling")


@pytest.mark.parametrize("family,M", FAMILIES)
def test_gemm_subnormal_and_max_bf16_operands(gpu, family, M):
    """bf16 subnormal inputs (|x| < 2^-126) against large weights, and +-max bf16 against tiny ones: products are ordinary float32 numbers and
    torch's bf16 matmul (CPU and CUDA alike) keeps them — a matrix core that flushed subnormal INPUTS would return zeros here"""
    from domain_rag_amd import ops
    N, K = 256, 512
    g = _g(M + 1)
    # (1) subnormal activations x 2^100-scale weights: results ~ 2^-30 * sqrt(K)
    a = _bf(torch.randn(M, K, generator=g) * (2.0 ** -129))
    assert (a.float().abs() < BF16_MIN_NORMAL).float().mean() > 0.9 and (a.float() != 0).float().mean() > 0.5
    w = _bf(torch.randn(N, K, generator=g) * (2.0 ** 100))
    out = ops.gemm(a.to(gpu), w.to(gpu))
    ref = a.double() @ w.double().T
    assert ref.abs().median() > 2.0 ** -34
    _gemm_check(out, a, w, what=f"{family} subnormal activations")
    # (2) +-max bf16 activations x 2^-110-scale weights
    sign = torch.sign(torch.randn(M, K, generator=g))
    a2 = _bf(sign * BF16_MAX)
    w2 = _bf(torch.randn(N, K, generator=g) * (2.0 ** -110))
    out2 = ops.gemm(a2.to(gpu), w2.to(gpu))
    _gemm_check(out2, a2, w2, what=f"{family} max-bf16 activations")
    # (3) subnormal OUTPUTS: tiny x tiny products sum to float32 subnormals, the bf16 rounding of which torch keeps as well
    a3 = _bf(torch.randn(M, K, generator=g) * (2.0 ** -70))
    w3 = _bf(torch.randn(N, K, generator=g) * (2.0 ** -64))
    out3 = ops.gemm(a3.to(gpu), w3.to(gpu)).cpu()
    ref3 = _bf((a3.float() @ w3.float().T))           # torch's own float32 route: same subnormal handling on the host
    lim = 2.0 ** -133                                   # one bf16 subnormal step
    assert (out3.double() - ref3.double()).abs().max() <= 2 * lim + BAR_OUT * ref3.double().abs().max()


def test_gemm_gate_residual_epilogue_with_outliers(gpu):
    """x + gate * (a w^T + b) on the DiT's row map (two batches inside one buffer) with outlier channels in a AND a residual stream that
    carries massive activations itself: torch's order is round(y), round(gate * y), round(x + .) — checked against float64 with the three
    bf16 roundings as the bar"""
    from domain_rag_amd import ops
    B, S, N, K = 2, 1280, 1024, 3072
    M = B * S
    a, w, _ = _outlier_operands(M, N, K, 5, 1e3)
    g = _g(9)
    bias = _bf(torch.randn(N, generator=g))
    gate = _bf(torch.randn(B, N, generator=g) * 0.5)
    resid = torch.randn(M, N, generator=g)
    resid[:, ::257] *= 500.0
    resid = _bf(resid)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=gpu)
    ops.gemm(a.to(gpu), w.to(gpu), out, bias=bias.to(gpu), gate=gate.to(gpu), resid=resid.to(gpu), c_rows_per_batch=S, c_batch_stride=S * N,
             ldg=N)
    y = a.double() @ w.double().T + bias.double()
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()
    gy = gate.double().repeat_interleave(S, 0) * y
    ref = resid.double() + gy
    err = (out.double().cpu() - ref).abs()
    # three roundings: y (its error scaled by |gate|), gate * y, the sum — 2^-8 (|ref| + 2 |gate y|), 2 % of slack for second-order terms
    bound = 1.02 * BAR_OUT * (ref.abs() + 2 * gy.abs()) + 2 * BAR_ACC * mag
    assert torch.isfinite(out.float()).all().item() and not (err > bound).any(), (err / bound).max().item()


def test_conv3x3_outlier_channels_and_cancelling_taps(gpu):
    """the VAE's 3x3 convolutions (implicit GEMM over 9 taps): outlier input channels, and a Laplacian-like kernel on a smooth bright image
    whose nine taps cancel to ~1e-3 of their magnitude sum"""
    from domain_rag_amd import ops
    B, H, W, Ci, Co = 1, 48, 48, 128, 256
    g = _g(1)
    x = torch.randn(B, Ci, H, W, generator=g)
    x[:, 5] *= 1e3
    x[:, 77] *= 1e2
    wt = torch.randn(Co, Ci, 3, 3, generator=g) * 0.05
    for name, xx, ww in (("outliers", x, wt), ("cancelling",
                                               100.0 + 0.01 * torch.randn(B, Ci, H, W, generator=g),
                                               (torch.tensor([[1., 1, 1], [1, -8, 1], [1, 1, 1]])[None, None] * (1 + 0.0 * wt)) * torch.randn(Co, Ci, 1, 1, generator=g) * 0.05)):
        xb, wb = _bf(xx), _bf(ww)
        xp = torch.zeros((B, H + 2, W + 2, Ci), dtype=torch.bfloat16)
        xp[:, 1:-1, 1:-1] = xb.permute(0, 2, 3, 1)
        y = torch.empty((B, H, W, Co), dtype=torch.bfloat16, device=gpu)
        ops.conv3x3(xp.to(gpu), wb.permute(0, 2, 3, 1).contiguous().to(gpu), y, B=B, Ho=H, Wo=W, Hp=H + 2, Wp=W + 2, Cin=Ci, Cout=Co)
        ref = torch.nn.functional.conv2d(xb.double(), wb.double(), padding=1)
        mag = torch.nn.functional.conv2d(xb.double().abs(), wb.double().abs(), padding=1)
        err = (y.double().cpu().permute(0, 3, 1, 2) - ref).abs()
        bound = BAR_OUT * ref.abs() + BAR_ACC * mag
        assert not (err > bound).any(), f"conv3x3 {name}: worst err/bound {(err / bound).max().item():.2f}"
        if name == "cancelling":
            assert (mag[:, :, 2:-2, 2:-2] / ref[:, :, 2:-2, 2:-2].abs().clamp_min(1e-30)).median() > 100


def test_gemm_pair_and_two_destinations_with_outliers(gpu):
    """the merged launches of the DiT (text + image rows as one launch; q|k|v and proj_mlp as one launch into two buffers) on outlier operands"""
    from domain_rag_amd import ops
    N, K = 768, 3072
    a1, w1, _ = _outlier_operands(1024, N, K, 31, 1e3)
    a2, w2, _ = _outlier_operands(512, N, K, 32, 1e2)
    o1 = torch.empty(1024, N, dtype=torch.bfloat16, device=gpu); o2 = torch.empty(512, N, dtype=torch.bfloat16, device=gpu)
    with ops.options(gemm_pair=2):
        ops.gemm_pair(dict(a=a1.to(gpu), w=w1.to(gpu), out=o1), dict(a=a2.to(gpu), w=w2.to(gpu), out=o2))
    _gemm_check(o1, a1, w1, what="pair, first segment")
    _gemm_check(o2, a2, w2, what="pair, second segment")
    a3, w3, _ = _outlier_operands(2500, 1024, 1024, 33, 1e3)
    oa = torch.empty(2500, 512, dtype=torch.bfloat16, device=gpu); ob = torch.empty(2500, 512, dtype=torch.bfloat16, device=gpu)
    ops.gemm(a3.to(gpu), w3.to(gpu), oa, out2=ob, ldc2=512, n_split=512)
    _gemm_check(torch.cat([oa, ob], 1), a3, w3, what="two destinations")


# ------------------------------------------------------------------ gemm_bf16_w4p: the kernel that runs two thirds of a composite batch
#  — the families above pick their kernel by launch shape and the policy sends none of those shapes to the 4-wave
# kernel (>= 768 tiles, or >= 256 with K >= 8192), whose evidence was bit-equality with the 8-wave kernel on N(0, 1) operands.  Here it is
# checked against float64 directly: FORCED ("gemm_kernel" = 3) on shapes small enough for a host float64 product, and through the POLICY on
# shapes it really takes (the float64 product then on the GPU, by torch — the checker, not the product).
def _forced_w4p():
    from domain_rag_amd import ops
    return ops.options(gemm_kernel=3)


def _gemm_check_gpu(out, a, w, *, bias=None, what="", extra_roundings=0):
    """_gemm_check with the float64 yardstick computed on the device (operands already there)"""
    a64, w64 = a.double(), w.double()
    ref = a64 @ w64.T
    mag = a64.abs() @ w64.abs().T
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    err = (out.double() - ref).abs()
    bound = (1.001 + extra_roundings) * BAR_OUT * ref.abs() + BAR_ACC * mag + 1e-40
    assert torch.isfinite(out.float()).all().item(), f"{what}: non-finite outputs"
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, f"{what}: worst err/bound {ratio:.2f}; max err/S {(err / (mag + 1e-300)).max().item():.2e}"
    return (err / (mag + 1e-300)).max().item()


def _is_w4p(M, N, K):
    from domain_rag_amd import _lib
    return _lib.load().drag_gemm_bf16_choice(M, 0, N, K) == 3


@pytest.mark.parametrize("factor", [1e2, 1e3])
@pytest.mark.parametrize("M", [2304, 2400])
def test_gemm_w4p_forced_outlier_channels(gpu, M, factor):
    """27 | 30 tiles (the second with a ragged last tile row: the EDGE epilogue, whose row predicate is a buffer-descriptor bound)"""
    from domain_rag_amd import ops
    N, K = 768, 3072
    a, w, ch = _outlier_operands(M, N, K, 70 + M, factor)
    bias = _bf(torch.randn(N, generator=_g(3)))
    with _forced_w4p():
        out = ops.gemm(a.to(gpu), w.to(gpu), bias=bias.to(gpu))
        out_act = ops.gemm(a.to(gpu), w.to(gpu), bias=bias.to(gpu), act=ops.ACT_GELU_TANH)
    _gemm_check(out, a, w, bias=bias, what=f"w4p forced, outliers x{factor:g}, M {M}")
    # GELU(tanh) as torch applies it to a bf16 Linear's output (the reference's F.gelu(linear(x))): the pre-activation is ROUNDED to bf16, the
    # activation evaluated in float32 on that, the result rounded again (csrc/gemm_bf16_kernels.h act4).  Against float64 of the exact pre-activation:
    # |gelu'| <= 1.13, so the first rounding (2^-8 |y|) and the accumulation error pass through at most amplified by that; then one output rounding.
    # (The first run of this test had the one-rounding bar and failed at 1.9 x it in the linear region, where |y| = |gelu(y)|: the bar was wrong.)
    y = a.double() @ w.double().T + bias.double()
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()
    ref = torch.nn.functional.gelu(y, approximate="tanh")
    err = (out_act.double().cpu() - ref).abs()
    bound = 1.01 * BAR_OUT * ref.abs() + 1.13 * (1.01 * BAR_OUT * y.abs() + BAR_ACC * mag) + 1e-6 * ref.abs() + 1e-30
    assert torch.isfinite(out_act.float()).all().item() and not (err > bound).any(), (err / bound).max().item()


def test_gemm_w4p_forced_cancelling_rows(gpu):
    from domain_rag_amd import ops
    M, N, K = 2400, 512, 2048
    g = _g(M)
    u = _bf(torch.randn(M, K // 2, generator=g) * 8)
    v = _bf(torch.randn(N, K // 2, generator=g))
    d = _bf(v.float() * (2.0 ** -7) * torch.sign(torch.randn(N, K // 2, generator=g)))
    a = torch.cat([u, -u], 1).contiguous()
    w = torch.cat([v, _bf(v.float() + d.float())], 1).contiguous()
    with _forced_w4p():
        out = ops.gemm(a.to(gpu), w.to(gpu))
        out32 = ops.gemm(a.to(gpu), w.to(gpu), out_f32=True)
    ref = a.double() @ w.double().T
    mag = a.double().abs() @ w.double().abs().T
    assert (mag / ref.abs().clamp_min(1e-30)).median() > 50
    _gemm_check(out, a, w, what="w4p forced, cancelling")
    # the float32 output carries no output rounding at all: the accumulation bar alone
    assert ((out32.double().cpu() - ref).abs() <= BAR_ACC * mag + 1e-40).all()


def test_gemm_w4p_forced_subnormal_and_max_bf16_operands(gpu):
    from domain_rag_amd import ops
    M, N, K = 600, 256, 512
    g = _g(M + 1)
    a = _bf(torch.randn(M, K, generator=g) * (2.0 ** -129))
    assert (a.float().abs() < BF16_MIN_NORMAL).float().mean() > 0.9 and (a.float() != 0).float().mean() > 0.5
    w = _bf(torch.randn(N, K, generator=g) * (2.0 ** 100))
    sign = torch.sign(torch.randn(M, K, generator=g))
    a2 = _bf(sign * BF16_MAX)
    w2 = _bf(torch.randn(N, K, generator=g) * (2.0 ** -110))
    a3 = _bf(torch.randn(M, K, generator=g) * (2.0 ** -70))
    w3 = _bf(torch.randn(N, K, generator=g) * (2.0 ** -64))
    with _forced_w4p():
        out = ops.gemm(a.to(gpu), w.to(gpu))
        out2 = ops.gemm(a2.to(gpu), w2.to(gpu))
        out3 = ops.gemm(a3.to(gpu), w3.to(gpu)).cpu()
    assert (a.double() @ w.double().T).abs().median() > 2.0 ** -34
    _gemm_check(out, a, w, what="w4p forced, subnormal activations")
    _gemm_check(out2, a2, w2, what="w4p forced, max-bf16 activations")
    ref3 = _bf((a3.float() @ w3.float().T))
    assert (out3.double() - ref3.double()).abs().max() <= 2 * 2.0 ** -133 + BAR_OUT * ref3.double().abs().max()


@pytest.mark.parametrize("S", [1241, 1280])
def test_gemm_w4p_forced_gate_residual_across_a_row_map_batch(gpu, S):
    """x + gate * (a w^T + b) in place on a two-batch row map.  S = 1241 (the DiT's text stream): the tile of rows 1024..1279 holds the end of
    batch 0 and the start of batch 1 — the EDGE epilogue's per-row choice between two bases and two gate vectors; the last tile is ragged.
    S = 1280: batches on tile boundaries (the fast form).  Outlier channels in a, massive activations in the residual stream."""
    from domain_rag_amd import ops
    B, N, K = 2, 1024, 3072
    M = B * S
    a, w, _ = _outlier_operands(M, N, K, 5 + S, 1e3)
    g = _g(9)
    bias = _bf(torch.randn(N, generator=g))
    gate = _bf(torch.randn(B, N, generator=g) * 0.5)
    resid = torch.randn(M, N, generator=g)
    resid[:, ::257] *= 500.0
    resid = _bf(resid)
    # each batch sits at its own place inside a larger buffer, as the joint [txt, img] stream does: batch stride > rows * ld
    stride = (S + 37) * N
    buf = torch.full((B * (S + 37) * N,), 3.0, dtype=torch.bfloat16)
    for b in range(B):
        buf[b * stride: b * stride + S * N] = resid[b * S:(b + 1) * S].reshape(-1)
    x = buf.to(gpu)
    with _forced_w4p():
        ops.gemm(a.to(gpu), w.to(gpu), x, bias=bias.to(gpu), gate=gate.to(gpu), resid=x, M=M, lda=K, ldc=N, c_rows_per_batch=S, c_batch_stride=stride, ldg=N)
    got = x.cpu()
    out = torch.cat([got[b * stride: b * stride + S * N].view(S, N) for b in range(B)])
    for b in range(B):      # the gaps between the batches are nobody's to write
        assert (got[b * stride + S * N: (b + 1) * stride] == 3.0).all()
    y = a.double() @ w.double().T + bias.double()
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()
    gy = gate.double().repeat_interleave(S, 0) * y
    ref = resid.double() + gy
    err = (out.double() - ref).abs()
    bound = 1.02 * BAR_OUT * (ref.abs() + 2 * gy.abs()) + 2 * BAR_ACC * mag
    assert torch.isfinite(out.float()).all().item() and not (err > bound).any(), (err / bound).max().item()


def test_gemm_w4p_forced_two_destinations_with_outliers(gpu):
    """q|k|v + proj_mlp as one launch into two buffers: columns >= n_split go to the second (addressed from C2 - n_split; the EDGE bound is
    the first invalid row's first byte IN THE WAVE'S COLUMNS — round 5's finding iii)"""
    from domain_rag_amd import ops
    M, N, K = 2500, 1024, 1024
    a3, w3, _ = _outlier_operands(M, N, K, 33, 1e3)
    bias = _bf(torch.randn(N, generator=_g(4)))
    oa = torch.full((M + 3, 512), 5.0, dtype=torch.bfloat16, device=gpu); ob = torch.full((M + 3, 512), 5.0, dtype=torch.bfloat16, device=gpu)
    with _forced_w4p():
        ops.gemm(a3.to(gpu), w3.to(gpu), oa, bias=bias.to(gpu), M=M, lda=K, ldc=512, out2=ob, ldc2=512, n_split=512)
    assert (oa[M:] == 5.0).all() and (ob[M:] == 5.0).all()                      # rows behind the ragged edge untouched in BOTH buffers
    _gemm_check(torch.cat([oa[:M], ob[:M]], 1), a3, w3, bias=bias, what="w4p forced, two destinations")


@pytest.mark.parametrize("M,N,K", [(8192, 6144, 384), (4096, 4096, 12288), (2 * 5337, 9216, 3072)])
def test_gemm_w4p_by_policy_outliers_and_cancellation(gpu, M, N, K):
    """shapes the POLICY gives to gemm_bf16_w4p (asserted): 768 tiles at an odd number of K-step pairs; 256 tiles at K = 12 288; the DiT's
    q|k|v launch at B = 2 (ragged edge, 36 x 42 tiles = several rounds of the persistent walk).  Outlier channels, then cancelling halves."""
    from domain_rag_amd import ops
    assert _is_w4p(M, N, K)
    g = torch.Generator(device="cpu").manual_seed(M + K)
    a = torch.randn(M, K, generator=g)
    ch = torch.randperm(K, generator=g)[: max(1, K // 1000)]
    a[:, ch] *= 1e3
    w = torch.randn(N, K, generator=g) * 0.02
    idx = torch.randint(0, N * K, (N * K // 1000,), generator=g)
    w.view(-1)[idx] *= 100.0
    a, w = _bf(a).to(gpu), _bf(w).to(gpu)
    bias = _bf(torch.randn(N, generator=g)).to(gpu)
    out = ops.gemm(a, w, bias=bias)
    _gemm_check_gpu(out, a, w, bias=bias, what=f"w4p by policy, outliers ({M}, {N}, {K})")
    # ... and with the output rounding taken out (float32 output): the accumulation alone, relative to sum |a w|
    out32 = ops.gemm(a, w, bias=bias, out_f32=True)
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()
    acc_err = ((out32.double() - (a.double() @ w.double().T + bias.double())).abs() / mag).max().item()
    assert acc_err < BAR_ACC, acc_err            # (measured 2.3e-6 at K = 3072 with x 1000 channels, 4.1e-6 at K = 12 288: float32 chains of K terms)
    del out, out32, mag
    # cancelling halves along K
    u = _bf(torch.randn(M, K // 2, generator=g) * 8).to(gpu)
    v = _bf(torch.randn(N, K // 2, generator=g)).to(gpu)
    sgn = torch.sign(torch.randn(N, K // 2, generator=g)).to(gpu)
    a2 = torch.cat([u, -u], 1).contiguous()
    w2 = torch.cat([v, _bf(v.float() * (1 + 2.0 ** -7 * sgn))], 1).contiguous()
    out2 = ops.gemm(a2, w2)
    _gemm_check_gpu(out2, a2, w2, what=f"w4p by policy, cancelling ({M}, {N}, {K})")


@pytest.mark.parametrize("M,N,K", [(1536, 3072, 15360), (512, 3072, 12288)])
def test_gemm_split_k_stacked_launch_on_outliers(gpu, M, N, K):
    """the split-K route (S stacked K slices in one gemm_bf16_w4p launch with per-batch W offsets + the reduce pass; the policy's choice for
    these shapes, asserted) on outlier channels that all fall into ONE slice and on cancelling halves that fall into DIFFERENT slices —
    the f32 partials must carry the cancellation; bias + gate + residual through the reduce pass"""
    import ctypes
    from domain_rag_amd import _lib, ops
    g = torch.Generator(device="cpu").manual_seed(K + M)
    a = torch.randn(M, K, generator=g)
    a[:, 5:K // 16:97] *= 1e3                                  # every outlier channel inside the first K slice
    w = torch.randn(N, K, generator=g) * 0.02
    a, w = _bf(a).to(gpu), _bf(w).to(gpu)
    bias = _bf(torch.randn(N, generator=g)).to(gpu)
    ops.gemm(a[:256], w[:256])                                 # (registers the workspace)
    args, _, _ = ops._gemm_args(a, w, bias=bias)
    assert _lib.load().drag_gemm_bf16_splitk_slices(ctypes.byref(args)) >= 2
    out = ops.gemm(a, w, bias=bias)
    _gemm_check_gpu(out, a, w, bias=bias, what=f"split-K, outliers in one slice ({M}, {N}, {K})")
    u = _bf(torch.randn(M, K // 2, generator=g) * 8).to(gpu)
    v = _bf(torch.randn(N, K // 2, generator=g)).to(gpu)
    sgn = torch.sign(torch.randn(N, K // 2, generator=g)).to(gpu)
    a2 = torch.cat([u, -u], 1).contiguous()
    w2 = torch.cat([v, _bf(v.float() * (1 + 2.0 ** -7 * sgn))], 1).contiguous()
    out2 = ops.gemm(a2, w2)
    _gemm_check_gpu(out2, a2, w2, what=f"split-K, cancelling across slices ({M}, {N}, {K})")
    # gate + residual through the reduce pass
    gate = _bf(torch.randn(1, N, generator=g) * 0.5).to(gpu)
    resid = torch.randn(M, N, generator=g); resid[:, ::257] *= 500.0
    resid = _bf(resid).to(gpu)
    x = resid.clone()
    ops.gemm(a, w, x, bias=bias, gate=gate, resid=x, c_rows_per_batch=M, c_batch_stride=M * N, ldg=N)
    y = a.double() @ w.double().T + bias.double()
    mag = a.double().abs() @ w.double().abs().T + bias.double().abs()
    gy = gate.double() * y
    ref = resid.double() + gy
    err = (x.double() - ref).abs()
    bound = 1.02 * BAR_OUT * (ref.abs() + 2 * gy.abs()) + 2 * BAR_ACC * mag
    assert torch.isfinite(x.float()).all().item() and not (err > bound).any().item(), (err / bound).max().item()


def test_gemm_pair_split_k_on_outliers(gpu):
    """the pair form of the split (configs[1]'s ff down-projections: ONE partial launch over both problems' stacked rows, the rows behind M1
    of every slice reading the second problem's A and W) with outlier channels in one problem only: nothing may leak across `split_m1`"""
    import ctypes
    from domain_rag_amd import _lib, ops
    M1, M2, N, K = 1024, 512, 3072, 12288
    g = torch.Generator(device="cpu").manual_seed(77)
    a1 = torch.randn(M1, K, generator=g); a1[:, 11::1000] *= 1e3
    a2 = torch.randn(M2, K, generator=g) * 1e-3                                   # a quiet second problem: a leak of the first would drown it
    w1 = torch.randn(N, K, generator=g) * 0.02
    w2 = torch.randn(N, K, generator=g) * 0.02
    a1, a2, w1, w2 = _bf(a1).to(gpu), _bf(a2).to(gpu), _bf(w1).to(gpu), _bf(w2).to(gpu)
    o1 = torch.empty(M1, N, dtype=torch.bfloat16, device=gpu); o2 = torch.empty(M2, N, dtype=torch.bfloat16, device=gpu)
    ops.gemm(a1[:256], w1[:256])
    g1, _, _ = ops._gemm_args(a1, w1)
    g2, _, _ = ops._gemm_args(a2, w2)
    assert _lib.load().drag_gemm_bf16_pair_splitk_slices(ctypes.byref(g1), ctypes.byref(g2)) >= 2
    ops.gemm_pair(dict(a=a1, w=w1, out=o1), dict(a=a2, w=w2, out=o2))
    _gemm_check_gpu(o1, a1, w1, what="pair split-K, loud problem")
    _gemm_check_gpu(o2, a2, w2, what="pair split-K, quiet problem")


# ------------------------------------------------------------------ row softmax (the VAE's mid-block attention)
@pytest.mark.parametrize("cols", [100, 4096, 16384])
def test_softmax_rows_dominant_logit_at_every_lane_position(gpu, cols):
    from domain_rag_amd import ops
    rows = 512
    g = _g(cols)
    x = torch.randn(rows, cols, generator=g) * 3
    pos = (torch.arange(rows) * 67 + (torch.arange(rows) // 64)) % cols           # every lane, every 16-byte slot, both row ends
    x[torch.arange(rows), pos] = 400.0                                              # scale 0.3: 120 above the rest, exp(120) overflows float32
    x[3] = -1e4                                                                     # a row of equal, hugely negative logits: uniform
    x[4, : cols // 2] = -float("inf")                                               # masked half
    x[5] = 0.0; x[5, cols - 1] = 88.0 / 0.3                                         # exp(88) is the last finite float32 power
    ld = (cols + 63) // 64 * 64
    y = torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=gpu)
    ops.softmax_rows(x.to(gpu), y, rows, cols, 0.3, ldy=ld)
    ref = torch.softmax(x.double() * 0.3, -1)
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    err = (got[:, :cols] - ref).abs()
    # one bf16 rounding of a float32 result that carries ~1e-6 of its own (exp, the row sum)
    assert not (err > 1.01 * BAR_OUT * ref + 1e-38).any(), (err / (BAR_OUT * ref + 1e-38)).max().item()
    assert (got[torch.arange(rows), pos][6:] == 1.0).all() and (got[:, cols:] == 0).all()
    assert abs(got[3, :cols].sum().item() - 1.0) < 4e-3 and (got[4, : cols // 2] == 0).all()


# ------------------------------------------------------------------ RMSNorm + RoPE + V^T at extreme row norms
def test_qk_norm_rope_vt_row_norms_from_1e_minus_20_to_1e18(gpu):
    """per-head RMSNorm of q / k rows whose norms span 38 decades: x * rsqrt(mean(x^2) + eps) with the mean in float32 like the reference
    (oracle/flux.py rms_norm == diffusers' RMSNorm) — squares of 1e18 sum to 1.3e38 (just finite), squares of 1e-20 are float32 subnormals"""
    from domain_rag_amd import ops
    from oracle import flux as oflux
    B, H = 1, 2
    exps = list(range(-20, 19))
    S = len(exps) * 4
    D = H * 128
    g = _g(0)
    qkv = torch.randn(B, S, 3 * D, generator=g)
    for i in range(S):
        qkv[0, i, : 2 * D] *= 10.0 ** exps[i // 4]
    qkv[0, 7, :128] = 0.0                                   # an all-zero head row: rsqrt(eps) * 0
    qkv[0, 9, 128:256] = 0.0; qkv[0, 9, 128 + 5] = 3e18     # one element carries the whole norm
    qkv = _bf(qkv)
    s_txt = 40
    wq, wk, cwq, cwk = (_bf(1 + 0.1 * torch.randn(128, generator=g)) for _ in range(4))
    ids = torch.zeros(S, 3); ids[s_txt:, 1] = torch.arange(S - s_txt) // 8; ids[s_txt:, 2] = torch.arange(S - s_txt) % 8
    cos, sin = oflux.rope_tables(ids)
    qd = qkv.to(gpu).clone()
    s_pad = (S + 63) // 64 * 64
    vt = torch.full((B, H, 128, s_pad), float("nan"), dtype=torch.bfloat16, device=gpu)
    ops.qk_norm_rope_vt(qd, vt, cwq.to(gpu), cwk.to(gpu), wq.to(gpu), wk.to(gpu), cos.to(gpu), sin.to(gpu), B, S, H, 3 * D, s_txt)
    got = qd.cpu()
    assert torch.isfinite(got.float()).all()
    for which, (wt, wi) in enumerate(((cwq, wq), (cwk, wk))):
        x = qkv[..., which * D:(which + 1) * D].view(B, S, H, 128).transpose(1, 2)
        ref = torch.cat([oflux.rms_norm(x[:, :, :s_txt], wt), oflux.rms_norm(x[:, :, s_txt:], wi)], 2)
        ref = oflux.apply_rope(ref, cos, sin)
        g_ = got[..., which * D:(which + 1) * D].view(B, S, H, 128).transpose(1, 2)
        # against the bf16 oracle (same rounding points): at most an ulp of bf16 per element, and nothing on most of them
        # (the rotation is a0 c - a1 s in float32: the kernel contracts it to one fma, torch rounds both products — a few float32 ulps of the
        #  PAIR's magnitude, which is all of an element the rotation made small)
        d = (g_.double() - ref.double()).abs()
        rpair = ref.double().reshape(*ref.shape[:-1], 64, 2).pow(2).sum(-1, keepdim=True).sqrt().expand(*ref.shape[:-1], 64, 2).reshape(ref.shape)
        # and the device's rsqrt is 1 ulp of float32 from the host's: now and then an input of the rotation lands on the other side of a bf16
        # rounding boundary, which moves BOTH outputs of its pair by up to that ulp — measured on 5 of 156 rows.  So: within one bf16 ulp of
        # the pair, and bit-identical on all but a few elements
        bad = d > 2.0 ** -7 * (ref.double().abs() + rpair) + 1e-30
        assert (g_ == ref).float().mean().item() > 0.995, (g_ == ref).float().mean().item()
        assert not bad.any(), ("q" if which == 0 else "k", "vs the bf16 oracle", (d / (rpair + 1e-30)).max().item(),
                               "rows (10^exponent of their scale):", sorted({(int(i[2]), exps[int(i[2]) // 4]) for i in bad.nonzero()})[:12])
        # against float64 of the definition, rowwise: the normalised row has unit rms whatever the input scale (rows of norm >= 1e-2:
        # below that eps = 1e-6 takes over by design)
        x64 = x.double()
        n64 = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + 1e-6)
        w64 = torch.cat([wt.double().expand(B, H, s_txt, 128), wi.double().expand(B, H, S - s_txt, 128)], 2)
        r64 = oflux.apply_rope((n64 * w64).float(), cos, sin).double()
        # three bf16 roundings (normalised x, x * weight, the rotated pair), the first two entering BOTH elements of a rotated pair: the
        # bar is relative to the pair's magnitude (which the rotation preserves), not to an element the rotation may have made small
        dd = (g_.double() - r64).abs()
        pair = r64.reshape(*r64.shape[:-1], 64, 2).pow(2).sum(-1, keepdim=True).sqrt().expand(*r64.shape[:-1], 64, 2).reshape(r64.shape)
        bad = dd > 4 * 2.0 ** -8 * pair + 1e-30
        assert not bad.any(), ("q" if which == 0 else "k", "vs float64", (dd / (pair + 1e-30)).max().item(),
                               "rows (10^exponent of their scale):", sorted({(int(i[2]), exps[int(i[2]) // 4]) for i in bad.nonzero()})[:12])
    assert torch.equal(got[..., 2 * D:], qkv[..., 2 * D:])
    v = qkv[..., 2 * D:].view(B, S, H, 128)
    # V^T image: keys permuted inside 16-groups (csrc/attention_prep.hip); compare as sets per (head, d, 16-key group)
    vtc = vt.cpu()[..., :S - S % 16].view(B, H, 128, -1, 16).float().sort(-1).values
    vr = v.permute(0, 2, 3, 1)[..., :S - S % 16].reshape(B, H, 128, -1, 16).float().sort(-1).values
    assert torch.equal(vtc, vr)


@pytest.mark.parametrize("S", [1100, 4160])
def test_attention_on_outlier_channels_and_near_duplicate_keys(gpu, S):
    """q / k with a massive channel (one head dimension 100 x the others: scores dominated by one product) and a block of keys that are
    exact duplicates (ties in the running maximum): both attention families against float64 on the kernel's own bf16 q / k"""
    from domain_rag_amd import ops
    from oracle import ops_ref
    B, H = 1, 2
    D = H * 128
    g = _g(S)
    qkv = torch.randn(B, S, 3 * D, generator=g)
    qkv[..., 17] *= 30.0; qkv[..., D + 17] *= 30.0              # one q and one k channel of head 0: scores ~ 900 x N(0, 1) / sqrt(128)
    qkv[0, 100:164, D:2 * D] = qkv[0, 100, D:2 * D].clone()       # 64 identical keys (a whole tile of ties)
    qkv = _bf(qkv)
    scale = 1 / math.sqrt(128)
    qd = qkv.to(gpu).clone()
    s_pad = (S + 63) // 64 * 64
    vt = torch.empty(B, H, 128, s_pad, dtype=torch.bfloat16, device=gpu)
    ops.qk_norm_rope_vt(qd, vt, None, None, None, None, None, None, B, S, H, 3 * D, 0)
    q, k, v = (t.view(B, S, H, 128).transpose(1, 2) for t in qkv.split(D, -1))
    ref = ops_ref.attention_ref_f64(q, k, v, scale)
    outs = []
    for q64 in (2, 1):                                          # 8-wave family, 64-query kernel
        with ops.options(attn_q64=q64):
            o = torch.full((B, S, D), float("nan"), dtype=torch.bfloat16, device=gpu)
            ops.attention(qd, qd.view(-1)[D:], vt, o, B, S, H, 3 * D, S * 3 * D, D, S * D, scale)
        o = o.cpu()
        assert torch.isfinite(o.float()).all()
        # P is rounded to bf16 before P V (like every flash kernel): 2^-8 of the value range per row + the output rounding
        err = (o.double() - ref).abs()
        outs.append(o)
        vmax = v.double().abs().amax()
        assert err.max() <= 1.5e-2 * vmax, (q64, err.max().item(), vmax.item())
    assert torch.equal(outs[0], outs[1]), "the two attention families must agree bit for bit on these inputs too"


# ------------------------------------------------------------------ the float32 CLIP tower's attention and the ResNet stem
@pytest.mark.parametrize("T,hd", [(50, 64), (64, 32), (17, 48)])
def test_attention_small_f32_hot_key_at_every_position(gpu, T, hd):
    """CLIP ViT attention (50 tokens x 64): one key owns each query's softmax, at every key position in turn, with scores around +-200
    (exp overflows float32 without the running maximum); plus a fully tied row"""
    from domain_rag_amd import ops
    B, H = T, 2                       # image b puts the hot key at position b
    D = H * hd
    g = _g(T)
    qkv = torch.randn(B * T, 3 * D, generator=g)
    q = qkv[:, :D].view(B, T, H, hd); k = qkv[:, D:2 * D].view(B, T, H, hd)
    for b in range(B):
        k[b, b] = 25.0 * q[b, 0]        # token 0's query scores 25 |q|^2 / sqrt(hd) ~ 25 sqrt(hd) against it, the others ~ N(0, 25) either way
    k[0, :, 1] = k[0, 0, 1].clone()     # head 1 of image 0: all keys equal -> uniform probabilities
    qkv = qkv.contiguous()
    out = torch.full((B * T, D), 9.0, device=gpu)
    scale = 1 / math.sqrt(hd)
    ops.attention_small_f32(qkv.to(gpu), out, B, T, H, hd, 3 * D, D, scale)
    qq, kk, vv = (qkv[:, i * D:(i + 1) * D].view(B, T, H, hd).permute(0, 2, 1, 3).double() for i in range(3))
    sc = qq @ kk.transpose(-1, -2) * scale
    assert sc.abs().max() > 100
    ref = (torch.softmax(sc, -1) @ vv).permute(0, 2, 1, 3).reshape(B * T, D)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    # float32 scores of magnitude |s| carry an absolute error ~ |s| 2^-24 x sqrt(hd) into the exponent: relative 3e-5 at |s| = 200
    assert (got - ref).abs().max().item() < 2e-4 * vv.abs().max().item(), (got - ref).abs().max().item()
    u = got.view(B, T, H, hd)[0, :, 1]
    assert (u - vv[0, 1].mean(0)).abs().max() < 1e-5


def test_stem_style_on_flat_and_hot_pixel_images(gpu):
    """the 128-d style vector is (mean, std) per stem channel: an almost constant image (std/mean ~ 1e-4: E[x^2] - E[x]^2 would lose it in
    float32) and an image with one saturated pixel on black"""
    from domain_rag_amd.retrieval import StemStyle
    from oracle import stem as ostem
    st = StemStyle(device=gpu, seed=3)
    g = _g(2)
    flat = 0.6 + 1e-4 * torch.randn(2, 3, 256, 256, generator=g)
    hot = torch.zeros(1, 3, 128, 192); hot[0, :, 77, 131] = 1.0
    bright = torch.full((1, 3, 96, 64), 1.0); bright[0, 1, ::7, ::5] = 0.0
    for name, x in (("flat", flat), ("hot pixel", hot), ("bright", bright)):
        got = st(x).cpu().double()
        ref64 = ostem.style_vector(x.double(), {k: (v.double() if torch.is_floating_point(v) else v) for k, v in st.state.items()}).double()
        assert torch.isfinite(got).all()
        err = (got - ref64).abs()
        # float32 convolution (147 taps) + float32 statistics over >= 1500 positions: 1e-5 relative to the channel's magnitude scale
        scale = ref64.abs().view(got.shape[0], 2, -1).amax(1, keepdim=True).expand(-1, 2, -1).reshape(got.shape) + 1e-6
        assert (err <= 2e-4 * scale + 1e-6).all(), (name, (err / scale).max().item())


# ------------------------------------------------------------------ blocks and the 30-step chain on heavy-tailed weights
def _heavy_tailed(params, seed, nu=3):
    """every Linear weight redrawn from Student-t(nu) at the variance init_params gave it: a 3072 x 3072 matrix then holds entries beyond
    100 sigma; biases and norm scales stay"""
    g = _g(seed)
    out = {}
    for k, v in params.items():
        if k.endswith(".weight") and v.dim() == 2:
            std = v.float().std().item()
            out[k] = (_student_t(tuple(v.shape), nu, g) * std).to(v.dtype)
        else:
            out[k] = v
    return out


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


def test_blocks_on_student_t_weights_and_outlier_hidden_states(gpu):
    """1 double + 1 single block at the real width (D = 3072, 24 heads) with Student-t(3) weights, hidden-state inputs that carry massive
    channels, against both oracles: HIP at most 1.3 x as far from float32 as the reference-dtype oracle (max) and 1.1 x (rms)"""
    from domain_rag_amd.flux import FluxTransformerHIP, latent_image_ids
    from domain_rag_amd.flux_params import FluxConfig, init_params
    from oracle import flux as oflux
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    cfg = FluxConfig(in_channels=384, num_layers=1, num_single_layers=1)
    params = _heavy_tailed(init_params(cfg, seed=41), 42)
    g = _g(43)
    St, h, w = 200, 24, 24
    hidden = torch.randn(1, h * w, 384, generator=g); hidden[..., 11] *= 300.0; hidden[..., 200] *= 50.0
    enc = torch.randn(1, St, 4096, generator=g); enc[..., 999] *= 1000.0
    hidden, enc = _bf(hidden), _bf(enc)
    pooled = _bf(torch.randn(1, 768, generator=g))
    t, gd = torch.tensor([0.6172]), torch.tensor([30.0])
    img_ids, txt_ids = latent_image_ids(h, w), torch.zeros(St, 3)
    ocfg = oflux.FluxConfig(**{k: getattr(cfg, k) for k in cfg.__dataclass_fields__})
    taps_ref, taps32, taps = {}, {}, {}
    p32 = {k: v.float() for k, v in params.items()}
    from conftest import oracle_threads
    with torch.no_grad():
        oracle_threads(torch.bfloat16)
        ref = oflux.flux_forward(params, ocfg, hidden, enc, pooled, t, img_ids, txt_ids, gd, taps=taps_ref)
        oracle_threads(torch.float32)
        ref32 = oflux.flux_forward(p32, ocfg, hidden.float(), enc.float(), pooled.float(), t, img_ids, txt_ids, gd, taps=taps32, time_dtype=torch.bfloat16)
    out = FluxTransformerHIP(cfg, params, gpu)(hidden.to(gpu), enc.to(gpu), pooled.to(gpu), t, img_ids, txt_ids, gd, taps=taps)
    rows = []
    for name, got, rbf, r32 in (("double.0", taps["double.0"], taps_ref["double.0"], taps32["double.0"]),
                                ("single.0", taps["single.0"], taps_ref["single.0"], taps32["single.0"]), ("out", out, ref, ref32)):
        assert torch.isfinite(got.float()).all(), name
        e, e_or, r, r_or = _rel(got, r32), _rel(rbf, r32), _rel_rms(got, r32), _rel_rms(rbf, r32)
        rows.append((name, e, e_or, r, r_or))
        print(f"[adversarial] student-t blocks {name}: HIP-f32 max {e:.3e} rms {r:.3e} | bf16 oracle-f32 max {e_or:.3e} rms {r_or:.3e} | ratios {e / max(e_or, 1e-30):.2f} {r / max(r_or, 1e-30):.2f}", flush=True)
    for name, e, e_or, r, r_or in rows:
        assert e < max(1e-2, 1.3 * e_or), f"{name}: HIP vs f32 {e:.4e}, bf16 oracle vs f32 {e_or:.4e} (bar 1.3)"
        assert r < max(2.5e-3, 1.1 * r_or), f"{name}: rms HIP vs f32 {r:.4e}, bf16 oracle vs f32 {r_or:.4e} (bar 1.1)"


def test_fill_30_chained_steps_on_student_t_weights(gpu):
    """the metric's 30-step Fill chain (tests/test_gpu_chained_steps.py) with every DiT Linear drawn from Student-t(3): per-step bars of that
    file (rms 1.1 x, max 1.4 x the bf16 oracle's distance from float32, linear growth), pixels within max(1e-2, 1.3 x)"""
    import json
    import time
    from domain_rag_amd import fill_pipeline as fp, vae
    from domain_rag_amd.flux import FluxTransformerHIP
    from oracle import fill as ofill
    import test_gpu_chained_steps as chained
    t_start = time.time()
    res, steps, strength, St = 256, 30, 1.0, 48
    cfg, ocfg, tp_dev, tp, vcfg, vp = chained._setup(384, 2, 4, 50, gpu)
    tp = _heavy_tailed(tp, 51)
    tp_dev = {k: v.to(gpu) for k, v in tp.items()}
    g = _g(52)
    yy, xx = torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")
    base = torch.stack([128 + 90 * torch.sin(xx / 23.0 + c) * torch.cos(yy / 17.0 - c) for c in range(3)], -1)
    image = (base + 8 * torch.randn(res, res, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]
    mask = torch.full((1, res, res), 255, dtype=torch.uint8); mask[:, 90:166, 80:170] = 0
    pe = torch.randn(1, St, 4096, generator=g); pe[..., 123] *= 200.0
    pe = _bf(pe); pp = _bf(torch.randn(1, 768, generator=g))
    en = _bf(torch.randn(1, 16, res // 8, res // 8, generator=g)); mn = _bf(torch.randn(1, 16, res // 8, res // 8, generator=g))
    nt = _bf(torch.randn(1, (res // 16) ** 2, 64, generator=g))
    fill = fp.FluxFillHIP(FluxTransformerHIP(cfg, tp_dev, gpu), vae.FluxVaeHIP(vcfg, vp, gpu))
    hip_lat = {}
    out = fill(image.to(gpu), mask.to(gpu), pe.to(gpu), pp.to(gpu), guidance_scale=30.0, num_inference_steps=steps, strength=strength,
               enc_noise=en.to(gpu), masked_enc_noise=mn.to(gpu), noise_tokens=nt.to(gpu),
               on_step=lambda i, lat: hip_lat.__setitem__(i, lat.float().cpu())).cpu()
    del fill, tp_dev
    torch.cuda.empty_cache()
    taps, imgs = {}, {}
    from conftest import oracle_threads
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        oracle_threads(dt)
        cast = (lambda d: {k: v.to(dt) for k, v in d.items()})
        taps[name] = {}
        with torch.no_grad():
            _, img = ofill.fill_pipeline(cast(tp), ocfg, cast(vp), dict(block_out=vcfg.block_out_channels, layers=vcfg.layers_per_block),
                                         image, mask, pe, pp, 30.0, steps, strength, en, mn, nt, dtype=dt, taps=taps[name])
        imgs[name] = img.float()
    rows = chained._curves(hip_lat, taps["f32"], taps["bf16"], range(steps))
    hip = out.float() / 255.0
    e = (hip - imgs["f32"].permute(0, 2, 3, 1)).abs().max().item()
    e_or = (imgs["bf16"] - imgs["f32"]).abs().max().item()
    chained._report("fill30_student_t", rows, {"pipeline": "Fill, 30 steps, 256x256, 2 double + 4 single blocks at D=3072, Student-t(3) weights, outlier text channel",
                                               "pixels_hip_vs_f32": e, "pixels_bf16_oracle_vs_f32": e_or, "pixel_ratio": e / max(e_or, 1e-30),
                                               "seconds": time.time() - t_start})
    chained._check(rows, "Fill x30, Student-t weights")
    assert e <= max(1e-2 + 0.5 / 255, 1.3 * e_or), f"pixels: HIP vs f32 {e:.4f}, bf16 oracle vs f32 {e_or:.4f}"


# ------------------------------------------------------------------ GroupNorm's shift, the VAE on extreme images and latents
def test_groupnorm_outlier_or_inf_at_the_pixels_the_shift_is_taken_from(gpu):
    """the statistics are sums of x - c and (x - c)^2 (round 4); c was the group's element at (pixel 0, first channel): ONE outlier there
    brought E[x^2] - E[x]^2 back for a large-mean group, ONE Inf there made every statistic of the group NaN.  c is now the
    mean of the group's channels at four pixels; a non-finite c counts as 0.  Against torch's float64 GroupNorm (the reference's is torch's)."""
    import torch.nn.functional as F
    from domain_rag_amd import ops
    g_ = _g(11)
    for C, H, W in [(128, 64, 64), (512, 24, 24)]:
        B, cpg = 2, C // 32
        x = torch.randn(B, C, H, W, generator=g_)
        for grp, (mean, spread) in {3: (100.0, 0.5), 7: (-300.0, 2.0)}.items():
            x[:, grp * cpg:(grp + 1) * cpg] = mean + spread * torch.randint(-1, 2, (B, cpg, H, W), generator=g_).float()
        x[0, 3 * cpg, 0, 0] = 3e4          # the old shift element of group 3: an outlier 300 x the group's mean
        x[1, 7 * cpg, 0, 0] = -2e5         # and of group 7 in the other image
        x[:, 5 * cpg:(5 + 1) * cpg, 0, 0] = 1e3      # every channel of group 5 at pixel 0 (one of the four shift pixels) is an outlier
        x = _bf(x).float()
        gam, bet = _bf(torch.randn(C, generator=g_)), _bf(torch.randn(C, generator=g_))
        ref = F.group_norm(x.double(), 32, gam.double(), bet.double(), 1e-6)
        y = torch.zeros((B, H, W, C), dtype=torch.bfloat16, device=gpu)
        ops.groupnorm_silu(_bf(x.permute(0, 2, 3, 1).contiguous()).to(gpu), y, gam.to(gpu), bet.to(gpu), B, H, W, C, out_pad=0, silu=False)
        got = y.cpu().double().permute(0, 3, 1, 2)
        for grp in (3, 7, 5, 0, 20):
            sl = slice(grp * cpg, (grp + 1) * cpg)
            e = ((got[:, sl] - ref[:, sl]).abs().max() / ref[:, sl].abs().max()).item()
            assert e < 1.5e-2, (C, grp, e)
        # one Inf: that group's output is non-finite in torch too; every OTHER group stays exact
        xi = x.clone(); xi[0, 9 * cpg, 0, 0] = float("inf")
        y2 = torch.zeros((B, H, W, C), dtype=torch.bfloat16, device=gpu)
        ops.groupnorm_silu(_bf(xi.permute(0, 2, 3, 1).contiguous()).to(gpu), y2, gam.to(gpu), bet.to(gpu), B, H, W, C, out_pad=0, silu=False)
        got2 = y2.cpu().double().permute(0, 3, 1, 2)
        keep = torch.ones(C, dtype=torch.bool); keep[9 * cpg:10 * cpg] = False
        assert torch.equal(got2[:, keep], got[:, keep]) and torch.equal(got2[1], got[1])
        assert not torch.isfinite(got2[0, 9 * cpg:10 * cpg]).all()


def test_vae_on_extreme_images_and_latents(gpu):
    """the Fill pipeline's two encodes on saturated / flat / checkerboard pictures (uint8 0 and 255 everywhere, a 1-pixel checkerboard: the
    largest high-frequency content an image can hold) and its decode on latents with a massive channel and a flat region — against the bf16
    and float32 oracles on the same weights, bar 1.3 x the reference dtype's own distance from float32"""
    from domain_rag_amd import vae
    from oracle import vae as ov
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    cfg = vae.VaeConfig()
    p = vae.init_params(cfg, seed=5)
    p32 = {k: v.float() for k, v in p.items()}
    model = vae.FluxVaeHIP(cfg, p, gpu)
    res, h, w = 256, 16, 16
    yy, xx = torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")
    imgs = torch.stack([torch.full((res, res, 3), 255, dtype=torch.uint8), torch.zeros((res, res, 3), dtype=torch.uint8),
                        (((yy + xx) % 2) * 255).to(torch.uint8)[..., None].expand(res, res, 3).contiguous(),
                        torch.where(xx[..., None] < res // 2, torch.tensor(255), torch.tensor(0)).to(torch.uint8).expand(res, res, 3).contiguous()])
    B = imgs.shape[0]
    toks = torch.empty((B, h * w, 64), dtype=torch.bfloat16, device=gpu)
    model.encode_to_tokens(imgs.to(gpu), None, None, toks, 64)
    toks = toks.cpu()
    assert torch.isfinite(toks.float()).all()
    with torch.no_grad():
        for b in range(B):
            x = ov.preprocess_image(imgs[b:b + 1])
            ref = ov.pack_latents(ov.sample_latents(ov.encode_moments(p32, x), None))
            refb = ov.pack_latents(ov.sample_latents(ov.encode_moments(p, x.bfloat16()), None))
            e, e_or = _rel(toks[b:b + 1], ref), _rel(refb, ref)
            print(f"[adversarial] vae encode image {b}: HIP-f32 {e:.3e} | bf16 oracle-f32 {e_or:.3e} | ratio {e / max(e_or, 1e-30):.2f}", flush=True)
            assert e < max(1.5e-2, 1.3 * e_or), (b, e, e_or)
    g = _g(6)
    lat = torch.randn(2, h * w, 64, generator=g)
    lat[0, :, 7] *= 40.0                    # a massive latent channel
    lat[1, : h * w // 2] = 0.25             # a flat half
    lat[1, 5, :] = 60.0                     # one hot token
    lat = _bf(lat)
    img_u8, rows = model.decode_tokens(lat.to(gpu), 2, h, w, return_rows=True)
    got = (rows.view(2, res, res, -1)[..., :3].float().cpu() / 2 + 0.5).clamp(0, 1).permute(0, 3, 1, 2)
    with torch.no_grad():
        for b in range(2):
            _, ref32 = ov.decode_tokens_to_u8(p32, lat[b:b + 1].float(), h, w)
            _, refbf = ov.decode_tokens_to_u8(p, lat[b:b + 1], h, w)
            e, e_or = _rel(got[b:b + 1], ref32), _rel(refbf, ref32)
            print(f"[adversarial] vae decode latents {b}: HIP-f32 {e:.3e} | bf16 oracle-f32 {e_or:.3e} | ratio {e / max(e_or, 1e-30):.2f}", flush=True)
            assert e < max(1e-2, 1.3 * e_or), (b, e, e_or)


# ------------------------------------------------------------------ operand room of the bf16 GEMM (ops._rows_reach / ops._fit)
def _gemm_exact_room_launch(gpu):
    """a batched launch (M = 5 rows in batches of 4, N = 8, K = 64) in which every operand's storage ends with the last element that the
    launch addresses: (keywords of ``ops.gemm``, {operand: elements}, the dense operands for the float64 yardstick)"""
    from domain_rag_amd import ops
    M, N, K, rpb = 5, 8, 64, 4
    lda, a_bs, ldc, c_bs, ldg = 72, 4 * 72, 16, 4 * 16 + 8, 16
    room = dict(a=ops._rows_reach(M, K, lda, rpb, a_bs), out=ops._rows_reach(M, N, ldc, rpb, c_bs), gate=ops._rows_reach(2, N, ldg), bias=N)
    assert room == dict(a=288 + K, out=72 + N, gate=ldg + N, bias=N)                       # the last row is row 0 of batch 1
    room["resid"] = room["out"]
    g = _g(5)
    a_rows, w, bias = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(N, K, generator=g)), _bf(torch.randn(N, generator=g))
    a = torch.full((room["a"],), float("nan"), dtype=torch.bfloat16)
    gate = torch.full((room["gate"],), float("nan"), dtype=torch.bfloat16)
    for r in range(M):
        a[(r // rpb) * a_bs + (r % rpb) * lda:][:K] = a_rows[r]
    gate[:N], gate[ldg:ldg + N] = 1.0, 2.0              # powers of two over a zero residual: each row is its batch's multiple of the plain product
    kw = dict(a=a.to(gpu), w=w.to(gpu), out=torch.full((room["out"],), -7.0, dtype=torch.bfloat16, device=gpu), bias=bias.to(gpu),
              gate=gate.to(gpu), resid=torch.zeros(room["resid"], dtype=torch.bfloat16, device=gpu), M=M, a_rows_per_batch=rpb, a_batch_stride=a_bs,
              lda=lda, c_rows_per_batch=rpb, c_batch_stride=c_bs, ldc=ldc, ldg=ldg)
    for name, n in room.items():
        assert ops._room(kw[name]) == n, name
    return kw, room, (a_rows.to(gpu), bias.to(gpu))


def test_gemm_passes_where_every_operand_has_exactly_the_room_it_reaches(gpu):
    from domain_rag_amd import ops
    kw, room, (a_rows, bias) = _gemm_exact_room_launch(gpu)
    out = ops.gemm(**kw)
    M, N, rpb, ldc, c_bs = kw["M"], 8, 4, kw["ldc"], kw["c_batch_stride"]
    offs = [(r // rpb) * c_bs + (r % rpb) * ldc for r in range(M)]
    got = torch.stack([out[o:o + N] / (1.0 + r // rpb) for r, o in enumerate(offs)])       # (the gate: 1 in batch 0, 2 in batch 1)
    _gemm_check_gpu(got, a_rows, kw["w"], bias=bias, what="room == reach")
    owned = torch.zeros(room["out"], dtype=torch.bool, device=gpu)
    for o in offs:
        owned[o:o + N] = True
    assert (out[~owned] == -7.0).all()


@pytest.mark.parametrize("short", ["a", "out", "resid", "gate", "bias"])
def test_gemm_refuses_an_operand_one_element_short_of_its_reach(gpu, short):
    """refused before anything is launched: the batched destination and the operands that only the MXFP8 route used to check"""
    from domain_rag_amd import ops
    kw, room, _ = _gemm_exact_room_launch(gpu)
    kw[short] = torch.zeros(room[short] - 1, dtype=torch.bfloat16, device=gpu)
    before = kw["out"].clone()
    with pytest.raises(ValueError, match=rf"gemm\.{short}"):
        ops.gemm(**kw)
    with pytest.raises(ValueError, match=rf"gemm\.{short}"):
        ops.gemm_pair(kw, kw)
    assert torch.equal(kw["out"], before)
