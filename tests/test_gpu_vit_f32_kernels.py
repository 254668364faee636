"""The float32 front end of the CLIP image tower and the ResNet stem (csrc/vit_f32.hip, csrc/stem.hip, and linear_f32 on conv2d_f32_kernel of
csrc/lama.hip), each kernel called directly.

vit_prepare only moves and divides: bit-equal to its numpy float32 restatement.  The kernels that sum (layernorm_f32, clip_embed_ln,
linear_f32, resnet_stem_style) cannot be restated bit for bit — a 64-lane tree or a matrix core adds in another order than any host loop —
so they are held to the reference's own float32 error: with ``ref`` = torch in float64 on the same inputs and ``e_t`` = the max abs error
of torch's float32 CPU operator against ``ref`` on that input, the kernel's max abs error against ``ref`` may be at most 4 e_t (the factor
covers the other summation order; it is not fitted to the kernel).  Where e_t is 0 the floor is 2^-22 max|ref|.  The measured ratios are
recorded in DESIGN.md (test notes).  Outputs are slices of a larger buffer filled with a sentinel (7.0), >= 256 guard elements on both
sides, gap columns included; all of them must hold the sentinel after the call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 256
F32 = np.float32


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), 7.0, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _is_sentinel(t):
    return bool((t.cpu().contiguous().view(torch.int32) == torch.tensor(7.0).view(torch.int32)).all())


def _assert_guards(buf, n):
    assert _is_sentinel(buf[:GUARD]), "guard before the buffer was written"
    assert _is_sentinel(buf[GUARD + n:]), "guard after the buffer was written"


def _bits(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().contiguous().view(torch.int32)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _check_ratio(name, got, ref64, t32):
    """the bound of the module docstring; prints the measured ratio (kernel vs float64 over torch-f32 vs float64)"""
    ref64 = ref64.double()
    e_k = (got.double().cpu() - ref64).abs().max().item()
    e_t = (t32.double() - ref64).abs().max().item()
    base = e_t if e_t > 0 else 2.0 ** -22 * ref64.abs().max().item()
    print(f"f32-ratio {name}: kernel {e_k:.3e} torch-f32 {e_t:.3e} ratio {e_k / base if base > 0 else 0.0:.2f}")
    assert e_k <= 4 * base, f"{name}: kernel error {e_k:.3e} vs float64, torch float32 {e_t:.3e} (bar 4 x)"


# ------------------------------------------------------------------ vit_prepare
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@pytest.mark.parametrize("npix", [300, 224 * 224 * 2])
def test_vit_prepare_u8(gpu, npix):
    """uint8 HWC -> NHWC float32 with a 4th channel of exactly +0: bit-equal to the numpy float32 ((u / 255) - mean) / std (two IEEE divisions)"""
    from domain_rag_amd import ops
    idx = np.arange(npix, dtype=np.int64)
    img = np.stack([(idx * 5 + 1) % 256, (idx * 3 + 101) % 256, (idx * 7 + 33) % 256], -1).astype(np.uint8)
    buf, out = _guarded(npix * 4, gpu)
    ops.vit_prepare(torch.from_numpy(img).to(gpu), out, CLIP_MEAN, CLIP_STD)
    _assert_guards(buf, npix * 4)
    got = out.cpu().view(npix, 4)
    want = (img.astype(F32) / F32(255.0) - np.array(CLIP_MEAN, dtype=F32)) / np.array(CLIP_STD, dtype=F32)
    assert want.dtype == np.float32
    assert torch.equal(_bits(got[:, :3]), _bits(want))
    assert bool((_bits(got[:, 3]) == 0).all())


@pytest.mark.parametrize("B,S", [(3, 7), (2, 224)])
def test_vit_prepare_f32(gpu, B, S):
    """normalised float NCHW -> NHWC float32 with a zero 4th channel: a pure move, bit-equal to img.permute(0, 2, 3, 1)"""
    from domain_rag_amd import ops
    img = _randn((B, 3, S, S), 3, 1.7)
    buf, out = _guarded(B * S * S * 4, gpu)
    ops.vit_prepare(img.to(gpu), out, None, None)
    _assert_guards(buf, B * S * S * 4)
    got = out.cpu().view(B, S, S, 4)
    assert torch.equal(_bits(got[..., :3]), _bits(img.permute(0, 2, 3, 1)))
    assert bool((_bits(got[..., 3]) == 0).all())


# ------------------------------------------------------------------ layernorm_f32
def _ln_rows(rows, D, seed):
    """random rows; from two rows on, row 1 has mean 1e4 against a spread of 1e-2 and (from three on) row 2 is constant"""
    x = _randn((rows, D), seed, 1.5) + 0.3
    if rows >= 2:
        x[1] = 1e4 + 1e-2 * _randn((D,), seed + 1)
    if rows >= 3:
        x[2] = -2.75
    return x


@pytest.mark.parametrize("D", [1, 63, 64, 65, 768, 1000, 1024])
def test_layernorm_f32(gpu, D):
    """rows of 1 / 5 / 8 (four rows per block: a lone row, a ragged and a full last block), dense and with ldx = 3 D + 4, ldy = D + 8 whose gap
    columns must stay untouched; every width class of the 64-lane x 16 register layout (below, at and past one and sixteen rounds)"""
    from domain_rag_amd import ops
    g, b = _randn((D,), 1) * 0.5 + 1.0, _randn((D,), 2) * 0.2
    for rows in (1, 5, 8):
        x = _ln_rows(rows, D, 10 + rows)
        ref = F.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-5)
        t32 = F.layer_norm(x, (D,), g, b, 1e-5)
        for ldx, ldy in ((D, D), (3 * D + 4, D + 8)):
            xs = torch.full((rows, ldx), 7.0)
            xs[:, :D] = x
            buf, y = _guarded(rows * ldy, gpu)
            ops.layernorm_f32(xs.to(gpu), y, g.to(gpu), b.to(gpu), rows, D, 1e-5, ldx=ldx, ldy=ldy)
            _assert_guards(buf, rows * ldy)
            got = y.cpu().view(rows, ldy)
            if ldy > D:
                assert _is_sentinel(got[:, D:]), "a gap column was written"
            _check_ratio(f"layernorm_f32 D={D} rows={rows} ldx={ldx}", got[:, :D], ref, t32)


def test_layernorm_f32_rejects_wide_rows(gpu):
    from domain_rag_amd import ops
    D = 1025
    x, y = torch.zeros((2, D), device=gpu), torch.zeros((2, D), device=gpu)
    with pytest.raises(RuntimeError):
        ops.layernorm_f32(x, y, torch.ones(D, device=gpu), torch.zeros(D, device=gpu), 2, D, 1e-5)


# ------------------------------------------------------------------ clip_embed_ln
@pytest.mark.parametrize("B,T,D", [(3, 50, 768), (1, 2, 64), (2, 5, 100)])
def test_clip_embed_ln(gpu, B, T, D):
    """x[b, 0] = ln(cls + pos[0]), x[b, t] = ln(emb[b, t - 1] + pos[t]): the reference builds exactly that (pos indexed by t, a different
    embedding in every batch slot), so a row taken from the wrong source or a pos row indexed by the flat row shows as an O(1) error"""
    from domain_rag_amd import ops
    emb, cls, pos = _randn((B, T - 1, D), 1), _randn((D,), 2), _randn((T, D), 3)
    g, b = _randn((D,), 4) * 0.5 + 1.0, _randn((D,), 5) * 0.2
    buf, x = _guarded(B * T * D, gpu)
    ops.clip_embed_ln(emb.to(gpu), cls.to(gpu), pos.to(gpu), g.to(gpu), b.to(gpu), x, B, T, D, 1e-5)
    _assert_guards(buf, B * T * D)

    def ref_of(dt):
        rows = torch.cat([cls.to(dt).expand(B, 1, D), emb.to(dt)], 1) + pos.to(dt)[None]
        return F.layer_norm(rows, (D,), g.to(dt), b.to(dt), 1e-5)
    _check_ratio(f"clip_embed_ln B={B} T={T} D={D}", x.cpu().view(B, T, D), ref_of(torch.float64), ref_of(torch.float32))


# ------------------------------------------------------------------ linear_f32
# conv2d_f32_kernel tiles 64 pixels x 64 channels (16- or 64-channel K steps; its 128 x 128 form needs >= 512 such tiles): N = 40 and K = 36 lie
# below one tile / one step, N = 100 and K = 200 past one and ragged in the last, K = 192 takes the 64-channel step
@pytest.mark.parametrize("M", [1, 50, 197])
@pytest.mark.parametrize("N,K", [(40, 36), (100, 200), (72, 192)])
def test_linear_f32_forms(gpu, M, N, K):
    """y = act(x w^T + bias) + resid: bias alone (dense), QuickGELU with ldx > K, and the residual read from y itself (``resid`` aliases ``y``
    as the CLIP tower's out-projections do) with ldy > N whose gap columns must stay untouched"""
    from domain_rag_amd import ops
    x, w, bias = _randn((M, K), 1), _randn((N, K), 2, K ** -0.5), _randn((N,), 3, 0.3)
    r0 = _randn((M, N), 4)
    dw, db = w.to(gpu), bias.to(gpu)
    for name, ldx, ldy, act, resid in (("bias", K, N, False, False), ("quick_gelu ldx>K", K + 12, N, True, False),
                                       ("resid=y ldy>N", K, N + 8, False, True), ("quick_gelu resid=y", K + 4, N + 4, True, True)):
        xs = torch.full((M, ldx), 7.0)
        xs[:, :K] = x
        buf, y = _guarded(M * ldy, gpu)
        if resid:
            ys = torch.full((M, ldy), 7.0)
            ys[:, :N] = r0
            y.copy_(ys.view(-1).to(gpu))
        ops.linear_f32(xs.to(gpu), dw, y, M, ldx=ldx, ldy=ldy, bias=db, act=ops.CONV_ACT_QUICK_GELU if act else ops.CONV_ACT_NONE,
                       resid=y if resid else None, ld_res=ldy if resid else 0)
        _assert_guards(buf, M * ldy)
        got = y.cpu().view(M, ldy)
        if ldy > N:
            assert _is_sentinel(got[:, N:]), "a gap column was written"

        def ref_of(dt):
            v = F.linear(x.to(dt), w.to(dt), bias.to(dt))
            if act:
                v = v * torch.sigmoid(1.702 * v)
            return v + r0.to(dt) if resid else v
        _check_ratio(f"linear_f32 M={M} N={N} K={K} {name}", got[:, :N], ref_of(torch.float64), ref_of(torch.float32))


# ------------------------------------------------------------------ resnet_stem_style
@pytest.mark.parametrize("H,W", [(33, 47), (64, 64), (225, 130)])
def test_resnet_stem_style(gpu, H, W):
    """conv 7x7/2 + folded BatchNorm + ReLU + maxpool 3x3/2 + channel mean | unbiased std, two different images: pooled maps of 9 x 12, 16 x 16
    and 57 x 33 (ragged against the kernel's 8 x 8 tile in one, neither and both directions; odd input sizes)"""
    from domain_rag_amd import ops
    from domain_rag_amd.retrieval import StemStyle
    from oracle import stem as ostem
    st = StemStyle(None, gpu, seed=4)
    img = torch.rand((2, 3, H, W), generator=torch.Generator().manual_seed(H))
    img[1] = img[1] * 0.5 + 0.25 * torch.linspace(0, 1, W)
    got = ops.resnet_stem_style(img.to(gpu), st.w, st.scale, st.shift, 1e-5)
    assert got.shape == (2, 128)
    ref = ostem.style_vector(img.double(), {k: v.double() for k, v in st.state.items()})
    t32 = ostem.style_vector(img, st.state)
    _check_ratio(f"resnet_stem_style {H}x{W}", got, ref, t32)
