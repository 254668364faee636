"""The bf16 / uint8 glue kernels of csrc/vae.hip and csrc/elementwise.hip (and patchify_f32 of csrc/stem.hip), each called directly.

What every test here does:
  * outputs and in-place operands are slices of a larger buffer filled with a sentinel (bf16 7.0, uint8 0xAB), with >= 256 guard elements
    on both sides and every gap column between ``cols`` and ``ld`` holding the sentinel too; after the call every guard and gap element
    must hold the sentinel bit for bit (a stray write shows);
  * one case per grid-stride kernel has more elements than the launch's grid cap x 256 (4096 blocks in csrc/vae.hip and patchify_f32, 2048
    in csrc/elementwise.hip) plus a ragged tail, so the second trip through ``for (i = ...; i < total; i += gridDim.x * 256)`` runs;
  * results are compared bit for bit with a numpy float32 restatement of the kernel's expression wherever every operation of it is an IEEE
    float32 operation (the build's ``-ffp-contract=on`` only fuses a * b + c where a * b is exact in the cases below, which is noted where it
    matters); otherwise against float64 with a bound derived in the test's docstring."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256
F32 = np.float32


# ------------------------------------------------------------------ helpers
def _rbf(a):
    """float32 ndarray -> the nearest bf16 (ties to even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _bits(t):
    """bit patterns of a bf16 / float32 tensor or ndarray"""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _bf_bits(a):
    """bit patterns of float32 values that are exact bf16 numbers"""
    return _bits(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16())


def _sentinel(dtype):
    return 0xAB if dtype == torch.uint8 else 7.0


def _guarded(n, dtype, dev):
    """(buffer, view): ``view`` = n elements of ``dtype`` with GUARD sentinel elements before and after, all n pre-filled with the sentinel"""
    buf = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _assert_guards(buf, n):
    b = buf.cpu()
    s = torch.full((1,), _sentinel(b.dtype), dtype=b.dtype)
    assert torch.equal(_bits(b[:GUARD]), _bits(s).expand(GUARD)), "guard before the buffer was written"
    assert torch.equal(_bits(b[GUARD + n:]), _bits(s).expand(GUARD)), "guard after the buffer was written"


def _assert_sentinel(t, what):
    t = t.cpu().contiguous()
    s = torch.full((1,), _sentinel(t.dtype), dtype=t.dtype)
    assert bool((_bits(t) == _bits(s)).all()), f"{what} was written"


def _randn_bf(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def _ulp_bf(a):
    """spacing of bf16 at magnitude |a| (float64 ndarray; 0 at 0): 2^(floor(log2 |a|) - 7)"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    _, e = np.frexp(a)
    return np.where(a == 0, 0.0, np.ldexp(1.0, e - 8))


def _rbf64(a):
    """float64 -> nearest bf16 (ties to even) in ONE rounding, as float64 (normal range)"""
    a = np.asarray(a, dtype=np.float64)
    q = _ulp_bf(a)
    return np.where(a == 0, 0.0, np.rint(a / np.where(q == 0, 1.0, q)) * q)


# ------------------------------------------------------------------ image_preprocess
def _pre_expected(img, mask):
    """numpy float32 restatement of image_preprocess_kernel: (2 * (u / 255) - 1) * keep, keep = (m / 255 < 0.5).  2 * q is exact, so the fused
    multiply-add the compiler may form gives the bits of the separate operations."""
    q = img.astype(F32) / F32(255.0)
    v = F32(2.0) * q - F32(1.0)
    if mask is not None:
        keep = np.where(mask.astype(F32) / F32(255.0) < F32(0.5), F32(1.0), F32(0.0))
        v = v * keep[..., None]
    return _rbf(v)


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 8), (1, 1025, 1024, 4)])
@pytest.mark.parametrize("masked", [False, True])
def test_image_preprocess(gpu, B, H, W, C, masked):
    """every byte value in every channel (the large image; the small one holds the 70 its pixels have room for) under a mask of the six bytes
    around the binarise threshold and the ends of the range: bit-equal to the float32 expression and to the oracle's preprocess; the halo
    ring and channels 3.. keep what the buffer held.  1025 x 1024 pixels = 4096 x 256 + 1024: the second trip of the loop."""
    from domain_rag_amd import ops
    from oracle import vae as ov
    idx = np.arange(B * H * W, dtype=np.int64).reshape(B, H, W)
    img = np.stack([(idx * 1 + 0) % 256, (idx * 3 + 85) % 256, (idx * 7 + 170) % 256], -1).astype(np.uint8)
    mvals = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
    mask = mvals[(idx // 3 + idx // 256) % 6] if masked else None          # every (byte, mask value) pair meets in the large image
    if B * H * W >= 256 * 6:
        assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    n = B * (H + 2) * (W + 2) * C
    buf, y = _guarded(n, torch.bfloat16, gpu)
    ops.image_preprocess(torch.from_numpy(img).to(gpu), torch.from_numpy(mask).to(gpu) if masked else None, y, B, H, W, C)
    _assert_guards(buf, n)
    got = y.cpu().view(B, H + 2, W + 2, C)
    want = _pre_expected(img, mask)
    assert torch.equal(_bits(got[:, 1:-1, 1:-1, :3]), _bf_bits(want))
    timg, tmask = torch.from_numpy(img), (torch.from_numpy(mask) if masked else None)
    ref = ov.preprocess_image(timg)
    if masked:
        ref = ref * (1 - ov.preprocess_mask(tmask))
    assert torch.equal(_bits(got[:, 1:-1, 1:-1, :3]), _bits(ref.permute(0, 2, 3, 1).bfloat16()))
    _assert_sentinel(got[:, 1:-1, 1:-1, 3:], "a channel past the third")
    for ring, name in ((got[:, 0], "top"), (got[:, -1], "bottom"), (got[:, :, 0], "left"), (got[:, :, -1], "right")):
        _assert_sentinel(ring, f"the {name} halo")
    if masked:      # the threshold itself: 127 keeps, 128 blanks
        inner = got[:, 1:-1, 1:-1, :3].float()
        assert bool((inner[torch.from_numpy(mask >= 128)] == 0).all())
        assert torch.equal(_bits(inner[torch.from_numpy(mask <= 127)].bfloat16()), _bf_bits(_pre_expected(img, None)[mask <= 127]))


# ------------------------------------------------------------------ image_postprocess
def _post_expected(x):
    """numpy float32 restatement of image_postprocess_kernel on float32 values x: v = bf16(x * 0.5 + 0.5) (x * 0.5 is exact: one rounding with or
    without the fused form), clamp to [0, 1], rint(v * 255).  NaN positions hold 0 here and are left out by the caller."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = _rbf(x * F32(0.5) + F32(0.5))
        v = np.minimum(np.maximum(v, F32(0.0)), F32(1.0))
        r = np.rint(v * F32(255.0))
    return np.where(np.isnan(r), 0, r).astype(np.uint8)


@pytest.mark.parametrize("ld", [3, 8])
def test_image_postprocess_every_bf16_value(gpu, ld):
    """all 65 536 bf16 bit patterns as x (21 846 pixels of 3 channels, the last two values 0): bit-equal bytes for every finite and infinite
    input; NaN inputs are in the data and left out of the comparison (the C conversion of NaN to uint8 is unspecified), so their neighbours are
    still checked.  ld = 8: the channels past the third hold a sentinel and are not read into the result."""
    from domain_rag_amd import ops
    npix = 21846
    pat = torch.zeros(npix * 3, dtype=torch.int32)
    pat[:65536] = torch.arange(65536, dtype=torch.int32)
    xb = pat.to(torch.int16).view(torch.bfloat16).view(npix, 3)
    x = torch.full((npix, ld), 7.0, dtype=torch.bfloat16)
    x[:, :3] = xb
    buf, out = _guarded(npix * 3, torch.uint8, gpu)
    ops.image_postprocess(x.to(gpu), out, npix, ld)
    _assert_guards(buf, npix * 3)
    xf = xb.float().numpy()
    want = _post_expected(xf)
    ok = ~np.isnan(xf)
    assert (~ok).sum() > 200 and ok.sum() > 65000
    got = out.cpu().numpy().reshape(npix, 3)
    assert np.array_equal(got[ok], want[ok])
    assert got[np.isposinf(xf)].tolist() == [255] and got[np.isneginf(xf)].tolist() == [0]


def test_image_postprocess_second_trip(gpu):
    """npix = 4096 x 256 + 77 rows of ld = 4: the loop's second trip and its ragged end"""
    from domain_rag_amd import ops
    npix, ld = 1048576 + 77, 4
    x = _randn_bf((npix, ld), 11, 1.5)
    buf, out = _guarded(npix * 3, torch.uint8, gpu)
    ops.image_postprocess(x.to(gpu), out, npix, ld)
    _assert_guards(buf, npix * 3)
    assert np.array_equal(out.cpu().numpy().reshape(npix, 3), _post_expected(x[:, :3].float().numpy()))


# ------------------------------------------------------------------ mask_pack
@pytest.mark.parametrize("B,H,W,ld", [(2, 32, 48, 256), (2, 32, 48, 320), (1, 1040, 1024, 256)])
def test_mask_pack_every_byte(gpu, B, H, W, ld):
    """a mask of all 256 byte values (127 -> 0, 128 -> 1 exactly): bit-equal to the oracle's pack_mask(preprocess_mask(.)); ld = 320 leaves 64
    gap columns per token that must stay untouched; 1040 x 1024 = 4096 x 256 + 16 384 elements: the second trip"""
    from domain_rag_amd import ops
    from oracle import vae as ov
    idx = np.arange(B * H * W, dtype=np.int64).reshape(B, H, W)
    mask = torch.from_numpy(((idx * 37 + idx // W) % 256).astype(np.uint8))
    assert len(torch.unique(mask)) == 256
    rows = B * (H // 16) * (W // 16)
    buf, tok = _guarded(rows * ld, torch.bfloat16, gpu)
    ops.mask_pack(mask.to(gpu), tok, B, H, W, ld)
    _assert_guards(buf, rows * ld)
    got = tok.cpu().view(rows, ld)
    want = ov.pack_mask(ov.preprocess_mask(mask)).reshape(rows, 256)
    assert torch.equal(_bits(got[:, :256]), _bits(want.bfloat16()))
    if ld > 256:
        _assert_sentinel(got[:, 256:], "a gap column")
    # the threshold, stated without the oracle: byte 127 packs to 0, byte 128 to 1
    m01 = (mask >= 128).float()[:, None]
    assert torch.equal(got[:, :256].float(), ov.pack_mask(m01).reshape(rows, 256))


# ------------------------------------------------------------------ unpack_latents
@pytest.mark.parametrize("B,h,w,C,ld", [(2, 3, 5, 64, 64), (2, 3, 5, 64, 128), (1, 129, 128, 16, 64)])
def test_unpack_latents(gpu, B, h, w, C, ld):
    """tokens -> haloed NHWC latents: bit-equal to the float32 restatement rbf(rbf(tok * (1 / scaling)) + shift) (no a * b + c in it), within
    1 bf16 ulp of the oracle (torch-CPU rounds the scalar shift to bf16 before the add, the kernel keeps it in float32: the bound of
    tests/test_gpu_vae.py), halo and channels 16.. untouched.  129 x 128 x 64 = 4096 x 256 + 8192: the second trip."""
    from domain_rag_amd import ops
    from oracle import vae as ov
    t = torch.full((B, h * w, ld), 7.0, dtype=torch.bfloat16)
    t[..., :64] = _randn_bf((B, h * w, 64), 9, 1.5)
    n = B * (2 * h + 2) * (2 * w + 2) * C
    buf, y = _guarded(n, torch.bfloat16, gpu)
    ops.unpack_latents(t.to(gpu), y, B, h, w, ld, C, ov.SCALING, ov.SHIFT)
    _assert_guards(buf, n)
    got = y.cpu().view(B, 2 * h + 2, 2 * w + 2, C)
    tok = t[..., :64].contiguous()
    tf = tok.float().numpy()
    inv = F32(1.0) / F32(ov.SCALING)
    want = _rbf(_rbf(tf * inv) + F32(ov.SHIFT))
    want = ov.unpack_latents(torch.from_numpy(want), h, w)                       # [B, 16, 2h, 2w]: the oracle's layout
    inner = got[:, 1:-1, 1:-1, :16].permute(0, 3, 1, 2)
    assert torch.equal(_bits(inner), _bf_bits(want.numpy()))
    ref = (ov.unpack_latents(tok, h, w) / ov.SCALING + ov.SHIFT).float()
    assert bool(((inner.float() - ref).abs() <= ref.abs() * 2 ** -7 + 1e-3).all())
    _assert_sentinel(got[:, 1:-1, 1:-1, 16:], "a channel past the 16th")
    for ring, name in ((got[:, 0], "top"), (got[:, -1], "bottom"), (got[:, :, 0], "left"), (got[:, :, -1], "right")):
        _assert_sentinel(ring, f"the {name} halo")


# ------------------------------------------------------------------ sample_pack_latents
@pytest.mark.parametrize("B,H,W,ldm,ld", [(2, 6, 10, 32, 64), (2, 6, 10, 64, 80), (1, 258, 256, 32, 64)])
@pytest.mark.parametrize("noisy", [False, True])
def test_sample_pack_latents(gpu, B, H, W, ldm, ld, noisy):
    """tok = rbf(rbf(z - shift) * scaling), z = mean (no noise) or rbf(mean + rbf(stdv * noise)), stdv = rbf(exp(rbf(0.5 * clamp(logvar,
    -30, 20)))), log-variances over [-40, 30] so that both clamps bind.  258 x 256 x 16 = 4096 x 256 + 8192 elements: the second trip.

    Without noise every operation is an IEEE float32 one (no a * b + c): bit-equal to the numpy float32 restatement.

    With noise the one operation that cannot be restated is ``__expf``.  Its error (a few float32 ulp: 2^-16 of a bf16 ulp) can move
    stdv = rbf(exp(.)) by at most one bf16 step against s = rbf64(exp_float64(.)), |d| <= ulp(s).  From there on the kernel computes, with
    r1..r4 its four later bf16 roundings (each of a float32 result: (1 + 2^-15) covers the float32 rounding under the bf16 one),
        tok = (((mean + (s + d) n + r1) + r2) - shift + r3) * scaling + r4,
    so against U = ((mean + s n) - shift) * scaling evaluated in float64
        |tok - U| <= scaling (ulp(s) |n| + |r1| + |r2| + |r3|) + |r4|,      |r_i| <= 1/2 ulp(the value rounded there) (1 + 2^-15),
    each ulp taken at the float64 value of that point plus the error bound accumulated before it (ulp is monotone in the magnitude).
    rbf(0.5 * logvar) is exact (a bf16 number halved).  No constant here is fitted.

    The NCHW quantities are packed into token order by the oracle's pack_latents (f = c * 4 + di * 2 + dj); U itself lies within
    scaling |n| ulp(s) / 2 of the oracle's float64 pack_latents(sample_latents(.)), which does not round s."""
    from domain_rag_amd import ops
    from oracle import vae as ov
    g = torch.Generator().manual_seed(5)
    mean = (torch.randn(B, 16, H, W, generator=g) * 2).bfloat16()
    logvar = (torch.rand(B, 16, H, W, generator=g) * 70 - 40).bfloat16()
    assert logvar.min() < -30 and logvar.max() > 20
    noise = torch.randn(B, 16, H, W, generator=g).bfloat16()
    mom = torch.full((B, H, W, ldm), 7.0, dtype=torch.bfloat16)
    mom[..., :16] = mean.permute(0, 2, 3, 1)
    mom[..., 16:32] = logvar.permute(0, 2, 3, 1)
    rows = B * (H // 2) * (W // 2)
    buf, tok = _guarded(rows * ld, torch.bfloat16, gpu)
    ops.sample_pack_latents(mom.to(gpu), noise.to(gpu) if noisy else None, tok, B, H, W, ldm, ld, ov.SCALING, ov.SHIFT)
    _assert_guards(buf, rows * ld)
    got = tok.cpu().view(rows, ld)
    if ld > 64:
        _assert_sentinel(got[:, 64:], "a gap column")
    got64 = got[:, :64].float().numpy().astype(np.float64)
    sc, sh = float(F32(ov.SCALING)), float(F32(ov.SHIFT))
    pack = lambda a: ov.pack_latents(torch.from_numpy(np.ascontiguousarray(a))).reshape(rows, 64).numpy()
    if not noisy:
        m32 = mean.float().numpy()
        want = _rbf(_rbf(m32 - F32(ov.SHIFT)) * F32(ov.SCALING))
        assert torch.equal(_bits(got[:, :64]), _bf_bits(pack(want)))
        return
    m, n = mean.double().numpy(), noise.double().numpy()
    half = 0.5 * np.clip(logvar.double().numpy(), -30.0, 20.0)
    assert np.array_equal(half, _rbf64(half))                                    # rbf(0.5 * logvar) rounds nothing
    s = _rbf64(np.exp(half))
    eps = 1.0 + 2.0 ** -15
    e0 = _ulp_bf(s) * np.abs(n)                                                  # d n
    r1 = 0.5 * _ulp_bf(np.abs(s * n) + e0) * eps
    r2 = 0.5 * _ulp_bf(np.abs(m + s * n) + e0 + r1) * eps
    r3 = 0.5 * _ulp_bf(np.abs(m + s * n - sh) + e0 + r1 + r2) * eps
    U = (m + s * n - sh) * sc
    r4 = 0.5 * _ulp_bf(np.abs(U) + sc * (e0 + r1 + r2 + r3)) * eps
    bound = sc * (e0 + r1 + r2 + r3) + r4
    err = np.abs(got64 - pack(U))
    worst = float((err / pack(bound)).max())
    print(f"sample_pack_latents noisy B={B} H={H} W={W}: max |tok - U| / bound = {worst:.3f}")
    assert (err <= pack(bound)).all(), worst
    # layout and chain against the oracle itself (float64, s not rounded there)
    mo = torch.cat([mean, logvar], 1).double()
    # (the oracle holds shift and scaling as Python floats, the kernel as float32: (z - sh) sc = (oracle / SCALING + SHIFT - sh) sc)
    oracle = ((ov.pack_latents(ov.sample_latents(mo, noise.double())) / ov.SCALING + ov.SHIFT - sh) * sc).reshape(rows, 64).numpy()
    slack = 1e-12 * (1.0 + np.abs(oracle))                                       # float64 evaluation order
    assert (np.abs(pack(U) - oracle) <= pack(sc * np.abs(n) * 0.5 * _ulp_bf(np.exp(half))) + slack).all()


# ------------------------------------------------------------------ scale_noise_rows / flow_euler_rows
ROW_SHAPES = [(37, 64), (16400, 64)]          # 16 400 x 64 = 4096 x 256 + 1024 elements: the second trip


def _strided(rows, cols, ld, seed, dev):
    """(cpu data [rows, cols], guarded buffer, its [rows, ld] view on ``dev`` with the gap columns holding the sentinel)"""
    data = _randn_bf((rows, cols), seed, 1.5)
    full = torch.full((rows, ld), 7.0, dtype=torch.bfloat16)
    full[:, :cols] = data
    buf, v = _guarded(rows * ld, torch.bfloat16, dev)
    v.copy_(full.view(-1).to(dev))
    return data, buf, v


@pytest.mark.parametrize("rows,cols", ROW_SHAPES)
def test_scale_noise_rows(gpu, rows, cols):
    """x = rbf(rbf(sg * noise) + rbf(om * x)), sg = rbf(sigma), om = rbf(1 - sg), on rows of stride ldx = 96 | 72 (noise dense): both products
    are bf16 x bf16, exact in float32, and are rounded before the add, so the numpy float32 restatement is exact: bit-equal, for sigma at
    both ends, the middle and two schedule values; the gap columns keep the sentinel"""
    from domain_rag_amd import ops
    ldx, ldn = (96 if rows < 1000 else 72), 64
    noise = _randn_bf((rows, ldn), 21)
    nd = noise.to(gpu)
    for sigma in (0.0, 1.0, 0.5, 0.0371, 0.9961):
        x, buf, xv = _strided(rows, cols, ldx, 20, gpu)
        ops.scale_noise_rows(xv, nd, rows, cols, ldx, ldn, sigma)
        _assert_guards(buf, rows * ldx)
        got = xv.cpu().view(rows, ldx)
        _assert_sentinel(got[:, cols:], "a gap column")
        sg = _rbf(np.array([sigma], dtype=F32))[0]
        om = _rbf(np.array([F32(1.0) - sg], dtype=F32))[0]
        want = _rbf(_rbf(sg * noise[:, :cols].float().numpy()) + _rbf(om * x.float().numpy()))
        assert torch.equal(_bits(got[:, :cols]), _bf_bits(want)), sigma


@pytest.mark.parametrize("rows,cols", ROW_SHAPES)
def test_flow_euler_rows(gpu, rows, cols):
    """x += dt * v on rows of stride ldx = 96 | 72, v of stride 80.  The kernel's x + a * v is a fused multiply-add (-ffp-contract=on): one
    rounding of the exact value to float32, then one to bf16 — the reference is float64 x + a v (a v is exact there) rounded to float32 and
    then to bf16, and the result may sit at most 1 bf16 ulp from it (float64's own rounding of the sum before the float32 one).  It must also
    have the bits of ops.flow_euler_step on the same data laid out densely: the two kernels state the same expression."""
    from domain_rag_amd import ops
    ldx, ldv = (96 if rows < 1000 else 72), 80
    for dt in (-0.0371, 0.25, -1.0):
        x, buf, xv = _strided(rows, cols, ldx, 30, gpu)
        v, _, vv = _strided(rows, cols, ldv, 31, gpu)
        ops.flow_euler_rows(xv, vv, rows, cols, ldx, ldv, dt)
        _assert_guards(buf, rows * ldx)
        got = xv.cpu().view(rows, ldx)
        _assert_sentinel(got[:, cols:], "a gap column")
        ref64 = x.double().numpy() + float(F32(dt)) * v.double().numpy()
        ref = torch.from_numpy(ref64).float().bfloat16().double().numpy()
        assert (np.abs(got[:, :cols].double().numpy() - ref) <= _ulp_bf(ref)).all(), dt
        dense = x.clone().to(gpu)
        ops.flow_euler_step(dense, v.contiguous().to(gpu), dt)
        assert torch.equal(_bits(got[:, :cols]), _bits(dense)), dt


# ------------------------------------------------------------------ patchify / patchify_f32
NORMS = [((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),      # CLIP
         ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),                                                # SigLIP
         ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]                                    # ImageNet


def _unfold(x, P, ldo):
    """NCHW [B, 3, H, W] -> patch rows [B * gh * gw, ldo], k = c * P * P + py * P + px, trailing pixels dropped, columns >= 3 P P zero"""
    B, _, H, W = x.shape
    gh, gw = H // P, W // P
    r = x[:, :, :gh * P, :gw * P].reshape(B, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 3 * P * P)
    out = torch.zeros((B * gh * gw, ldo), dtype=x.dtype)
    out[:, :3 * P * P] = r
    return out


# (B, H, W, P, ldo): 45 / 14 drops three trailing pixels and pads K 588 -> 640; 406 / 14: 841 rows x 640 = 2048 x 256 + 13 952 elements
PATCH_GEOMS = [(2, 45, 45, 14, 640), (2, 32, 48, 16, 768), (1, 406, 406, 14, 640)]


@pytest.mark.parametrize("B,H,W,P,ldo", PATCH_GEOMS)
def test_patchify_u8(gpu, B, H, W, P, ldo):
    """uint8 image -> normalised bf16 patch rows: bit-equal to the numpy float32 ((u / 255) - mean) / std (two IEEE divisions, no a * b + c)
    rounded to bf16, for every byte value under three mean / std sets, and to the oracle's normalize_u8 unfolded; the K padding is zeros"""
    from domain_rag_amd import ops
    from oracle import vit as ovit
    idx = np.arange(B * H * W, dtype=np.int64).reshape(B, H, W)
    img = np.stack([(idx * 5 + 1) % 256, (idx * 3 + 101) % 256, (idx * 7 + 33) % 256], -1).astype(np.uint8)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    rows = B * (H // P) * (W // P)
    d_img = torch.from_numpy(img).to(gpu)
    for mean, std in (NORMS if rows < 100 else NORMS[:1]):
        buf, out = _guarded(rows * ldo, torch.bfloat16, gpu)
        ops.patchify(d_img, out, B, H, W, P, ldo, mean, std)
        _assert_guards(buf, rows * ldo)
        got = out.cpu().view(rows, ldo)
        m, s = np.array(mean, dtype=F32), np.array(std, dtype=F32)
        v = (img.astype(F32) / F32(255.0) - m) / s
        want = _unfold(torch.from_numpy(_rbf(v)).permute(0, 3, 1, 2), P, ldo)
        assert torch.equal(_bits(got), _bf_bits(want.numpy()))
        ref = _unfold(ovit.normalize_u8(torch.from_numpy(img), mean, std).bfloat16(), P, ldo)
        assert torch.equal(_bits(got), _bits(ref))
        if ldo > 3 * P * P:
            assert bool((_bits(got[:, 3 * P * P:]) == 0).all())          # +0.0, not -0.0 or the sentinel


@pytest.mark.parametrize("B,H,W,P,ldo", PATCH_GEOMS + [(7, 224, 224, 32, 3072)])     # 343 rows x 3072 = 4096 x 256 + 5120 elements
def test_patchify_f32(gpu, B, H, W, P, ldo):
    """normalised float NCHW -> bf16 patch rows: bit-equal to img.bfloat16() unfolded"""
    from domain_rag_amd import ops
    img = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(40)) * 1.7
    rows = B * (H // P) * (W // P)
    buf, out = _guarded(rows * ldo, torch.bfloat16, gpu)
    ops.patchify_f32(img.to(gpu), out, B, H, W, P, ldo)
    _assert_guards(buf, rows * ldo)
    assert torch.equal(_bits(out.cpu().view(rows, ldo)), _bits(_unfold(img.bfloat16(), P, ldo)))


# ------------------------------------------------------------------ scale_sum
@pytest.mark.parametrize("G,N,elems", [(2, 3, 1001), (2, 2, 262200), (3, 1, 777)])      # 2 x 262 200 = 2048 x 256 + 112 elements
def test_scale_sum(gpu, G, N, elems):
    """out[g] = rbf(sum_n rbf(rbf(scale[g, n]) * x[g, n])) with a float32 accumulator and n ascending: each product is bf16 x bf16 (exact in
    float32) and rounded before it is added, so the numpy float32 restatement is exact: bit-equal"""
    from domain_rag_amd import ops
    x = _randn_bf((G, N, elems), 50, 2.0)
    scales = torch.randn(G * N, generator=torch.Generator().manual_seed(51)) * 1.3
    buf, out = _guarded(G * elems, torch.bfloat16, gpu)
    ops.scale_sum(x.to(gpu), scales.to(gpu), out, G, N, elems)
    _assert_guards(buf, G * elems)
    s = _rbf(scales.numpy()).reshape(G, N)
    xf = x.float().numpy()
    acc = np.zeros((G, elems), dtype=F32)
    for n in range(N):
        acc = acc + _rbf(s[:, n, None] * xf[:, n])
    assert acc.dtype == np.float32
    assert torch.equal(_bits(out.cpu().view(G, elems)), _bf_bits(_rbf(acc)))
