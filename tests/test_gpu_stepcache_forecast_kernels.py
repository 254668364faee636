"""``ops.stepcache_forecast_images`` (``drag_stepcache_forecast_images_bf16``, csrc/stepcache.hip), called directly: the first-order forecast
of a reused step, per element ``x <- bf16(f32(x) + (c * (f32(r) - f32(p)) + f32(r)))`` in four individually rounded float32 operations.

Everything is compared BIT FOR BIT with the numpy float32 restatement (tests/helpers/stepcache_forecast_ref.py: numpy cannot fuse the
multiply into the add, so a contracted FMA in the kernel shows as a differing bit), NaN by position.  As in
tests/test_gpu_stepcache_image_kernels.py (its frame is copied here: that file may change), every operand is a slice of a sentinel-filled
buffer (bf16 7.0) with 256 guard elements on both sides, and ``x`` is the image-row part of a joint [B, text + rows, cols] buffer whose
text rows hold the sentinel too: ``x`` may change in the listed images' rows only, and ``r``, ``p``, every guard and every gap not at all.

One test is not bit for bit: on residuals that are linear in t the forecast must land at least 8 times nearer the true step than the
plain reuse does (the bound is the issue's; on the CPU restatement the two errors are 0.0055 and 0.102, a factor of 18)."""
import ctypes
import itertools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import stepcache_forecast_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 7.0
COEFS = [1.0, 0.5, -0.75, 3.0, 0.0, 1.0 / 3.0]          # 1/3 is not representable: the float32 the wrapper passes is what the helper uses
LISTS = [[0], [3], [0, 1, 2, 3], [0, 3], [1, 3]]          # B = 4: single (first, last), all, first + last, non-contiguous


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _sent_bits():
    return _bits(torch.full((1,), SENT, dtype=torch.bfloat16)).item()


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.bfloat16, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _assert_guards(buf, n, what):
    b, s = _bits(buf), _sent_bits()
    assert bool((b[:GUARD] == s).all()), f"{what}: guard before the buffer was written"
    assert bool((b[GUARD + n:] == s).all()), f"{what}: guard after the buffer was written"


def _randn_bf(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).bfloat16()


class _Joint:
    """a joint [B, T + rows, cols] buffer with sentinel text rows; x = its flat view from the first image row on; r, p dense and guarded"""

    def __init__(self, B, rows, cols, T, dev, x_host=None, r_host=None, p_host=None):
        self.B, self.rows, self.cols, self.T, self.dev = B, rows, cols, T, dev
        self.stride = (T + rows) * cols
        self.x_host = _randn_bf((B, rows, cols), 1) if x_host is None else x_host
        self.r_host = _randn_bf((B, rows, cols), 5) if r_host is None else r_host
        self.p_host = _randn_bf((B, rows, cols), 6) if p_host is None else p_host
        self.buf, joint = _guarded(B * self.stride, dev)
        self.joint = joint.view(B, T + rows, cols)
        self.joint[:, T:] = self.x_host.to(dev)
        self.x = joint[T * cols:]
        self.rbuf, self.r = self._dense(self.r_host)
        self.pbuf, self.p = self._dense(self.p_host)

    def _dense(self, host):
        buf, v = _guarded(host.numel(), self.dev)
        v.copy_(host.reshape(-1).to(self.dev))
        return buf, v

    def args(self):
        return self.B, self.rows, self.cols, self.stride

    def x_now(self):
        return self.joint[:, self.T:].cpu()

    def assert_frame(self, what):
        n = self.B * self.rows * self.cols
        _assert_guards(self.buf, self.B * self.stride, what + ": joint buffer")
        _assert_guards(self.rbuf, n, what + ": r")
        _assert_guards(self.pbuf, n, what + ": p")
        if self.T:
            assert bool((_bits(self.joint[:, :self.T]) == _sent_bits()).all()), f"{what}: a gap row of the joint buffer was written"
        assert torch.equal(_bits(self.r), _bits(self.r_host.reshape(-1))), f"{what}: r was written"
        assert torch.equal(_bits(self.p), _bits(self.p_host.reshape(-1))), f"{what}: p was written"

    def assert_untouched(self, what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(self.x_now()), _bits(self.x_host)), f"{what}: x was written"
        self.assert_frame(what)


def _check(c, images, coefs, what):
    """after the call: the listed images hold the helper's bits (NaN by position), every other image its own, the frame is whole"""
    torch.cuda.synchronize()
    got = c.x_now()
    rest = [b for b in range(c.B) if b not in images]
    for b, cf in zip(images, coefs):
        want = ref.forecast(c.x_host[b], c.r_host[b], c.p_host[b], cf)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got[b]), nan), f"{what}: image {b} (c = {cf}): NaN positions differ"
        differ = (_bits(got[b]) != _bits(want)) & ~nan
        assert not bool(differ.any()), f"{what}: image {b} (c = {cf}): {int(differ.sum())} of {want.numel()} elements differ from the float32 restatement"
    assert torch.equal(_bits(got[rest]), _bits(c.x_host[rest])), f"{what}: an image outside the list was written"
    c.assert_frame(what)


@pytest.mark.parametrize("cols", [8, 136])
@pytest.mark.parametrize("T", [0, 3])          # dense, and a batch stride with a gap
def test_bits_of_every_list(gpu, cols, T):
    """every list, each image of a call with its own coefficient; over the lists every coefficient of COEFS is used, with every image"""
    from domain_rag_amd import ops
    used = set()
    for k, images in enumerate(LISTS + [[0, 1, 2, 3]]):
        coefs = [COEFS[(k + i) % len(COEFS)] for i in range(len(images))]
        used.update(coefs)
        c = _Joint(4, 7, cols, T, gpu)
        ops.stepcache_forecast_images(c.x, c.r, c.p, *c.args(), images, coefs)
        _check(c, images, coefs, f"images {images}")
    assert used == set(COEFS)


def test_many_workgroups_per_image_and_a_grid_stride_remainder(gpu):
    """the shape of test_swap_of_many_workgroups_per_image: 70 400 vectors per image, 1024 workgroups per image at the grid cap, so the
    grid-stride loop makes 68 full trips and a partial one"""
    from domain_rag_amd import ops
    c = _Joint(3, 1100, 512, 1, gpu)
    images, coefs = [0, 2], [1.0 / 3.0, -0.75]
    ops.stepcache_forecast_images(c.x, c.r, c.p, *c.args(), images, coefs)
    _check(c, images, coefs, "large forecast")


def _bf_from_bits(bits):
    return torch.tensor([b - 65536 if b >= 32768 else b for b in bits], dtype=torch.int16).view(torch.bfloat16)


def test_special_values(gpu):
    """+-max bf16, the smallest and the largest subnormal of both signs, +-0, +-inf and NaN in every combination over (r, p, x) — r == p, the
    cancelling case, among them — with a positive, a negative, a zero and an inexact coefficient"""
    from domain_rag_amd import ops
    specials = _bf_from_bits([0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x007F, 0x807F, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xC040])
    n = len(specials)
    idx = torch.tensor(list(itertools.product(range(n), repeat=3)))          # n^3 triples
    pad = (-len(idx)) % 8
    idx = torch.cat([idx, idx[:pad]])
    rows, B = len(idx) // 8, 4
    r1, p1, x1 = (specials[idx[:, k]].view(1, rows, 8).expand(B, rows, 8).contiguous() for k in range(3))
    c = _Joint(B, rows, 8, 2, gpu, x_host=x1, r_host=r1, p_host=p1)
    images, coefs = [0, 1, 2, 3], [0.5, -0.75, 0.0, 1.0 / 3.0]
    ops.stepcache_forecast_images(c.x, c.r, c.p, *c.args(), images, coefs)
    _check(c, images, coefs, "special values")
    want = ref.forecast(x1[0], r1[0], p1[0], 0.5)
    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any()) and bool((want == 0).any())          # the cases are really there


def test_linear_residuals_are_forecast(gpu):
    """residuals linear in t, res(t) = bf16(A + t Bc): from res(0.9) and res(0.8) the forecast of the step at t = 0.7 must be at most 1/8 as far
    (rms, float64) from x0 + A + 0.7 Bc as the plain reuse of res(0.8) is"""
    from domain_rag_amd import ops
    from domain_rag_amd.step_cache import forecast_coefficient
    B, rows, cols = 4, 24, 64
    g = torch.Generator().manual_seed(0)
    A = torch.randn((B, rows, cols), generator=g, dtype=torch.float64)
    Bc = torch.randn((B, rows, cols), generator=g, dtype=torch.float64)
    x0 = torch.randn((B, rows, cols), generator=g, dtype=torch.float64).bfloat16()
    t_prev, t_last, t_now = 0.9, 0.8, 0.7

    def res(t):
        return (A + t * Bc).bfloat16()
    truth = x0.double() + A + t_now * Bc
    coef = forecast_coefficient(t_now, t_last, t_prev)
    assert abs(coef - 1.0) < 1e-12
    c = _Joint(B, rows, cols, 3, gpu, x_host=x0, r_host=res(t_last), p_host=res(t_prev))
    ops.stepcache_forecast_images(c.x, c.r, c.p, *c.args(), list(range(B)), [coef] * B)
    _check(c, list(range(B)), [coef] * B, "linear residuals")
    forecast = c.x_now().double()
    c = _Joint(B, rows, cols, 3, gpu, x_host=x0, r_host=res(t_last), p_host=res(t_prev))
    ops.stepcache_apply(c.x, c.r, *c.args(), +1)
    torch.cuda.synchronize()
    reuse = c.x_now().double()
    e1, e0 = ((v - truth).pow(2).mean().sqrt().item() for v in (forecast, reuse))
    print(f"rms distance from the true step: forecast {e1:.4e}, plain reuse {e0:.4e}, ratio {e0 / e1:.1f}")
    assert e1 <= e0 / 8


def test_refused_calls_launch_nothing(gpu):
    from domain_rag_amd import _lib, ops
    c = _Joint(5, 7, 136, 3, gpu)
    B, rows, cols, stride = c.args()
    name = "drag_stepcache_forecast_images_bf16"

    def call(x=c.x, r=c.r, p=c.p, cols=cols, lst=(0, 3), coefs=None):
        ops.stepcache_forecast_images(x, r, p, B, rows, cols, stride, lst, [0.5] * len(lst) if coefs is None else coefs)
    bad = [dict(cols=12),                                         # cols % 8 != 0
           dict(x=c.x[4:]),                                       # a pointer that is 8-byte but not 16-byte aligned
           dict(lst=(0, B)), dict(lst=(-1,)),                     # out of range
           dict(lst=(3, 1)), dict(lst=(1, 1)),                    # not strictly increasing
           dict(lst=tuple(range(65))),                            # 65 entries
           dict(coefs=[0.5, math.nan]), dict(coefs=[math.inf, 0.5]), dict(coefs=[0.5, -math.inf]), dict(coefs=[1e39, 0.5])]      # 1e39 is inf as float32
    for kw in bad:
        with pytest.raises(RuntimeError, match=name):
            call(**kw)
        c.assert_untouched(f"refused call {sorted(kw)}")
    # null pointers: only the library can be handed one
    lib, two, half = _lib.load(), (ctypes.c_int32 * 2)(0, 1), (ctypes.c_float * 2)(0.5, 0.5)
    xp, rp, pp = (ctypes.c_void_p(t.data_ptr()) for t in (c.x, c.r, c.p))
    assert lib.drag_stepcache_forecast_images_bf16(xp, rp, None, B, rows, cols, stride, two, half, 2, None) == -1
    assert name in lib.drag_last_error().decode()
    assert lib.drag_stepcache_forecast_images_bf16(None, rp, pp, B, rows, cols, stride, two, half, 2, None) == -1
    assert lib.drag_stepcache_forecast_images_bf16(xp, None, pp, B, rows, cols, stride, two, half, 2, None) == -1
    assert lib.drag_stepcache_forecast_images_bf16(xp, rp, pp, B, rows, cols, stride, None, half, 2, None) == -1
    assert lib.drag_stepcache_forecast_images_bf16(xp, rp, pp, B, rows, cols, stride, two, None, 2, None) == -1
    assert lib.drag_stepcache_forecast_images_bf16(xp, rp, pp, B, rows, cols, rows * cols - 8, two, half, 2, None) == -1      # a batch stride shorter than an image
    for rq, pq in ((c.r.data_ptr() + 8, c.p.data_ptr()), (c.r.data_ptr(), c.p.data_ptr() + 8)):      # r, p 8-byte but not 16-byte aligned
        assert lib.drag_stepcache_forecast_images_bf16(xp, ctypes.c_void_p(rq), ctypes.c_void_p(pq), B, rows, cols, stride, two, half, 2, None) == -1
    c.assert_untouched("null and misaligned pointers")
    # an empty list is a successful no-op
    assert lib.drag_stepcache_forecast_images_bf16(xp, rp, pp, B, rows, cols, stride, two, half, 0, None) == 0
    call(lst=())
    c.assert_untouched("empty list")
    # the wrapper refuses a CPU tensor, an operand too small for the addressing and a coefficient list of another length
    with pytest.raises(RuntimeError, match="GPU"):
        call(p=c.p.cpu())
    with pytest.raises(ValueError):
        call(p=c.p[: c.p.numel() - 8])
    with pytest.raises(ValueError, match="coefficients"):
        call(coefs=[0.5])
    c.assert_untouched("wrapper refusals")
