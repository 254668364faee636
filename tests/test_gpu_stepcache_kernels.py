"""The two kernels of csrc/stepcache.hip (``ops.stepcache_delta``, ``ops.stepcache_apply``), each called directly.

As in tests/test_gpu_glue_kernels.py, every operand a kernel writes is a slice of a sentinel-filled buffer (bf16 7.0) with 256 guard
elements on both sides; ``x`` is the image-row part of a joint [B, text + rows, cols] buffer whose text rows (the gap rows between two
images) hold the sentinel too.  After a call every guard and gap element must hold the sentinel bit for bit.

The element-wise results are single IEEE float32 operations followed by one round-to-nearest-even to bf16: compared bit for bit with the
torch expression.  The ratios are float64 sums of exactly representable terms (bf16 -> float64 is exact, so is the difference of two bf16
numbers): only the order of summation is free, which bounds the relative difference from a float64 torch evaluation by N * 2^-53 for N
terms of one sign — 1.2e-10 for the largest N here (4096 x 256), so the bar of 1e-9 has a factor of a few in hand."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 7.0
# (B, rows_per_batch, cols, leading text rows)
SHAPES = [(1, 1, 128, 0),           # smallest
          (2, 5, 128, 3),           # batch stride > rows * cols
          (3, 333, 256, 7),         # neither a multiple of a workgroup's chunk (256 x 8 elements) nor of 64 rows
          (2, 4096, 256, 24)]       # many workgroups (512 per image) and partial sums: the second stage's lanes add 8 partials each
SHAPES.append((8, 1100, 512, 1))    # beyond the issue's table: 70 400 vectors per image over 256 workgroups x 256 lanes — the grid-stride loop's second trip
RTOL = 1e-9


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.bfloat16, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _assert_guards(buf, n, what):
    b = _bits(buf)
    s = _bits(torch.full((1,), SENT, dtype=torch.bfloat16)).item()
    assert bool((b[:GUARD] == s).all()), f"{what}: guard before the buffer was written"
    assert bool((b[GUARD + n:] == s).all()), f"{what}: guard after the buffer was written"


def _randn_bf(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


class _Case:
    """device operands of one shape: the joint buffer with sentinel text rows, x = its flat view from the first image row on"""

    def __init__(self, shape, dev, seed=0):
        self.B, self.rows, self.cols, self.T = B, rows, cols, T = shape
        self.dev = dev
        self.stride = (T + rows) * cols
        self.x_host = _randn_bf((B, rows, cols), seed + 1)
        self.joint_buf, joint = _guarded(B * self.stride, dev)
        self.joint = joint.view(B, T + rows, cols)
        self.joint[:, T:] = self.x_host.to(dev)
        self.x = joint[T * cols:]

    def dense(self, host):
        buf, v = _guarded(host.numel(), self.dev)
        v.copy_(host.reshape(-1).to(self.dev))
        return buf, v

    def args(self):
        return self.B, self.rows, self.cols, self.stride

    def assert_joint_frame(self, what):
        """guards and text (gap) rows of the joint buffer still hold the sentinel"""
        _assert_guards(self.joint_buf, self.B * self.stride, what + ": joint buffer")
        if self.T:
            s = _bits(torch.full((1,), SENT, dtype=torch.bfloat16)).item()
            assert bool((_bits(self.joint[:, :self.T]) == s).all()), f"{what}: a text (gap) row of the joint buffer was written"

    def x_now(self):
        return self.joint[:, self.T:].cpu()


def _ratio_ref(e_bf16, f_bf16):
    """float64 torch evaluation over the stored values, per image"""
    e, f = e_bf16.double(), f_bf16.double()
    B = e.shape[0]
    num, den = (e - f).abs().reshape(B, -1).sum(1), f.abs().reshape(B, -1).sum(1)
    return [(n / d).item() if d.item() != 0 or math.isnan(n.item()) else math.inf for n, d in zip(num, den)]


def _ws(c):
    from domain_rag_amd import ops
    nbytes = ops.stepcache_workspace_bytes(c.B, c.rows, c.cols)
    assert nbytes >= 16 * c.B and nbytes % 16 == 0
    return torch.empty(nbytes, dtype=torch.uint8, device=c.dev)


@pytest.mark.parametrize("shape", SHAPES)
def test_delta_bits_ratio_and_frame(gpu, shape):
    from domain_rag_amd import ops
    c = _Case(shape, gpu)
    n = c.B * c.rows * c.cols
    e0, f0 = _randn_bf((c.B, c.rows, c.cols), 2), _randn_bf((c.B, c.rows, c.cols), 3, 0.7)
    want_e = (c.x_host.float() - e0.float()).bfloat16()
    want_r = _ratio_ref(want_e, f0)
    got = []
    for run in range(2):
        ebuf, e = c.dense(e0)
        fbuf, f = c.dense(f0)
        ratios = torch.full((c.B + 2,), -3.0, dtype=torch.float64, device=gpu)
        ops.stepcache_delta(c.x, e, f, ratios[1:], _ws(c), *c.args())
        torch.cuda.synchronize()
        assert torch.equal(_bits(e), _bits(want_e.reshape(-1))), "e after the delta"
        assert torch.equal(_bits(f), _bits(f0.reshape(-1))), "f was written"
        assert torch.equal(_bits(c.x_now()), _bits(c.x_host)), "x was written"
        _assert_guards(ebuf, n, "e"); _assert_guards(fbuf, n, "f"); c.assert_joint_frame("delta")
        r = ratios.cpu()
        assert r[0].item() == -3.0 and r[-1].item() == -3.0, "a ratio outside [0, B) was written"
        got.append(r[1:-1].clone())
    for b in range(c.B):
        print(f"{shape} image {b}: ratio {got[0][b].item():.17g}, float64 torch {want_r[b]:.17g}, rel {abs(got[0][b].item() - want_r[b]) / want_r[b]:.3e}")
        assert abs(got[0][b].item() - want_r[b]) <= RTOL * want_r[b]
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), "two runs gave different 64-bit ratios"


@pytest.mark.parametrize("shape", SHAPES)
def test_apply_both_forms(gpu, shape):
    from domain_rag_amd import ops
    c = _Case(shape, gpu)
    n = c.B * c.rows * c.cols
    r0 = _randn_bf((c.B, c.rows, c.cols), 5)
    # sign = +1: x <- bf16(x + r), r untouched
    rbuf, r = c.dense(r0)
    ops.stepcache_apply(c.x, r, *c.args(), +1)
    torch.cuda.synchronize()
    want_x = (c.x_host.float() + r0.float()).bfloat16()
    assert torch.equal(_bits(c.x_now()), _bits(want_x)), "x after apply(+1)"
    assert torch.equal(_bits(r), _bits(r0.reshape(-1))), "r was written by apply(+1)"
    _assert_guards(rbuf, n, "r"); c.assert_joint_frame("apply +1")
    # sign = -1, the capture form: r <- bf16(x - r), x untouched
    ops.stepcache_apply(c.x, r, *c.args(), -1)
    torch.cuda.synchronize()
    want_r = (want_x.float() - r0.float()).bfloat16()
    assert torch.equal(_bits(r), _bits(want_r.reshape(-1))), "r after apply(-1)"
    assert torch.equal(_bits(c.x_now()), _bits(want_x)), "x was written by apply(-1)"
    _assert_guards(rbuf, n, "r"); c.assert_joint_frame("apply -1")


def test_zero_f_gives_inf_and_nan_stays_in_its_image(gpu):
    from domain_rag_amd import ops
    c = _Case(SHAPES[2], gpu)
    e0 = _randn_bf((c.B, c.rows, c.cols), 2)
    f0 = _randn_bf((c.B, c.rows, c.cols), 3)
    _, e = c.dense(e0)
    _, f = c.dense(torch.zeros_like(f0))
    ratios = torch.zeros(c.B, dtype=torch.float64, device=gpu)
    ops.stepcache_delta(c.x, e, f, ratios, _ws(c), *c.args())
    assert all(v == math.inf for v in ratios.cpu().tolist()), ratios
    # one NaN in image 1 of x: that image's ratio is NaN, the others' are what they are without it
    c.joint[1, c.T + 17, 33] = float("nan")
    _, e = c.dense(e0)
    _, f = c.dense(f0)
    ops.stepcache_delta(c.x, e, f, ratios, _ws(c), *c.args())
    got = ratios.cpu().tolist()
    want = _ratio_ref((c.x_host.float() - e0.float()).bfloat16(), f0)
    assert math.isnan(got[1]), got
    for b in (0, 2):
        assert abs(got[b] - want[b]) <= RTOL * want[b], (b, got[b], want[b])


def test_without_f_no_ratio_is_written(gpu):
    from domain_rag_amd import ops
    c = _Case(SHAPES[1], gpu)
    e0 = _randn_bf((c.B, c.rows, c.cols), 2)
    ebuf, e = c.dense(e0)
    ratios = torch.full((c.B,), -3.0, dtype=torch.float64, device=gpu)
    ws = _ws(c)
    ws.fill_(0xAB)
    ops.stepcache_delta(c.x, e, None, ratios, ws, *c.args())
    torch.cuda.synchronize()
    assert torch.equal(_bits(e), _bits((c.x_host.float() - e0.float()).bfloat16().reshape(-1)))
    assert ratios.cpu().tolist() == [-3.0] * c.B and bool((ws.cpu() == 0xAB).all())
    _assert_guards(ebuf, e.numel(), "e"); c.assert_joint_frame("delta without f")
    ops.stepcache_delta(c.x, e, None, None, None, *c.args())      # ... and neither buffer is needed
    torch.cuda.synchronize()


def test_refused_calls_launch_nothing(gpu):
    from domain_rag_amd import ops
    c = _Case(SHAPES[1], gpu)
    e0, f0 = _randn_bf((c.B, c.rows, c.cols), 2), _randn_bf((c.B, c.rows, c.cols), 3)
    _, e = c.dense(e0)
    _, f = c.dense(f0)
    ratios = torch.full((c.B,), -3.0, dtype=torch.float64, device=gpu)
    ws = _ws(c)
    B, rows, cols, stride = c.args()

    def untouched():
        torch.cuda.synchronize()
        assert torch.equal(_bits(e), _bits(e0.reshape(-1))) and torch.equal(_bits(f), _bits(f0.reshape(-1)))
        assert torch.equal(_bits(c.x_now()), _bits(c.x_host)) and ratios.cpu().tolist() == [-3.0] * B
        c.assert_joint_frame("refused call")

    for bad in (dict(cols=100), dict(stride=rows * cols - 8)):          # cols % 8 != 0; a batch stride shorter than an image
        a = dict(B=B, rows=rows, cols=cols, stride=stride); a.update(bad)
        with pytest.raises(RuntimeError, match="drag_stepcache_delta_bf16"):
            ops.stepcache_delta(c.x, e, f, ratios, ws, a["B"], a["rows"], a["cols"], a["stride"])
        untouched()
        for sign in (+1, -1):
            with pytest.raises(RuntimeError, match="drag_stepcache_apply_bf16"):
                ops.stepcache_apply(c.x, f, a["B"], a["rows"], a["cols"], a["stride"], sign)
            untouched()
    with pytest.raises(RuntimeError, match="drag_stepcache_apply_bf16"):
        ops.stepcache_apply(c.x, f, B, rows, cols, stride, 0)           # sign must be +1 or -1
    untouched()
    # a CPU tensor anywhere is refused by the wrapper (there is no CPU path)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.stepcache_delta(c.x.cpu(), e, f, ratios, ws, B, rows, cols, stride)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.stepcache_delta(c.x, e, f.cpu(), ratios, ws, B, rows, cols, stride)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.stepcache_apply(c.x, f.cpu(), B, rows, cols, stride, +1)
    untouched()
    # operands too small for the addressing are the wrapper's to refuse: an error here, not a memory fault there
    with pytest.raises(ValueError):
        ops.stepcache_delta(c.x, e, f, ratios, ws, B + 1, rows, cols, stride)
    with pytest.raises(ValueError):
        ops.stepcache_apply(c.x, f[: f.numel() - 8], B, rows, cols, stride, +1)
    with pytest.raises(ValueError):
        ops.stepcache_delta(c.x, e, f, ratios, ws[:8], B, rows, cols, stride)
    untouched()
