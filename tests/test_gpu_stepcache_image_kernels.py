"""The list forms of csrc/stepcache.hip (``ops.stepcache_swap``, ``ops.stepcache_apply_images``, ``ops.stepcache_copy_images``), each called
directly.

As in tests/test_gpu_stepcache_kernels.py, every operand a kernel writes is a slice of a sentinel-filled buffer (bf16 7.0) with 256 guard
elements on both sides; ``x`` is the image-row part of a joint [B, text + rows, cols] buffer whose text rows (the gap between two images)
hold the sentinel too.  After a call every guard and gap element must hold the sentinel bit for bit.

None of the three does arithmetic of its own: a swap and a copy move bits, and ``apply_images`` must give, on the listed images, the bits
the whole-batch ``ops.stepcache_apply`` gives and leave the bits of every other image alone.  Everything is compared bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 7.0


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
    """a joint [B, T + rows, cols] buffer with sentinel text rows; x = its flat view from the first image row on"""

    def __init__(self, B, rows, cols, T, dev, seed=1):
        self.B, self.rows, self.cols, self.T, self.dev = B, rows, cols, T, dev
        self.stride = (T + rows) * cols
        self.x_host = _randn_bf((B, rows, cols), seed)
        self.buf, joint = _guarded(B * self.stride, dev)
        self.joint = joint.view(B, T + rows, cols)
        self.joint[:, T:] = self.x_host.to(dev)
        self.x = joint[T * cols:]

    def args(self):
        return self.B, self.rows, self.cols, self.stride

    def x_now(self):
        return self.joint[:, self.T:].cpu()

    def assert_frame(self, what):
        _assert_guards(self.buf, self.B * self.stride, what + ": joint buffer")
        if self.T:
            assert bool((_bits(self.joint[:, :self.T]) == _sent_bits()).all()), f"{what}: a gap row of the joint buffer was written"

    def dense(self, host):
        buf, v = _guarded(host.numel(), self.dev)
        v.copy_(host.reshape(-1).to(self.dev))
        return buf, v


@pytest.mark.parametrize("cols", [8, 136])
@pytest.mark.parametrize("T", [0, 3])          # dense, and a batch stride with a gap
def test_swap(gpu, cols, T):
    from domain_rag_amd import ops
    c = _Joint(5, 7, cols, T, gpu)
    ops.stepcache_swap(c.x, *c.args(), [(0, 3), (1, 4)])
    torch.cuda.synchronize()
    want = c.x_host[[3, 4, 2, 0, 1]]
    assert torch.equal(_bits(c.x_now()), _bits(want)), "images after the swap (2 must be untouched)"
    c.assert_frame("swap")
    ops.stepcache_swap(c.x, *c.args(), [(0, 3), (1, 4)])          # the same swaps again restore the order
    ops.stepcache_swap(c.x, *c.args(), [])                        # no pairs: nothing happens
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.x_now()), _bits(c.x_host))
    c.assert_frame("swap back")


def test_swap_of_many_workgroups_per_image(gpu):
    """70 400 vectors per image: more than one trip of the grid-stride loop at the grid cap (2048 workgroups over 1 pair)"""
    from domain_rag_amd import ops
    c = _Joint(3, 1100, 512, 1, gpu)
    ops.stepcache_swap(c.x, *c.args(), [(0, 2)])
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.x_now()), _bits(c.x_host[[2, 1, 0]]))
    c.assert_frame("large swap")


LISTS = [[0], [3], [1, 3], [0, 1, 2, 3], []]          # B = 4: the first, the last, two inside, all, none


@pytest.fixture(scope="module")
def whole_batch(gpu):
    """what the whole-batch kernels give on the test's operands, computed once: (x after +1, r after -1 on the ORIGINAL x)"""
    from domain_rag_amd import ops
    c = _Joint(4, 333, 136, 5, gpu)
    r0 = _randn_bf((c.B, c.rows, c.cols), 5)
    _, r = c.dense(r0)
    ops.stepcache_apply(c.x, r, *c.args(), +1)
    x_plus = c.x_now()
    c = _Joint(4, 333, 136, 5, gpu)
    ops.stepcache_apply(c.x, r, *c.args(), -1)
    torch.cuda.synchronize()
    return dict(r0=r0, x_plus=x_plus, r_minus=r.cpu().view(c.B, c.rows, c.cols).clone())


@pytest.mark.parametrize("images", LISTS)
def test_apply_images_both_signs(gpu, whole_batch, images):
    from domain_rag_amd import ops
    c = _Joint(4, 333, 136, 5, gpu)
    r0 = whole_batch["r0"]
    n = r0.numel()
    rest = [b for b in range(c.B) if b not in images]
    rbuf, r = c.dense(r0)
    ops.stepcache_apply_images(c.x, r, *c.args(), +1, images)
    torch.cuda.synchronize()
    got = c.x_now()
    assert torch.equal(_bits(got[images]), _bits(whole_batch["x_plus"][images])), "listed images after apply_images(+1)"
    assert torch.equal(_bits(got[rest]), _bits(c.x_host[rest])), "an image outside the list was written by apply_images(+1)"
    assert torch.equal(_bits(r), _bits(r0.reshape(-1))), "r was written by apply_images(+1)"
    _assert_guards(rbuf, n, "r"); c.assert_frame("apply_images +1")
    c = _Joint(4, 333, 136, 5, gpu)
    ops.stepcache_apply_images(c.x, r, *c.args(), -1, images)
    torch.cuda.synchronize()
    got = r.cpu().view(c.B, c.rows, c.cols)
    assert torch.equal(_bits(got[images]), _bits(whole_batch["r_minus"][images])), "listed images of r after apply_images(-1)"
    assert torch.equal(_bits(got[rest]), _bits(r0[rest])), "an image of r outside the list was written by apply_images(-1)"
    assert torch.equal(_bits(c.x_now()), _bits(c.x_host)), "x was written by apply_images(-1)"
    _assert_guards(rbuf, n, "r"); c.assert_frame("apply_images -1")


@pytest.mark.parametrize("images", LISTS)
@pytest.mark.parametrize("strided", [True, False])
def test_copy_images(gpu, images, strided):
    """the source is the joint buffer (strided) or a dense buffer; the whole-batch counterpart is ``dst.copy_(src)``"""
    from domain_rag_amd import ops
    c = _Joint(4, 333, 136, 5 if strided else 0, gpu)
    d0 = _randn_bf((c.B, c.rows, c.cols), 9)
    dbuf, d = c.dense(d0)
    rest = [b for b in range(c.B) if b not in images]
    ops.stepcache_copy_images(d, c.x, c.stride, c.B, c.rows, c.cols, images)
    torch.cuda.synchronize()
    got = d.cpu().view(c.B, c.rows, c.cols)
    assert torch.equal(_bits(got[images]), _bits(c.x_host[images])), "listed images after copy_images"
    assert torch.equal(_bits(got[rest]), _bits(d0[rest])), "an image outside the list was written by copy_images"
    assert torch.equal(_bits(c.x_now()), _bits(c.x_host)), "the source was written"
    _assert_guards(dbuf, d0.numel(), "dst"); c.assert_frame("copy_images")


def test_refused_calls_launch_nothing(gpu):
    import ctypes
    from domain_rag_amd import _lib, ops
    c = _Joint(5, 7, 136, 3, gpu)
    r0 = _randn_bf((c.B, c.rows, c.cols), 5)
    _, r = c.dense(r0)
    B, rows, cols, stride = c.args()

    def untouched():
        torch.cuda.synchronize()
        assert torch.equal(_bits(r), _bits(r0.reshape(-1))) and torch.equal(_bits(c.x_now()), _bits(c.x_host))
        c.assert_frame("refused call")

    calls = {
        "drag_stepcache_swap_bf16": lambda x=c.x, cols=cols, lst=((0, 3),): ops.stepcache_swap(x, B, rows, cols, stride, lst),
        "drag_stepcache_apply_images_bf16": lambda x=c.x, cols=cols, lst=(0, 3): ops.stepcache_apply_images(x, r, B, rows, cols, stride, +1, lst),
        "drag_stepcache_copy_images_bf16": lambda x=c.x, cols=cols, lst=(0, 3): ops.stepcache_copy_images(r, x, stride, B, rows, cols, lst),
    }
    bad_lists = {
        "drag_stepcache_swap_bf16": [((0, B),), ((0, 3), (3, 4)), ((1, 1),), ((-1, 2),), tuple((i, i + 33) for i in range(33))],      # an index equal to B; overlapping pairs; a pair with itself; 66 entries
        "drag_stepcache_apply_images_bf16": [(0, B), (1, 1), (3, 1), (-1,), tuple(range(65))],      # an index equal to B; a repeated index; not increasing; 65 entries
    }
    bad_lists["drag_stepcache_copy_images_bf16"] = bad_lists["drag_stepcache_apply_images_bf16"]
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=name):
            call(cols=12)                                         # cols % 8 != 0
        untouched()
        with pytest.raises(RuntimeError, match=name):
            call(x=c.x[4:])                                       # a pointer that is 8-byte but not 16-byte aligned
        untouched()
        for lst in bad_lists[name]:
            with pytest.raises(RuntimeError, match=name):
                call(lst=lst)
            untouched()
    with pytest.raises(RuntimeError, match="drag_stepcache_apply_images_bf16"):
        ops.stepcache_apply_images(c.x, r, B, rows, cols, stride, 0, (0,))          # sign must be +1 or -1
    with pytest.raises(RuntimeError, match="drag_stepcache_swap_bf16"):
        ops.stepcache_swap(c.x, B, rows, cols, rows * cols - 8, ((0, 1),))          # a batch stride shorter than an image
    untouched()
    # null pointers: only the library can be handed one
    lib, one = _lib.load(), (ctypes.c_int32 * 2)(0, 1)
    xp, rp = ctypes.c_void_p(c.x.data_ptr()), ctypes.c_void_p(r.data_ptr())
    assert lib.drag_stepcache_swap_bf16(None, B, rows, cols, stride, one, 1, None) == -1
    assert lib.drag_stepcache_swap_bf16(xp, B, rows, cols, stride, None, 1, None) == -1
    assert lib.drag_stepcache_apply_images_bf16(xp, None, B, rows, cols, stride, 1, one, 2, None) == -1
    assert lib.drag_stepcache_apply_images_bf16(xp, rp, B, rows, cols, stride, 1, None, 2, None) == -1
    assert lib.drag_stepcache_copy_images_bf16(None, xp, stride, B, rows, cols, one, 2, None) == -1
    assert lib.drag_stepcache_copy_images_bf16(rp, None, stride, B, rows, cols, one, 2, None) == -1
    untouched()
    # a CPU tensor is refused by the wrapper, and so is an operand too small for the addressing
    with pytest.raises(RuntimeError, match="GPU"):
        ops.stepcache_swap(c.x.cpu(), B, rows, cols, stride, ((0, 1),))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.stepcache_apply_images(c.x, r.cpu(), B, rows, cols, stride, +1, (0,))
    with pytest.raises(ValueError):
        ops.stepcache_swap(c.x, B + 1, rows, cols, stride, ((0, 1),))
    with pytest.raises(ValueError):
        ops.stepcache_copy_images(r[: r.numel() - 8], c.x, stride, B, rows, cols, (0,))
    untouched()
