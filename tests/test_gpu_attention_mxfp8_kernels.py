"""``ops.qkv_prep_mxfp8`` and ``ops.attention_mxfp8`` on the GPU.

1. the prep pass byte for byte against ``mx.quantize_ref`` of what ``ops.qk_norm_rope_vt`` writes (q, k) and of the zero-padded natural-order
   V^T, padding included, ``qkv`` untouched;
2. the kernel's operand maps on exact data (uniform scores, one-hot scores), under the single-stream blocks' output layout;
3. random data within the format's own distance: the kernel may sit at most 1.3 x further from float64 attention than ``mx.attention_ref``
   does, per case and per head (the figures go to profiles/attn_mxfp8_kernel_distance.json);
4. the wrappers' refusals.

Every device buffer is pre-filled with a sentinel and has guard elements on both sides; whatever a launch does not own must keep it."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "attn_mxfp8_kernel_distance.json")
SLACK = 1.3                 # the project's bar for a second evaluation of the same graph (tests/test_gpu_flux.py)
SENT = 0x7FC1               # a quiet NaN no kernel here produces
SENT8 = 0xA5                # image bytes nobody wrote
GUARD = 64
SCALE = 1 / math.sqrt(128)
B = 2


def _s_pad(S):
    return (S + 127) // 128 * 128


def _sentinel(n, dev):
    return torch.full((n,), SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _guarded_images(S, H, dev):
    """the six images as views into sentinel-filled stores with GUARD bytes on both sides -> (views, stores)"""
    sp = _s_pad(S)
    shapes = ((sp, 128), (sp, 4), (sp, 128), (sp, 4), (128, sp), (128, sp // 32))
    views, stores = [], []
    for shp in shapes:
        n = B * H * shp[0] * shp[1]
        store = torch.full((n + 2 * GUARD,), SENT8, dtype=torch.uint8, device=dev)
        stores.append(store)
        views.append(store[GUARD:GUARD + n].view(B, H, *shp))
    return tuple(views), stores


def _guards_hold(stores):
    return all(bool((s[:GUARD] == SENT8).all()) and bool((s[-GUARD:] == SENT8).all()) for s in stores)


def _prepared(q, k, v, dev):
    """prepared bf16 q, k, v [B, S, H, 128] (host) -> the six images on the device (no norm, no RoPE: the values are used as they are)"""
    from domain_rag_amd import ops
    S, H = q.shape[1], q.shape[2]
    D = H * 128
    qkv = torch.cat([q.reshape(B, S, D), k.reshape(B, S, D), v.reshape(B, S, D)], dim=2).contiguous().to(dev)
    images, stores = _guarded_images(S, H, dev)
    ops.qkv_prep_mxfp8(qkv, images, None, None, None, None, None, None, B, S, H, 3 * D, 0)
    torch.cuda.synchronize()
    assert _guards_hold(stores)
    return images


def _attend(images, S, H, layout="single"):
    """one launch under an output layout -> the owned [B, S, H, 128] region on the host; everything else must keep the sentinel"""
    from domain_rag_amd import ops
    D = H * 128
    dev = images[0].device
    if layout == "single":            # the single-stream blocks: attention | mlp side by side (F = 4 D), plus an 8-byte offset of the view
        ld_o, off = 5 * D, 4
    else:
        ld_o, off = D, 0
    o_bs = S * ld_o
    store = _sentinel(off + B * o_bs + GUARD, dev)
    out = store[off:]
    ops.attention_mxfp8(images, out, B, S, H, ld_o, o_bs, SCALE)
    torch.cuda.synchronize()
    owned = torch.zeros(store.numel(), dtype=torch.bool)
    view = torch.as_strided(torch.arange(store.numel()), (B, S, D), (o_bs, ld_o, 1), off)
    owned[view.reshape(-1)] = True
    bits = store.view(torch.int16).cpu()
    assert bool((bits[~owned] == SENT).all()), "an element outside the owned region was written"
    res = torch.as_strided(store, (B, S, D), (o_bs, ld_o, 1), off).cpu().view(B, S, H, 128)
    assert not bool((res.view(torch.int16) == SENT).any()), "an owned element was not written"
    return res


def _ulp_bf16(x):
    """one bf16 ulp at |x| (float64 tensor), with the smallest normal's ulp as the floor"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the prep pass, byte for byte
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,s_txt", [(17, 0), (17, 5), (64, 5), (65, 0), (129, 70), (333, 5), (333, 200)])
def test_prep_equals_the_host_quantiser_byte_for_byte(gpu, S, s_txt):
    from domain_rag_amd import mx, ops
    H = 3 if S == 65 else 2
    D = H * 128
    ld = 3 * D + 40                              # wide rows: the columns beyond belong to the caller
    g = torch.Generator().manual_seed(S * 31 + s_txt)
    store = _sentinel(B * S * ld + GUARD, gpu)
    qkv = torch.as_strided(store, (B, S, 3 * D), (S * ld, ld, 1), 0)
    host = (torch.randn(B, S, 3 * D, generator=g) * torch.exp(torch.randn(B, S, 1, generator=g))).bfloat16()
    host[0, S // 2, 2 * D:2 * D + 128] = 0       # an all-zero V row and an all-zero k row (a zero block: byte 127)
    host[1, 0, D:D + 128] = 0
    qkv.copy_(host.to(gpu))
    w = [(1 + 0.1 * torch.randn(128, generator=g)).bfloat16().to(gpu) for _ in range(4)]
    ang = torch.rand(S, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).contiguous().to(gpu), torch.sin(ang).contiguous().to(gpu)
    before = store.clone()
    images, stores = _guarded_images(S, H, gpu)
    ops.qkv_prep_mxfp8(qkv, images, w[0], w[1], w[2], w[3], cos, sin, B, S, H, ld, s_txt)
    torch.cuda.synchronize()
    assert torch.equal(store.view(torch.int16), before.view(torch.int16)), "qkv was modified"
    assert _guards_hold(stores)
    # what the bf16 pass writes, on a copy
    copy = before.clone()
    sp64 = (S + 63) // 64 * 64
    vt = torch.empty(B, H, 128, sp64, dtype=torch.bfloat16, device=gpu)
    ops.qk_norm_rope_vt(torch.as_strided(copy, (B, S, 3 * D), (S * ld, ld, 1), 0), vt, w[0], w[1], w[2], w[3], cos, sin, B, S, H, ld, s_txt)
    torch.cuda.synchronize()
    prep = torch.as_strided(copy, (B, S, 3 * D), (S * ld, ld, 1), 0).cpu()
    qq, qs, kq, ks, vq, vs = (t.cpu() for t in images)
    sp = _s_pad(S)
    for name, col, eb, sb in (("q", 0, qq, qs), ("k", D, kq, ks)):
        rows = prep[:, :, col:col + D].reshape(B, S, H, 128).permute(0, 2, 1, 3).reshape(-1, 128).contiguous()
        rb, rs = mx.quantize_ref(rows)
        assert torch.equal(eb[:, :, :S].reshape(-1, 128), rb), f"{name} bytes differ at {(eb[:, :, :S].reshape(-1, 128) != rb).nonzero()[:4].tolist()}"
        assert torch.equal(sb[:, :, :S].reshape(-1, 4), rs), f"{name} scales differ at {(sb[:, :, :S].reshape(-1, 4) != rs).nonzero()[:4].tolist()}"
        assert bool((eb[:, :, S:] == 0).all()) and bool((sb[:, :, S:] == 127).all()), f"{name}: padding rows must be (0, 127)"
    # V^T: natural key order, keys >= S zero, blocks of 32 keys
    vnat = torch.zeros(B, H, 128, sp, dtype=torch.bfloat16)
    vnat[:, :, :, :S] = host[:, :, 2 * D:].reshape(B, S, H, 128).permute(0, 2, 3, 1)
    rb, rs = mx.quantize_ref(vnat.reshape(-1, sp))
    assert torch.equal(vq.reshape(-1, sp), rb), f"V^T bytes differ at {(vq.reshape(-1, sp) != rb).nonzero()[:4].tolist()}"
    assert torch.equal(vs.reshape(-1, sp // 32), rs), f"V^T scales differ at {(vs.reshape(-1, sp // 32) != rs).nonzero()[:4].tolist()}"
    assert bool((vq[..., S:] == 0).all())
    first_all_pad = (S + 31) // 32
    assert bool((vs[..., first_all_pad:] == 127).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. operand maps on exact data
# ---------------------------------------------------------------------------------------------------------------------------------------
def _exact_v(S, H, g):
    """V [B, S, H, 128]: integers in [-4, 4] times a power of two that differs per (32-key block, d): every V^T scale byte differs from its
    neighbours and every element is an e4m3 value under its block's scale"""
    ints = torch.randint(-4, 5, (B, S, H, 128), generator=g).float()
    blk = (torch.arange(S) // 32).view(1, S, 1, 1)
    d = torch.arange(128).view(1, 1, 1, 128)
    hh = torch.arange(H).view(1, 1, H, 1)
    return (ints * torch.pow(2.0, ((blk * 3 + d + hh) % 7 - 3).float())).bfloat16()


@pytest.mark.parametrize("S", [17, 64, 65, 128, 129, 333])
def test_uniform_scores_average_v_exactly(gpu, S):
    """q = 0: every score is 0, P^ = 1, l = S, the accumulators are exact sums: out is within one bf16 ulp of bf16(sum V^ / S).  A V^T scale
    applied to the wrong block, or a P register under the wrong key, changes the sum."""
    from domain_rag_amd import mx
    H = 2
    g = torch.Generator().manual_seed(100 + S)
    v = _exact_v(S, H, g)
    k = torch.randn(B, S, H, 128, generator=g).bfloat16()
    q = torch.zeros(B, S, H, 128, dtype=torch.bfloat16)
    images = _prepared(q, k, v, gpu)
    # the test's premise: V survives its quantisation exactly
    vq, vs = images[4].cpu(), images[5].cpu()
    sp = _s_pad(S)
    vhat = mx.dequantize_ref(vq.reshape(-1, sp), vs.reshape(-1, sp // 32)).view(B, H, 128, sp)[..., :S].permute(0, 3, 1, 2)
    assert torch.equal(vhat, v.float())
    assert len(torch.unique(vs[0, 0, :7, 0])) == 7
    out = _attend(images, S, H).double()
    want = (v.double().sum(dim=1, keepdim=True) / S).expand(B, S, H, 128)
    err = (out - want.float().bfloat16().double()).abs()
    assert bool((err <= _ulp_bf16(want)).all()), f"max error {err.max().item():.3e} at {(err > _ulp_bf16(want)).nonzero()[:4].tolist()}"


@pytest.mark.parametrize("S", [17, 64, 65, 128, 129, 333])
def test_one_hot_scores_pick_the_permuted_row(gpu, S):
    """k rows are +-1 codes, q_i = 4 k_pi(i): query i scores key pi(i) at least 20 log2 units above every other key (asserted on the data), so
    P^ is a permutation matrix and out[i] is V[pi(i)] to within one bf16 ulp (plus what exact softmax itself leaks from the other keys).  pi is a fixed permutation that is no involution and crosses
    the 128-key tiles (where S has more than one): a key landing in the wrong P register, or a K row under the wrong score, picks another
    row of V."""
    H = 2
    g = torch.Generator().manual_seed(200 + S)
    pi = torch.randperm(S, generator=g)
    assert not torch.equal(pi[pi], torch.arange(S))
    if S > 128:
        assert bool(((pi // 128) != (torch.arange(S) // 128)).any())
    k = (torch.randint(0, 2, (B, S, H, 128), generator=g) * 2 - 1).float()
    q = 4.0 * k[:, pi]
    scores = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * SCALE * math.log2(math.e)
    top = scores.gather(3, pi.view(1, 1, S, 1).expand(B, H, S, 1))
    others = scores.scatter(3, pi.view(1, 1, S, 1).expand(B, H, S, 1), float("-inf"))
    gap = (top.squeeze(3) - others.amax(dim=3)).min().item()
    assert gap >= 20.0
    v = _exact_v(S, H, g)
    images = _prepared(q.bfloat16(), k.bfloat16(), v, gpu)
    out = _attend(images, S, H).double()
    want = v[:, pi].double()
    err = (out - want).abs()
    # exact softmax itself leaves sum_{j != pi(i)} 2^-gap_j V[j] next to V[pi(i)] (visible where V[pi(i)] is 0, and kept by a flash evaluation
    # whose early tiles ran under a smaller maximum): at most S 2^-gap max|V| on top of the one ulp
    leak = S * 2.0 ** -gap * v.double().abs().max().item()
    assert bool((err <= _ulp_bf16(want) + leak).all()), f"leak bound {leak:.3e}, max error {err.max().item():.3e} at {(err > _ulp_bf16(want)).nonzero()[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. within the format's own distance
# ---------------------------------------------------------------------------------------------------------------------------------------
def _record(key, values):
    try:
        with open(RECORD) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        rec = {}
    rec[key] = values
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _rms_rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _draw(dist, S, H, g):
    q, k, v = (torch.randn(B, S, H, 128, generator=g) for _ in range(3))
    if dist == "hot":                         # hot logits
        q = q * 4
    elif dist == "outlier_k":                 # one x30 channel in k
        k[..., 5] *= 30
    elif dist == "student_t_v":               # heavy tails in v (3 degrees of freedom)
        chi = torch.randn(B, S, H, 128, 3, generator=g).pow(2).sum(-1)
        v = v / (chi / 3).sqrt()
    elif dist == "all_negative":              # every score of every row below -126 log2 units
        u = torch.ones(128)
        q = 8 * u + 0.5 * q
        k = -2 * u + 0.25 * k
    elif dist == "max_in_last_tile":          # every row's maximum is key S - 3, inside the last, partly padded tile
        u = (torch.randint(0, 2, (128,), generator=g) * 2 - 1).float()
        q = q + u
        k[:, S - 3] = 2 * u
    elif dist != "normal":
        raise KeyError(dist)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def _exact(q, k, v):
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * SCALE
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=3), v.double()), s


CASES3 = [(dist, S) for S in (72, 333, 1241) for dist in ("normal", "hot", "outlier_k", "student_t_v")] + \
         [("all_negative", 333), ("max_in_last_tile", 333)]


@pytest.mark.parametrize("dist,S", CASES3)
def test_kernel_within_the_formats_own_distance(gpu, dist, S):
    from domain_rag_amd import mx
    H = 2
    g = torch.Generator().manual_seed(300 + S + 17 * len(dist))
    q, k, v = _draw(dist, S, H, g)
    exact, scores = _exact(q, k, v)
    if dist == "all_negative":
        assert (scores * math.log2(math.e)).max().item() < -126.0
    if dist == "max_in_last_tile":
        assert S % 128 != 0 and S - 3 >= S // 128 * 128 and bool((scores.argmax(dim=3) == S - 3).all())
    out = _attend(_prepared(q, k, v, gpu), S, H, layout="dense")
    assert bool(torch.isfinite(out.float()).all())
    figures = {}
    for b in range(B):
        for h in range(H):
            ref = mx.attention_ref(q[b, :, h], k[b, :, h], v[b, :, h], SCALE)
            d_ref, d_hip = _rms_rel(ref, exact[b, :, h]), _rms_rel(out[b, :, h], exact[b, :, h])
            figures[f"b{b}h{h}"] = dict(kernel_vs_exact=d_hip, attention_ref_vs_exact=d_ref, ratio=d_hip / d_ref)
            print(f"{dist} S={S} b={b} h={h}: kernel vs float64 {d_hip:.4e}, mx.attention_ref vs float64 {d_ref:.4e}, ratio {d_hip / d_ref:.3f}")
    _record(f"{dist}_S{S}", dict(bar=SLACK, **figures))
    for key, f in figures.items():
        assert f["kernel_vs_exact"] <= SLACK * f["attention_ref_vs_exact"], (dist, S, key, f)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. argument checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(gpu):
    from domain_rag_amd import _lib, ops
    S, H = 65, 2
    D = H * 128
    images = ops.attention_mxfp8_images(B, S, H, gpu)
    assert [tuple(t.shape) for t in images] == [(B, H, 128, 128), (B, H, 128, 4), (B, H, 128, 128), (B, H, 128, 4), (B, H, 128, 128), (B, H, 128, 4)]
    out = torch.empty(B * S * D, dtype=torch.bfloat16, device=gpu)
    qkv = torch.zeros(B, S, 3 * D, dtype=torch.bfloat16, device=gpu)
    ops.qkv_prep_mxfp8(qkv, images, None, None, None, None, None, None, B, S, H, 3 * D, 0)
    ops.attention_mxfp8(images, out, B, S, H, D, S * D, SCALE)                   # the well-formed call
    for i in range(6):                                                           # every image one byte short
        short = list(images)
        short[i] = images[i].view(-1)[1:]
        with pytest.raises(ValueError):
            ops.attention_mxfp8(short, out, B, S, H, D, S * D, SCALE)
        with pytest.raises(ValueError):
            ops.qkv_prep_mxfp8(qkv, short, None, None, None, None, None, None, B, S, H, 3 * D, 0)
    with pytest.raises(ValueError):
        ops.attention_mxfp8(images[:5], out, B, S, H, D, S * D, SCALE)
    with pytest.raises(ValueError):
        ops.attention_mxfp8(tuple(t.int() for t in images), out, B, S, H, D, S * D, SCALE)
    with pytest.raises(ValueError):                                              # short output
        ops.attention_mxfp8(images, out[1:], B, S, H, D, S * D, SCALE)
    with pytest.raises(ValueError):                                              # negative strides
        ops.attention_mxfp8(images, out, B, S, H, -D, S * D, SCALE)
    with pytest.raises(ValueError):
        ops.attention_mxfp8(images, out, B, S, H, D, -S * D, SCALE)
    with pytest.raises(ValueError):                                              # overlapping output rows
        ops.attention_mxfp8(images, out, B, S, H, D - 8, S * D, SCALE)
    with pytest.raises(ValueError):                                              # qkv short for its row map
        ops.qkv_prep_mxfp8(qkv, images, None, None, None, None, None, None, B, S, H, 3 * D + 8, 0)
    # what the library itself refuses, before any launch
    big = torch.empty(B * S * (D + 2) + 8, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError):
        ops.attention_mxfp8(images, big, B, S, H, D + 2, S * (D + 2), SCALE)     # ld_o % 4
    with pytest.raises(RuntimeError):
        ops.attention_mxfp8(images, big[1:], B, S, H, D, S * D, SCALE)           # out not 8-byte aligned
    with pytest.raises(RuntimeError):
        ops.attention_mxfp8(images, out, B, S, H, D, S * D, 0.0)                 # the scale must be positive
    lib = _lib.load()
    assert ops.attention_mxfp8_supported(B, S, H) and ops.attention_mxfp8_supported(8, 24166, 24)
    for shape in ((1, (1 << 23) + 1, 1), (70000, 16, 1), (1, 16, 70000), (0, 16, 1)):
        assert not ops.attention_mxfp8_supported(*shape)
        p = [t.data_ptr() for t in images]
        assert lib.drag_attention_mxfp8(*p, out.data_ptr(), *shape, 128 * shape[2], 0, SCALE, None) != 0
        assert lib.drag_qkv_prep_mxfp8(qkv.data_ptr(), None, None, None, None, None, None, *shape, 3 * 128 * shape[2], 0, 1e-6, *p, None) != 0
    assert lib.drag_attention_mxfp8_s_pad(S) == 128 and lib.drag_attention_mxfp8_s_pad(128) == 128 and lib.drag_attention_mxfp8_s_pad(129) == 256
    assert lib.drag_attention_mxfp8_kernel_name(S).decode().startswith("attention_mxfp8_kernel")
    torch.cuda.synchronize()
