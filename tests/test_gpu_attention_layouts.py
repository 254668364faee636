"""The head_dim-128 attention path under the layouts it is used with, not only the dense one.

A layout changes addresses, not arithmetic: for one kernel under one set of switches a strided launch gives the bits of the dense launch and
leaves every element it does not own as it was.  Every buffer is pre-filled with one NaN bit pattern and compared through int16 views, so no
tolerance is involved — except one float64 anchor of the dense result itself, at the bar tests/test_gpu_kernels.py::test_attention uses.
The prep pass (``qk_norm_rope_vt`` / ``k_norm_rope_vt``) gets the same treatment, its V^T image a host-built expectation bit for bit, and the
wrappers' operand room checks their refusal cases (the arithmetic itself: tests/test_attention_room_host.py, no GPU)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 0x7FC1               # a quiet NaN no kernel here produces: "nobody wrote this element"
SCALE = 1 / math.sqrt(128)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _sentinel(n, dev):
    return torch.full((n,), SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _first_diff(a, b):
    """index of the first element whose bits differ (a, b: same shape), or None"""
    ne = (_bits(a) != _bits(b)).nonzero()
    return None if ne.numel() == 0 else tuple(ne[0].tolist())


def _strided(store, shape, strides, off):
    return torch.as_strided(store, shape, strides, off)


# ---- the kernel families: the smallest shape that reaches each, the switches that select it, and what the library's own dispatch query must
# answer for it (drag_attention_bf16_choice, drag_attention_bf16_kernel_name): a later policy change fails the test instead of hollowing it out.
# route: "plain" = attention over a prepared q, "qprep" = attention_qprep, "v" / "vq" = attention_v without / with the fused q preparation.
# s_txt of the q-prep routes is no multiple of 64.
D128 = "attention_d128_kernel<%d, ..., %s, ...>"
CASES = {
    # 4-wave, default switches: a ragged last 128-query block
    "w4": dict(B=2, H=2, S=200, s_txt=0, opts={}, route="plain", code=4, name=D128 % (4, "false")),
    "w4_qprep": dict(B=2, H=2, S=200, s_txt=24, opts={}, route="qprep", code=4, name=D128 % (4, "true")),
    # 8-wave: 65 KV tiles, a ragged last 256-query block
    "w8": dict(B=2, H=1, S=4100, s_txt=0, opts=dict(attn_q64=2), route="plain", code=8, name=D128 % (8, "false")),
    "w8_qprep": dict(B=2, H=1, S=4100, s_txt=300, opts=dict(attn_q64=2), route="qprep", code=8, name=D128 % (8, "true")),
    # the hand-placed 64-query kernel: 17 tiles do not pair up
    "q64": dict(B=2, H=2, S=1030, s_txt=0, opts=dict(attn_q64=1), route="plain", code=64, name="attention_q64_kernel<false>"),
    "q64_qprep": dict(B=2, H=2, S=1030, s_txt=300, opts=dict(attn_q64=1), route="qprep", code=64, name="attention_q64_kernel<true>"),
    # the generated stream (18 tiles), without the fold ...
    "q64g": dict(B=2, H=2, S=1100, s_txt=0, opts=dict(attn_q64=1), route="plain", code=640, name="attention_q64g_kernel<false, false>"),
    "q64g_qprep_nofold": dict(B=2, H=2, S=1100, s_txt=300, opts=dict(attn_q64=1, attn_gen=2), route="qprep", code=640,
                              name="attention_q64g_kernel<true, false>"),
    # ... and with it (the product's choice under the fused q preparation)
    "q64g_fold": dict(B=2, H=2, S=1100, s_txt=300, opts=dict(attn_q64=1, attn_gen=0), route="qprep", code=641,
                      name="attention_q64g_kernel<true, true>"),
    # walking: 8 (batch, head) x 5 query blocks = 40 items behind 8 workgroups, the last block ragged
    "walk": dict(B=2, H=4, S=1100, s_txt=0, opts=dict(attn_q64=1, attn_walk=8), route="plain", code=640,
                 name="attention_q64g_kernel<false, false>", walk=8),
    "walk_fold": dict(B=2, H=4, S=1100, s_txt=300, opts=dict(attn_q64=1, attn_walk=8, attn_gen=0), route="qprep", code=641,
                      name="attention_q64g_kernel<true, true>", walk=8),
    # row-major V, both block sizes, without and with the fused q preparation
    "vrow_w4": dict(B=2, H=2, S=200, s_txt=0, opts={}, route="v", code=4, name=D128 % (4, "false")),
    "vrow_w4_qprep": dict(B=2, H=2, S=200, s_txt=24, opts={}, route="vq", code=4, name=D128 % (4, "true")),
    "vrow_w8": dict(B=2, H=1, S=4100, s_txt=0, opts=dict(attn_q64=2), route="v", code=8, name=D128 % (8, "false")),
    "vrow_w8_qprep": dict(B=2, H=1, S=4100, s_txt=300, opts=dict(attn_q64=2), route="vq", code=8, name=D128 % (8, "true")),
}
LAYOUTS = ["L1", "L2", "L3a", "L3b", "L3c"]


def _out_layout(layout, S, D):
    """(ld_o, o_batch_stride, offset of the out view in its storage) of a layout"""
    if layout == "dense":
        return D, S * D, 0
    if layout == "L1":        # the DiT's single-stream blocks: attention | mlp side by side, F = 4 D
        return 5 * D, S * 5 * D, 0
    if layout == "L2":        # padded everywhere
        return D + 24, (S + 2) * (D + 24), 8
    if layout == "L3a":       # rows 8-byte aligned only: ld_o % 8 == 4
        return D + 4, S * (D + 4), 0
    if layout == "L3b":       # out itself 8-byte aligned only
        return D + 8, S * (D + 8), 4
    if layout == "L3c":       # batch 1's rows 8-byte aligned only: o_batch_stride % 8 == 4
        return D + 8, S * (D + 8) + 4, 0
    raise KeyError(layout)


def _narrow_reasons(out_ptr, ld_o, o_bs):
    """which of attention_launch's three conditions drop the 16-byte epilogue stores"""
    return [ld_o % 8 != 0, out_ptr % 16 != 0, o_bs % 8 != 0]


@functools.lru_cache(maxsize=None)
def _operands(name):
    """the operands of a case, built once: qkv drawn densely on the host, prepared once on the dense copy on the GPU"""
    from domain_rag_amd import ops
    c = CASES[name]
    B, S, H, s_txt = c["B"], c["S"], c["H"], c["s_txt"]
    D = H * 128
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + S + 7 * H + s_txt)
    qkv = torch.randn(B, S, 3 * D, generator=g).bfloat16()
    w = [(1 + 0.1 * torch.randn(128, generator=g)).bfloat16().to(dev) for _ in range(4)]      # wq_txt, wk_txt, wq_img, wk_img
    ang = torch.rand(S, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev)
    d = qkv.to(dev)
    s_pad = (S + 63) // 64 * 64
    vt = _sentinel(B * H * 128 * s_pad, dev).view(B, H, 128, s_pad)
    if c["route"] in ("qprep", "vq"):
        ops.k_norm_rope_vt(d, vt, w[1], w[3], cos, sin, B, S, H, 3 * D, s_txt)
    else:
        ops.qk_norm_rope_vt(d, vt, None, None, None, None, None, None, B, S, H, 3 * D, 0)
    torch.cuda.synchronize()
    return dict(qkv=d, host_qkv=qkv, vt=vt, w=w, cos=cos, sin=sin)


def _launch(name, layout):
    """one attention launch of a case under a layout -> (the [B, S, D] region it owns, the whole output storage, a mask of the owned
    elements), all on the host.  Inputs are dense except under L2; every gap of every buffer holds the sentinel before the launch, and the
    inputs are checked to hold their bits after it."""
    from domain_rag_amd import _lib, ops
    c, x = CASES[name], _operands(name)
    B, S, H, s_txt, route = c["B"], c["S"], c["H"], c["s_txt"], c["route"]
    D = H * 128
    dev = x["qkv"].device
    if layout == "L2":
        ld, bs, off = 3 * D + 72, (S + 3) * (3 * D + 72), 136
        store = _sentinel(off + (B - 1) * bs + (S - 1) * ld + 3 * D + 40, dev)
        _strided(store, (B, S, 3 * D), (bs, ld, 1), off).copy_(x["qkv"])
    else:
        ld, bs, off, store = 3 * D, S * 3 * D, 0, x["qkv"].view(-1)
    before = store.clone()
    q, k, v = store[off:], store[off + D:], store[off + 2 * D:]
    assert all(t.data_ptr() % 16 == 0 for t in (q, k, v)) and ld % 8 == 0          # inside the kernels' contract
    ld_o, o_bs, o_off = _out_layout(layout, S, D)
    ostore = _sentinel(o_off + (B - 1) * o_bs + S * ld_o + 24, dev)
    out = ostore[o_off:]
    assert out.data_ptr() % 8 == 0 and ld_o % 4 == 0
    lib = _lib.load()
    assert ops.get_option("attn_tune") & 2, "the default asks for 16-byte epilogue stores: the dense launch takes them"
    reasons = _narrow_reasons(out.data_ptr(), ld_o, o_bs)
    assert sum(reasons) == {"dense": 0, "L1": 0, "L2": 0, "L3a": 1, "L3b": 1, "L3c": 1}[layout], (layout, reasons)
    if layout.startswith("L3"):
        assert reasons.index(True) == "abc".index(layout[2]), (layout, reasons)    # each of the three exactly once
    vrow, qprep = route in ("v", "vq"), route in ("qprep", "vq")
    with ops.options(**c["opts"]):
        # the kernel that runs is the intended one, by the library's own dispatch queries under these switches
        assert lib.drag_attention_bf16_choice(S, int(vrow), int(qprep)) == c["code"], name
        assert lib.drag_attention_bf16_kernel_name(S, int(vrow), int(qprep)).decode() == c["name"], name
        if "walk" in c:
            # attention_launch walks when a grid is forced ("attn_walk" = 8), every item exists (B H a multiple of 8) and there are more
            # items (8 * ceil(B H / 8) * ceil(S / 256)) than workgroups
            items = 8 * ((B * H + 7) // 8) * ((S + 255) // 256)
            assert ops.get_option("attn_walk") == c["walk"] and (B * H) % 8 == 0 and items == 40 > c["walk"]
        prep = (x["w"][0], x["w"][2], x["cos"], x["sin"], s_txt)
        if route == "plain":
            ops.attention(q, k, x["vt"], out, B, S, H, ld, bs, ld_o, o_bs, SCALE)
        elif route == "qprep":
            ops.attention_qprep(q, k, x["vt"], out, B, S, H, ld, bs, ld_o, o_bs, SCALE, *prep)
        elif route == "v":
            ops.attention_v(q, k, v, out, B, S, H, ld, bs, ld_o, o_bs, SCALE)
        else:
            ops.attention_v(q, k, v, out, B, S, H, ld, bs, ld_o, o_bs, SCALE, *prep)
    torch.cuda.synchronize()
    assert torch.equal(_bits(store), _bits(before)), (name, layout, "the launch wrote into its inputs")
    owned = torch.zeros(ostore.numel(), dtype=torch.bool, device=dev)
    _strided(owned, (B, S, D), (o_bs, ld_o, 1), o_off).fill_(True)
    return _strided(ostore, (B, S, D), (o_bs, ld_o, 1), o_off).cpu(), ostore.cpu(), owned.cpu()


@functools.lru_cache(maxsize=None)
def _dense(name):
    got, store, owned = _launch(name, "dense")
    assert torch.isfinite(got.float()).all(), name
    assert (_bits(store)[~owned] == SENT).all(), (name, "dense: wrote past its [B, S, D]")
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_strided_launch_equals_the_dense_launch_bit_for_bit(gpu, name, layout):
    """every kernel family x every layout: the owned [B, S, D] region holds the dense launch's bits, everything else still the sentinel.
    L1 is the layout flux.py gives 38 of Flux's 57 blocks; L3a-c each take the 8-byte epilogue stores for one of attention_launch's three
    reasons (in the walking kernels the same bit sets the store count a workgroup waits behind before it reuses registers)."""
    ref = _dense(name)
    got, store, owned = _launch(name, layout)
    at = _first_diff(got, ref)
    if at is not None:
        b, s, col = at
        pytest.fail(f"{name} ({CASES[name]['name']}) under {layout}: first differing (b, s, h, d) = ({b}, {s}, {col // 128}, {col % 128}): "
                    f"{got[at].item()} vs dense {ref[at].item()}; {(_bits(got) != _bits(ref)).sum().item()} elements differ")
    stray = ((_bits(store) != SENT) & ~owned).nonzero()
    assert stray.numel() == 0, f"{name} under {layout}: {stray.shape[0]} elements outside the owned region overwritten, first at storage offset {stray[0].item()}"


def test_dense_4_wave_result_against_float64(gpu):
    """the dense launch is the code under test everywhere above: anchored once, under L1, against float64 attention over the kernel's own bf16
    q / k (test_attention's bar, tests/test_gpu_kernels.py)"""
    from oracle import ops_ref
    c, x = CASES["w4"], _operands("w4")
    B, S, H = c["B"], c["S"], c["H"]
    got, _, _ = _launch("w4", "L1")
    q, k, v = (t.view(B, S, H, 128).transpose(1, 2) for t in x["qkv"].cpu().split(H * 128, dim=-1))       # (no weights, no RoPE: as drawn)
    assert torch.equal(x["qkv"].cpu(), x["host_qkv"])
    assert _rel(got, ops_ref.attention_ref_f64(q, k, v, SCALE)) < 1.5e-2


# ------------------------------------------------------------------ the prep pass
def _vt_expected(v, S):
    """the V^T image from v [B, S, H, 128] (host), by the kernel's comment (attention_prep.hip: position q of a 64-key tile -> group q >> 4,
    within = q & 15 = 8 h + jj -> key offset 8 (jj >> 2) + 4 h + (jj & 3)): position 16 g + w of row d holds
    V[16 g + 8 ((w >> 2) & 1) + 4 (w >> 3) + (w & 3)][d]; keys >= S are +0.0; the image is s_pad = S rounded up to 64 wide"""
    B, _, H, _ = v.shape
    s_pad = (S + 63) // 64 * 64
    pos = torch.arange(s_pad)
    w = pos & 15
    key = (pos & ~15) + 8 * ((w >> 2) & 1) + 4 * (w >> 3) + (w & 3)
    assert sorted(key.tolist()) == list(range(s_pad))          # a permutation, inside each group of 16
    assert ((key >> 4) == (pos >> 4)).all()
    vp = torch.zeros(B, s_pad, H, 128, dtype=torch.bfloat16)    # +0.0
    vp[:, :S] = v
    return vp[:, key].permute(0, 2, 3, 1).contiguous()          # [B, H, 128, s_pad]


PREP_LAYOUTS = ["dense", "wide", "offset"]


def _prep_run(S, form, layout):
    """one prep launch (form: "qk" = qk_norm_rope_vt with weights + RoPE, "k" = k_norm_rope_vt with a vt, "k_only" = with vt = None) under a
    layout -> (storage before, storage after, vt or None, (ld, off)), on the host.  Batch b lies at b * S * ld from the view's start."""
    from domain_rag_amd import ops
    B, H, s_txt = 2, 2, 24
    D = H * 128
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(77 + S)
    qkv = torch.randn(B, S, 3 * D, generator=g).bfloat16()
    w = [(1 + 0.1 * torch.randn(128, generator=g)).bfloat16().to(dev) for _ in range(4)]
    ang = torch.rand(S, 64, generator=g) * 6.28
    cos, sin = torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev)
    ld, off = {"dense": (3 * D, 0), "wide": (3 * D + 72, 0), "offset": (136 + 3 * D + 72, 136)}[layout]
    store = _sentinel(off + (B * S - 1) * ld + 3 * D + (0 if layout == "dense" else 40), dev)
    _strided(store, (B * S, 3 * D), (ld, 1), off).copy_(qkv.view(B * S, 3 * D))
    before = store.cpu()
    view = store[off:]
    assert view.data_ptr() % 16 == 0 and ld % 8 == 0
    s_pad = (S + 63) // 64 * 64
    vt = None if form == "k_only" else _sentinel(B * H * 128 * s_pad, dev).view(B, H, 128, s_pad)
    if form == "qk":
        ops.qk_norm_rope_vt(view, vt, w[0], w[1], w[2], w[3], cos, sin, B, S, H, ld, s_txt)
    else:
        ops.k_norm_rope_vt(view, vt, w[1], w[3], cos, sin, B, S, H, ld, s_txt)
    torch.cuda.synchronize()
    return before, store.cpu(), None if vt is None else vt.cpu(), (ld, off), qkv


@functools.lru_cache(maxsize=None)
def _prep_dense(S, form):
    return _prep_run(S, form, "dense")


@pytest.mark.parametrize("layout", PREP_LAYOUTS)
@pytest.mark.parametrize("form", ["qk", "k", "k_only"])
@pytest.mark.parametrize("S", [70, 200])
def test_prep_pass_layouts_and_the_exact_vt_image(gpu, S, form, layout):
    """q, k and V^T equal the dense run's bits; v and every gap column keep theirs; k_norm_rope_vt leaves q alone; and the whole
    [B, H, 128, s_pad] image — the permutation inside each group of 16 keys, the last partial group, the zero padding — equals the host-built
    tensor bit for bit, under every layout"""
    B, H = 2, 2
    D = H * 128
    _, dense_after, _, _, qkv = _prep_dense(S, form)
    before, after, vt, (ld, off), qkv2 = _prep_run(S, form, layout)
    assert torch.equal(qkv, qkv2)
    dense_rows = dense_after.view(B * S, 3 * D)
    assert torch.equal(_bits(dense_rows[:, 2 * D:]), _bits(qkv.view(B * S, 3 * D)[:, 2 * D:])), "dense run: v must be untouched"
    if form != "qk":
        assert torch.equal(_bits(dense_rows[:, :D]), _bits(qkv.view(B * S, 3 * D)[:, :D])), "dense run: k_norm_rope_vt leaves q as projected"
    else:
        assert not torch.equal(_bits(dense_rows[:, :D]), _bits(qkv.view(B * S, 3 * D)[:, :D]))
    assert not torch.equal(_bits(dense_rows[:, D:2 * D]), _bits(qkv.view(B * S, 3 * D)[:, D:2 * D]))
    # the storage after the launch = the storage before it with the dense run's q | k in place: v, the gap columns, the elements in front of an
    # offset view and behind the last row all keep their bits
    want = before.clone()
    _strided(want, (B * S, 2 * D), (ld, 1), off).copy_(dense_rows[:, :2 * D])
    ne = (_bits(after) != _bits(want)).nonzero()
    if ne.numel():
        o = ne[0].item() - off
        pytest.fail(f"{form} S={S} {layout}: {ne.shape[0]} elements differ, first at row {o // ld} (b = {o // ld // S}, s = {o // ld % S}), column {o % ld}")
    if form == "k_only":
        return
    want_vt = _vt_expected(qkv.view(B, S, 3, H, 128)[:, :, 2], S)
    at = _first_diff(vt, want_vt)
    assert at is None, f"{form} S={S} {layout}: V^T differs from the host-built image first at (b, h, d, position) = {at}"


# ------------------------------------------------------------------ refusals
def test_operands_that_do_not_fit_are_refused_before_any_launch(gpu):
    """a wrong stride or a short buffer is an error, not a memory fault: every case raises (ValueError from the wrapper, RuntimeError where
    the library reports), and nothing was launched — the outputs still hold the sentinel, the inputs their bits"""
    from domain_rag_amd import ops
    B, S, H, s_txt = 2, 70, 2, 24
    D = H * 128
    s_pad = 128
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, S, 3 * D, generator=g).bfloat16().to(gpu)
    qkv0 = qkv.clone()
    flat = qkv.view(-1)
    w = (1 + 0.1 * torch.randn(128, generator=g)).bfloat16().to(gpu)
    cos, sin = torch.rand(S, 64, generator=g).to(gpu), torch.rand(S, 64, generator=g).to(gpu)
    vt = _sentinel(B * H * 128 * s_pad, gpu).view(B, H, 128, s_pad)
    vt_short = _sentinel(B * H * 128 * S, gpu).view(B, H, 128, S)             # S, not s_pad
    out = _sentinel(B * S * D, gpu)
    out_short = _sentinel((B * S - 1) * D, gpu)                                 # one row short
    out_wide = _sentinel(B * S * 5 * D, gpu)
    cos_short = cos[: S - 1].clone()
    dense = (B, S, H, 3 * D, S * 3 * D, D, S * D, SCALE)
    prep = (w, w, cos, sin, s_txt)
    cases = {
        "vt of S columns (attention)": lambda: ops.attention(flat, flat[D:], vt_short, out, *dense),
        "vt of S columns (prep)": lambda: ops.qk_norm_rope_vt(qkv, vt_short, w, w, w, w, cos, sin, B, S, H, 3 * D, s_txt),
        "vt of S columns (k prep)": lambda: ops.k_norm_rope_vt(qkv, vt_short, w, w, cos, sin, B, S, H, 3 * D, s_txt),
        "out one row short": lambda: ops.attention(flat, flat[D:], vt, out_short, *dense),
        "out one row short (row-major v)": lambda: ops.attention_v(flat, flat[D:], flat[2 * D:], out_short, *dense),
        "ld_o = D - 8": lambda: ops.attention(flat, flat[D:], vt, out_wide, B, S, H, 3 * D, S * 3 * D, D - 8, S * D, SCALE),
        "cos of S - 1 rows (q prep)": lambda: ops.attention_qprep(flat, flat[D:], vt, out, *dense, w, w, cos_short, sin, s_txt),
        "cos of S - 1 rows (prep)": lambda: ops.k_norm_rope_vt(qkv, vt, w, w, cos_short, sin, B, S, H, 3 * D, s_txt),
        "k one element short": lambda: ops.attention(flat, flat[2 * D + 1:], vt, out, *dense),
        "v one element short": lambda: ops.attention_v(flat, flat[D:], flat[2 * D + 1:], out, *dense),
        "qkv one row short (prep)": lambda: ops.qk_norm_rope_vt(flat[: (B * S - 1) * 3 * D].clone(), vt, w, w, w, w, cos, sin, B, S, H, 3 * D, s_txt),
        "ld beyond the buffer (prep)": lambda: ops.k_norm_rope_vt(qkv, vt, w, w, cos, sin, B, S, H, 3 * D + 8, s_txt),
        "negative ld_qk": lambda: ops.attention(flat, flat[D:], vt, out, B, S, H, -3 * D, S * 3 * D, D, S * D, SCALE),
        "negative o_batch_stride": lambda: ops.attention_qprep(flat, flat[D:], vt, out, B, S, H, 3 * D, S * 3 * D, D, -S * D, SCALE, *prep),
        "negative ld (prep)": lambda: ops.qk_norm_rope_vt(qkv, vt, w, w, w, w, cos, sin, B, S, H, -3 * D, s_txt),
        "a host weight (q prep)": lambda: ops.attention_qprep(flat, flat[D:], vt, out, *dense, w.cpu(), w, cos, sin, s_txt),
        "a host weight (prep)": lambda: ops.k_norm_rope_vt(qkv, vt, w, w.cpu(), cos, sin, B, S, H, 3 * D, s_txt),
        "a bf16 RoPE table": lambda: ops.attention_v(flat, flat[D:], flat[2 * D:], out, *dense, w, w, cos.bfloat16(), sin, s_txt),
    }
    for what, call in cases.items():
        with pytest.raises((ValueError, RuntimeError)):
            call()
            pytest.fail(f"{what}: not refused")
    torch.cuda.synchronize()
    for t in (vt, vt_short, out, out_short, out_wide):
        assert (_bits(t) == SENT).all(), "a refused call launched something"
    assert torch.equal(_bits(qkv), _bits(qkv0)), "a refused call launched something"
    # ... and the same operands, sized right, are accepted
    ops.k_norm_rope_vt(qkv, vt, w, w, cos, sin, B, S, H, 3 * D, s_txt)
    ops.attention_qprep(flat, flat[D:], vt, out, *dense, *prep)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
