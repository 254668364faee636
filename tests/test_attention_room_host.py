"""``ops._attention_reach`` — the element count that the head_dim-128 attention wrappers compare with an operand's storage before they launch —
against every address enumerated by brute force, on small shapes with padded and offset strides (no GPU, no library)."""
import itertools

import pytest

SHAPES = [(B, S, H) for B in (1, 2, 3) for S in (1, 2, 5) for H in (1, 2)]


def _reach(*a, **kw):
    from domain_rag_amd import ops
    return ops._attention_reach(*a, **kw)


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_rows_reach_is_the_largest_address_plus_one(B, S, H):
    """q, k, row-major v and out: token s of batch b at b * batch_stride + s * ld, head h at + 128 h, element d at + d"""
    D = H * 128
    for ld in (D, D + 8, D + 24, 3 * D, 3 * D + 72, 5 * D):
        # dense, padded between batches, odd paddings (out's batch stride need only be a multiple of 4), batches closer than their rows (reads)
        for bs in (S * ld, S * ld + 4, (S + 3) * ld, (S + 2) * ld + 8, 0, ld):
            top = max(b * bs + s * ld + h * 128 + d for b in range(B) for s in range(S) for h in range(H) for d in (0, 127))
            assert _reach("rows", B, S, H, ld, bs) == top + 1, (ld, bs)


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_prep_reach_is_the_largest_address_plus_one(B, S, H):
    """the prep pass's qkv: batch b at b * S * ld (no batch stride of its own), q | k | v of head h at + which * H * 128 + 128 h"""
    D = H * 128
    for ld in (3 * D, 3 * D + 72, 136 + 3 * D + 72):
        top = max((b * S + s) * ld + which * D + h * 128 + d
                  for b in range(B) for s in range(S) for which in range(3) for h in range(H) for d in (0, 127))
        assert _reach("prep", B, S, H, ld) == top + 1, ld


@pytest.mark.parametrize("S,s_pad", [(1, 64), (63, 64), (64, 64), (65, 128), (70, 128), (200, 256)])
def test_vt_reach_rounds_s_up_to_64(S, s_pad):
    """V^T [B, H, 128, s_pad]: every position of every row is written, the padding included"""
    for B, H in itertools.product((1, 2, 3), (1, 2)):
        top = max(((b * H + h) * 128 + d) * s_pad + pos for b in range(B) for h in range(H) for d in (0, 127) for pos in (0, s_pad - 1))
        assert _reach("vt", B, S, H) == top + 1 == B * H * 128 * s_pad


def test_table_and_weight_reach():
    for S in (1, 2, 5, 64, 65):
        assert _reach("rope", 2, S, 2) == max(s * 64 + j for s in range(S) for j in range(64)) + 1       # f32 [S, 64]
    assert _reach("norm", 3, 5, 2) == 128                                                            # bf16 [128], whatever the shape
    with pytest.raises(KeyError):
        _reach("no such operand", 1, 1, 1)


def test_views_the_callers_pass_have_exactly_the_room_they_reach():
    """flux.py, vit.py and the tests pass k and v as qkv.view(-1)[D:] / [2D:] of a dense [B, S, 3D]: v's room is exactly its reach"""
    for B, S, H in SHAPES:
        D = H * 128
        total = B * S * 3 * D
        reach = _reach("rows", B, S, H, 3 * D, S * 3 * D)
        assert reach <= total - D and reach == total - 2 * D       # k (offset D) has room to spare, v (offset 2 D) exactly its reach
        assert _reach("prep", B, S, H, 3 * D) == total


def test_room_check_on_host_tensors():
    """``ops._attention_room`` itself, on CPU tensors (it reads storage sizes and offsets only): the layouts the callers use pass, one
    element short raises"""
    import torch
    from domain_rag_amd import ops
    B, S, H = 2, 5, 2
    D = H * 128
    s_pad = 64
    qkv = torch.zeros(B, S, 3 * D, dtype=torch.bfloat16)
    out = torch.zeros(B, S, D, dtype=torch.bfloat16)
    vt = torch.zeros(B, H, 128, s_pad, dtype=torch.bfloat16)

    def short(n):         # (room is the STORAGE behind a view: a slice of a large enough tensor has all of it, a short allocation does not)
        return torch.zeros(n, dtype=torch.bfloat16)

    def rows(q=qkv, k=qkv.view(-1)[D:], v=qkv.view(-1)[2 * D:], o=out, ld_o=D, o_bs=S * D, ld=3 * D, bs=S * 3 * D):
        return (("q", q, ld, bs), ("k", k, ld, bs), ("v", v, ld, bs), ("out", o, ld_o, o_bs))
    ops._attention_room("t", B, S, H, rows=rows(), vt=vt, prep=(qkv, 3 * D))
    ops._attention_room("t", 0, S, H, rows=rows(o=out[:1]), vt=vt[:1])                 # a shape the library refuses is the library's to report
    cat = torch.zeros(B, S, 5 * D, dtype=torch.bfloat16)                                # the single-stream blocks' concatenated buffer
    ops._attention_room("t", B, S, H, rows=rows(o=cat, ld_o=5 * D, o_bs=S * 5 * D), vt=vt)
    for bad, match in ((dict(rows=rows(v=qkv.view(-1)[2 * D + 1:])), r"t\.v"), (dict(rows=rows(k=qkv.view(-1)[2 * D + 8:])), r"t\.k"),
                       (dict(rows=rows(o=short(B * S * D - 1))), r"t\.out"), (dict(rows=rows(o=short((B * S - 1) * D))), r"t\.out"),
                       (dict(rows=rows(o=cat, ld_o=D - 8, o_bs=S * D)), "overlap"), (dict(rows=rows(ld=-3 * D)), "negative"),
                       (dict(rows=rows(o_bs=-S * D)), "negative"), (dict(rows=rows(), vt=short(B * H * 128 * S)), r"t\.vt"),
                       (dict(rows=rows(), vt=vt.view(-1)[1:]), r"t\.vt"), (dict(prep=(qkv.view(-1)[8:], 3 * D)), r"t\.qkv"),
                       (dict(prep=(qkv, 3 * D + 8)), r"t\.qkv"), (dict(prep=(qkv, -8)), "negative")):
        with pytest.raises(ValueError, match=match):
            ops._attention_room("t", B, S, H, **bad)
    # optional operands: a GPU tensor of the dtype (a host tensor is refused before its size is looked at), then the size
    cos = torch.zeros(S, 64)
    w = torch.zeros(128, dtype=torch.bfloat16)
    for bad in (dict(ropes=(("rope_cos", cos),)), dict(norms=(("wq_txt", w),)), dict(norms=(("wq_txt", [1.0] * 128),))):
        with pytest.raises(ValueError, match="expected a GPU"):
            ops._attention_room("t", B, S, H, **bad)
