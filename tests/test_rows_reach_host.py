"""``ops._rows_reach`` — the element count that every wrapper with a batched-row map compares with an operand's storage before it launches —
against every address enumerated by brute force, and ``ops._fit``, the comparison itself, on CPU tensors (no GPU, no library)."""
import pytest

SHAPES = [(B, S, H) for B in (1, 2, 3) for S in (1, 2, 5) for H in (1, 2)]         # those of test_attention_room_host.py


def _reach(*a, **kw):
    from domain_rag_amd import ops
    return ops._rows_reach(*a, **kw)


def _addresses(M, cols, ld, rows_per_batch, batch_stride):
    """the library's rule (``drag_gemm_bf16``, ``drag_quantize_mxfp8``): row r of M at (r // rpb) * batch_stride + (r % rpb) * ld"""
    rpb = rows_per_batch if 0 < rows_per_batch < M else M
    return [(r // rpb) * batch_stride + (r % rpb) * ld + c for r in range(M) for c in range(cols)]


@pytest.mark.parametrize("M", range(1, 8))
def test_rows_reach_is_the_largest_address_plus_one(M):
    """dense and padded rows; one batch, full batches, a short last batch; batches apart, touching, overlapping and on top of each other"""
    for cols in (1, 8):
        for ld in (cols, cols + 8, 3 * cols):
            for rows_per_batch in (0, 1, 2, 3, 4, M, M + 1):
                rpb = rows_per_batch if 0 < rows_per_batch < M else M
                for batch_stride in (0, 8, ld, rpb * ld, rpb * ld + 8, (rpb + 2) * ld):
                    top = max(_addresses(M, cols, ld, rows_per_batch, batch_stride))
                    assert _reach(M, cols, ld, rows_per_batch, batch_stride) == top + 1, (cols, ld, rows_per_batch, batch_stride)


def test_short_last_batch_reaches_as_far_as_the_full_batch_before_it():
    """five rows in batches of four, the batches 8 elements apart: row 3 of batch 0 ends at element 512, the last row (row 0 of batch 1) at 136"""
    assert _reach(5, 128, 128, 4, 8) == 512
    assert max(_addresses(5, 128, 128, 4, 8)) + 1 == 512


def test_nothing_to_address():
    for M, cols in ((0, 8), (-1, 8), (3, 0), (3, -8)):
        assert _reach(M, cols, 8, 2, 64) == 0


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_attention_rows_and_prep_are_row_maps(B, S, H):
    """``_attention_reach``'s "rows" = B * S rows of H * 128 in batches of S; "prep" = B * S rows of 3 * H * 128 in one batch"""
    from domain_rag_amd import ops
    D = H * 128
    for ld in (D, D + 8, 3 * D, 3 * D + 72):
        for bs in (S * ld, S * ld + 4, (S + 3) * ld, 0, ld):
            assert ops._attention_reach("rows", B, S, H, ld, bs) == _reach(B * S, D, ld, S, bs)
        assert ops._attention_reach("prep", B, S, H, ld) == _reach(B * S, 3 * D, ld)


def test_fit_on_host_tensors():
    """room is the STORAGE behind a view, from the view's first element on: a view of exactly its reach passes, one element short raises, a
    slice of a larger tensor has all that follows it"""
    import torch
    from domain_rag_amd import ops
    M, cols, ld, rpb, bs = 5, 8, 16, 4, 72
    reach = _reach(M, cols, ld, rpb, bs)
    assert reach == 80
    ops._fit(torch.zeros(reach, dtype=torch.bfloat16), reach, "t.x", M, cols, ld, rpb, bs)
    with pytest.raises(ValueError, match=r"t\.x.* 80 .* 79"):
        ops._fit(torch.zeros(reach - 1, dtype=torch.bfloat16), reach, "t.x", M, cols, ld, rpb, bs)
    big = torch.zeros(reach + 24, dtype=torch.float32)
    ops._fit(big[:3], reach, "t.x")                             # three elements by its shape, the whole storage by its room
    ops._fit(big[24:], reach, "t.x")
    with pytest.raises(ValueError, match=r"t\.x"):
        ops._fit(big[25:], reach, "t.x")
    ops._fit(big, 0, "t.x")
