"""The GPU JPEG writer (csrc/jpeg_enc.hip through ``jpeg.encode``) against Pillow itself: every file is the bytes ``Image.save``
writes for the same pixels (lama_inpaint/lama_inpaint.py:211 writes the stage-0 frames that way and stages 1 and 2 read them back).
The shared arithmetic is checked on the host in tests/test_jpeg_enc_core_host.py; here the kernels run: the block / dummy-block
geometry, the scans, the bit packing across block boundaries, the byte stuffing, batches and the cached work buffers."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (8, 8), (16, 16), (17, 9), (9, 17), (33, 17), (16, 1), (40, 24), (24, 40), (30, 22), (72, 48), (101, 77)]   # (W, H)
QUALITIES = (1, 10, 75, 95, 100)


def natural_image(rng, h, w):
    """smooth colour fields + noise: exercises long and short Huffman codes, EOB and ZRL runs"""
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-20, 20, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def contents(rng, h, w):
    """uint8 [5, h, w, 3]: natural, noise (long codes, stuffed 0xFF bytes), flat (EOB-only blocks), 8-pixel stripes of 0 / 255
    (DC category 11, large AC), 128 +- 3 checker (ZRL runs)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([
        natural_image(rng, h, w),
        rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
        np.full((h, w, 3), (200, 30, 90), np.uint8),
        np.repeat((((xx // 8) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2),
        np.repeat((128 + 3 * (1 - 2 * ((xx + yy) % 2))).astype(np.uint8)[:, :, None], 3, axis=2),
    ])


def pil_bytes(arr, **kw):
    bio = io.BytesIO()
    Image.fromarray(arr).save(bio, "JPEG", **kw)
    return bio.getvalue()


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_is_byte_identical_to_pillow(gpu, size):
    """the matrix of the host test; the five contents of a size travel as one batch of five"""
    from domain_rag_amd import jpeg
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    arr = contents(rng, h, w)
    dev = torch.from_numpy(arr).to(gpu)
    grey = np.ascontiguousarray(arr[:, :, :, 1:2])
    dgrey = torch.from_numpy(grey).to(gpu)
    for sub in (0, 1, 2):
        for q in QUALITIES:
            files = jpeg.encode(dev, quality=q, subsampling=sub)
            assert len(files) == len(arr)
            for i, got in enumerate(files):
                ref = pil_bytes(arr[i], quality=q, subsampling=sub)
                assert got == ref, (size, i, sub, q, len(got), len(ref), first_difference(got, ref))
    for q in (30, 90):
        files = jpeg.encode(dgrey, quality=q)
        for i, got in enumerate(files):
            ref = pil_bytes(grey[i, :, :, 0], quality=q)
            assert got == ref, (size, i, "L", q, first_difference(got, ref))


def test_stage0_sized_frame_and_the_defaults(gpu, tmp_path):
    """one 504 x 376 frame (several workgroups per kernel, more than one round of the scans); ``encode(frame)`` with no settings is
    ``Image.save(path)`` with none"""
    from domain_rag_amd import jpeg
    rng = np.random.default_rng(7)
    arr = natural_image(rng, 376, 504)
    arr[100:200, 300:400] = rng.integers(0, 256, (100, 100, 3), dtype=np.uint8)
    dev = torch.from_numpy(arr).to(gpu)
    Image.fromarray(arr).save(tmp_path / "frame.jpg")
    got = jpeg.encode(dev)
    assert len(got) == 1 and got[0] == (tmp_path / "frame.jpg").read_bytes()
    for sub, q in ((0, 95), (1, 75), (2, 100)):
        assert jpeg.encode(dev, quality=q, subsampling=sub)[0] == pil_bytes(arr, quality=q, subsampling=sub), (sub, q)
    assert b"\xff\x00" in pil_bytes(arr, quality=100, subsampling=2)            # the stuffing path really ran


def test_batch_files_equal_single_files_and_buffer_history(gpu):
    """file i of a batch is image i alone; and n = 1 after n = 3 after n = 1 on another size reproduces the first file (the work
    buffers are cached and regrown: the rule of tests/test_gpu_history.py)"""
    from domain_rag_amd import jpeg
    rng = np.random.default_rng(3)
    arr = np.stack([natural_image(rng, 24, 40), rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), natural_image(rng, 24, 40)])
    other = natural_image(rng, 77, 101)
    dev, dother = torch.from_numpy(arr).to(gpu), torch.from_numpy(other).to(gpu)
    first = jpeg.encode(dev[0])
    assert jpeg.encode(dother)[0] == pil_bytes(other, quality=75, subsampling=2)
    batch = jpeg.encode(dev)
    again = jpeg.encode(dev[0])
    assert first == again and first[0] == pil_bytes(arr[0], quality=75, subsampling=2)
    for i in range(3):
        assert batch[i] == jpeg.encode(dev[i])[0] == pil_bytes(arr[i], quality=75, subsampling=2), i


def test_non_contiguous_views_are_made_dense(gpu):
    from domain_rag_amd import jpeg
    rng = np.random.default_rng(4)
    big = natural_image(rng, 60, 90)
    dbig = torch.from_numpy(big).to(gpu)
    crop = dbig[5:38, 7:58]                                   # 33 x 51 window: row stride 270, not 153
    assert not crop.is_contiguous()
    assert jpeg.encode(crop)[0] == pil_bytes(np.ascontiguousarray(big[5:38, 7:58]), quality=75, subsampling=2)
    chw = dbig.permute(2, 0, 1).contiguous().permute(1, 2, 0)  # [H, W, 3] view of planar storage
    assert not chw.is_contiguous()
    assert jpeg.encode(chw, quality=90, subsampling=0)[0] == pil_bytes(big, quality=90, subsampling=0)
    flipped = dbig.flip(0)[::2]                               # every other row, bottom up
    assert jpeg.encode(flipped)[0] == pil_bytes(np.ascontiguousarray(big[::-1][::2]), quality=75, subsampling=2)


def test_refusals(gpu):
    from domain_rag_amd import jpeg
    ok = torch.zeros((8, 8, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises((ValueError, RuntimeError)):
        jpeg.encode(torch.zeros((8, 8, 3), dtype=torch.uint8))                      # a CPU tensor
    with pytest.raises((ValueError, RuntimeError)):
        jpeg.encode(ok.float())
    with pytest.raises((ValueError, RuntimeError)):
        jpeg.encode(ok.to(torch.int8))
    for shape in ((8, 8, 4), (8, 8, 2), (2, 8, 8, 4), (8, 8), (1, 2, 8, 8, 3)):
        with pytest.raises((ValueError, RuntimeError)):
            jpeg.encode(torch.zeros(shape, dtype=torch.uint8, device=gpu))
    for q in (0, 101, -1, 75.0, None):
        with pytest.raises((ValueError, RuntimeError)):
            jpeg.encode(ok, quality=q)
    for s in (3, -1, "4:2:0"):
        with pytest.raises((ValueError, RuntimeError)):
            jpeg.encode(ok, subsampling=s)
    with pytest.raises((ValueError, RuntimeError)):
        jpeg.encode(torch.zeros((4097, 4096, 1), dtype=torch.uint8, device=gpu))     # more than 2^24 pixels
    assert jpeg.encode(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=gpu)) == []
    assert jpeg.encode(ok)[0] == pil_bytes(np.zeros((8, 8, 3), np.uint8), quality=75, subsampling=2)      # still in working order


def test_own_files_decode_on_the_device_like_pil(gpu):
    """writer -> reader: ``jpeg.decode_files`` on the encoder's files gives the pixels PIL decodes from them"""
    from domain_rag_amd import jpeg
    rng = np.random.default_rng(9)
    arr = np.stack([natural_image(rng, 48, 72), rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)])
    dev = torch.from_numpy(arr).to(gpu)
    files = []
    for sub, q in ((0, 90), (1, 60), (2, 75)):
        files += jpeg.encode(dev, quality=q, subsampling=sub)
    files += jpeg.encode(dev[:, :, :, :1].contiguous(), quality=80)
    one_grey = jpeg.encode(dev[0, :, :, 1:2], quality=80)            # the [H, W, 1] form (a strided view): ONE grey image
    assert one_grey == [pil_bytes(np.ascontiguousarray(arr[0, :, :, 1]), quality=80)]
    files += one_grey
    dec = jpeg.decode_files(files, gpu)
    for i, f in enumerate(files):
        assert int(dec.status[i]) == 0, (i, int(dec.status[i]))
        assert np.array_equal(dec.image(i).cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))), i
