"""csrc/jpeg_enc_core.h compiled for the HOST (tests/helpers/jpeg_enc_host.cpp: a serial composition of the functions the gfx950
kernels of csrc/jpeg_enc.hip run) against Pillow's own writer: colour conversion, edge replication, downsampling, ISLOW forward DCT,
quantisation, the Annex K tables, entropy coding, byte stuffing and the header must reproduce ``Image.save`` BYTE FOR BYTE, or the
stage-0 .jpg files (lama_inpaint/lama_inpaint.py:211) that stages 1 and 2 read stop being the reference's.  The kernels
themselves are compared with Pillow in tests/test_gpu_jpeg_encode.py; this file checks the shared arithmetic where there is no GPU."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (8, 8), (16, 16), (17, 9), (9, 17), (33, 17), (16, 1), (40, 24), (24, 40), (30, 22), (72, 48), (101, 77)]   # (W, H)
QUALITIES = (1, 10, 75, 95, 100)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jpeg_enc_host") / "libjpeg_enc_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, os.path.join(ROOT, "tests", "helpers", "jpeg_enc_host.cpp")],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.jpeg_enc_host_encode.restype = ctypes.c_int64
    lib.jpeg_enc_host_encode.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int64]
    lib.jpeg_enc_host_quant_zigzag.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def natural_image(rng, h, w):
    """smooth colour fields + noise: exercises long and short Huffman codes, EOB and ZRL runs"""
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-20, 20, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def contents(rng, h, w):
    """name -> uint8 [h, w, 3]"""
    yy, xx = np.mgrid[0:h, 0:w]
    return {
        "natural": natural_image(rng, h, w),
        "noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),                                   # long codes, stuffed 0xFF bytes
        "flat": np.full((h, w, 3), (200, 30, 90), np.uint8),                                         # EOB-only blocks, zero DC differences
        "stripes": np.repeat((((xx // 8) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2),       # DC category 11, large AC (quality 100)
        "checker": np.repeat((128 + 3 * (1 - 2 * ((xx + yy) % 2))).astype(np.uint8)[:, :, None], 3, axis=2),   # only the last zigzag coefficient
    }


def pil_bytes(arr, **kw):
    bio = io.BytesIO()
    Image.fromarray(arr).save(bio, "JPEG", **kw)
    return bio.getvalue()


def host_bytes(host, arr, quality, subsampling):
    arr = np.ascontiguousarray(arr)
    h, w = arr.shape[:2]
    c = 1 if arr.ndim == 2 else 3
    out = np.zeros(4096 + 16 * h * w + 4096, np.uint8)
    n = host.jpeg_enc_host_encode(arr.ctypes.data, h, w, c, quality, subsampling, out.ctypes.data, out.size)
    assert n > 0, n
    return out[:n].tobytes()


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


@pytest.mark.parametrize("size", SIZES + [(500, 375)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_is_byte_identical_to_pillow(host, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    images = contents(rng, h, w)
    if size == (500, 375):
        images = {"natural": images["natural"]}               # one large frame
    for name, arr in images.items():
        for sub in (0, 1, 2):
            for q in QUALITIES:
                ref = pil_bytes(arr, quality=q, subsampling=sub)
                got = host_bytes(host, arr, q, sub)
                assert got == ref, (size, name, sub, q, len(got), len(ref), first_difference(got, ref))
        for q in (30, 90):
            grey = np.ascontiguousarray(arr[:, :, 1])
            ref = pil_bytes(grey, quality=q)
            got = host_bytes(host, grey, q, 2)                # subsampling is ignored for grey
            assert got == ref, (size, name, "L", q, first_difference(got, ref))


def test_contents_reach_the_coder_paths_they_are_meant_for():
    """a check of the FIXTURES, not of the encoder (only Pillow runs here): the reference files themselves show that the contents
    above exercise what they claim: stuffed bytes for noise, ZRL codes for the checker (a lone last coefficient behind 62 zeros
    needs three)"""
    rng = np.random.default_rng(5)
    c = contents(rng, 48, 72)
    noise = pil_bytes(c["noise"], quality=95, subsampling=0)
    sos = noise.index(b"\xff\xda")
    assert b"\xff\x00" in noise[sos:]
    # the grey checker at quality 90 (one of the grey cases above): DC difference 0 (the mean is 128), then ZRL ZRL ZRL and the
    # (14, size) code of coefficient 63 -- the only AC coefficient that survives that table -- and no EOB
    chk = pil_bytes(np.ascontiguousarray(c["checker"][:8, :8, 1]), quality=90)
    scan = chk[chk.index(b"\xff\xda") + 10: -2]
    bits = "".join(f"{b:08b}" for b in scan.replace(b"\xff\x00", b"\xff"))
    assert bits[:2] == "00" and bits[2:2 + 33] == "11111111001" * 3, bits[:48]


def test_default_save_is_quality_75_subsampling_420(host, tmp_path):
    """``Image.save(path)`` with no arguments on a .jpg name: the defaults stage 0 relies on (result.save(output_filename))"""
    rng = np.random.default_rng(11)
    for (w, h) in ((72, 48), (33, 17)):
        arr = natural_image(rng, h, w)
        for name in ("a.jpg", "b.JPEG", "c.jpe", "d.jfif"):
            Image.fromarray(arr).save(tmp_path / name)
            assert (tmp_path / name).read_bytes() == host_bytes(host, arr, 75, 2), (w, h, name)


def test_quality_scaled_tables_match_pillows_dqt_segments(host):
    arr = np.zeros((8, 8, 3), np.uint8)
    got = np.zeros(64, np.uint8)
    for q in range(1, 101):
        data = pil_bytes(arr, quality=q, subsampling=0)
        pos = 0
        for which in (0, 1):
            pos = data.index(b"\xff\xdb", pos)
            assert data[pos + 2: pos + 5] == bytes([0, 67, which])
            host.jpeg_enc_host_quant_zigzag(which, q, got.ctypes.data)
            assert got.tobytes() == data[pos + 5: pos + 69], (q, which)
            pos += 69


def test_bad_arguments_are_refused(host):
    a = np.zeros((8, 8, 3), np.uint8)
    out = np.zeros(4096, np.uint8)
    enc = host.jpeg_enc_host_encode
    assert enc(a.ctypes.data, 8, 8, 3, 0, 2, out.ctypes.data, out.size) == -1
    assert enc(a.ctypes.data, 8, 8, 3, 101, 2, out.ctypes.data, out.size) == -1
    assert enc(a.ctypes.data, 8, 8, 2, 75, 2, out.ctypes.data, out.size) == -1
    assert enc(a.ctypes.data, 8, 8, 3, 75, 3, out.ctypes.data, out.size) == -1
    assert enc(a.ctypes.data, 8, 8, 3, 75, 2, out.ctypes.data, 100) == -2


def test_core_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """random sizes (1 .. 70), settings and contents (noise, 0 / 255 only, flat, stripes) through the same composition, built with
    -fsanitize=address,undefined: no access outside a buffer, no undefined arithmetic, no block above the reserved stream size"""
    flags = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")          # decided on an empty program, before any project code is compiled
    exe = str(tmp_path / "jpeg_enc_sanitize")
    r = subprocess.run(flags + ["-o", exe, os.path.join(ROOT, "tests", "helpers", "jpeg_enc_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "iterations 300" in r.stdout
