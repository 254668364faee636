"""csrc/jpeg_par_core.h compiled for the HOST (tests/helpers/jpeg_par_host.cpp): the parallel entropy route — subsequences, Jacobi
rounds to the fixed point, count scan, writing pass, DC pass, fallback to the lane decoder — must give PIL's bytes for clean files
WITHOUT falling back, and the lane decoder's status, scan flag and pixels for everything else.  The gfx950 kernels of
csrc/jpeg_par.hip run the same functions (tests/test_gpu_jpeg_parallel.py); this file checks them where there is no GPU, with
subsequence sizes down to 4 bytes so that every boundary case (a boundary on a stuffed zero, on the 0xFF before one, inside an RSTn,
symbols longer than a subsequence) occurs in small files."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "helpers")
BIG = 1 << 20          # a round cap that never binds: the small geometries need more rounds than the product's cap allows


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jpeg_par_host") / "libjpeg_par_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, os.path.join(HELPERS, "jpeg_par_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.jpeg_par_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.jpeg_par_host_geometry.argtypes = [ctypes.c_void_p] * 3
    return lib


@pytest.fixture(scope="module")
def geometry(host):
    g = (ctypes.c_int32 * 3)()
    host.jpeg_par_host_geometry(ctypes.byref(g, 0), ctypes.byref(g, 4), ctypes.byref(g, 8))
    return int(g[0]), int(g[1]), int(g[2])          # S, span, round cap


def natural_image(rng, h, w):
    """smooth colour fields + noise: long and short Huffman codes, EOB and ZRL runs"""
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-20, 20, (h, w, 3))
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))


def encode(im, **kw):
    from PIL import ImageFile
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, im.size[0] * im.size[1] * 4)
    bio = io.BytesIO()
    im.save(bio, "JPEG", **kw)
    return bio.getvalue()


def decode(host, data, S, span, cap, mode=1, shape=None):
    """-> (status, stats[6] = route, rounds, subsequences, reason, scan flag, local iterations; pixels)"""
    if shape is None:
        w, h = Image.open(io.BytesIO(data)).size
        shape = (h, w, 3)
    out = np.zeros(shape, np.uint8)
    stats = np.zeros(6, np.int32)
    st = host.jpeg_par_host_decode(data, len(data), S, span, cap, mode, out.ctypes.data, out.size, stats.ctypes.data)
    return st, stats, out


def scan_offset(data):
    i = data.index(b"\xff\xda")
    return i + 2 + int.from_bytes(data[i + 2: i + 4], "big")


def boundary_kinds(data, S):
    """what the subsequence boundaries of this file fall on, found from the bytes"""
    off = scan_offset(data)
    kinds = set()
    for b in range(off + S, len(data) - 2, S):
        if data[b] == 0 and data[b - 1] == 0xFF:
            kinds.add("stuffed zero")
        if data[b] == 0xFF and data[b + 1] == 0:
            kinds.add("0xFF before a stuffed zero")
        if data[b - 1] == 0xFF and 0xD0 <= data[b] <= 0xD7:
            kinds.add("inside RSTn")
    return kinds


SIZES = [(8, 8), (16, 1), (5, 3), (33, 17), (101, 77), (504, 376)]


def matrix(size):
    """(label, file bytes) over subsampling x quality, optimised tables, restart intervals and grey for one size"""
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    im = natural_image(rng, h, w)
    subs = (0,) if w <= 4 else (0, 1, 2)
    for sub in subs:
        for q in (10, 75, 95, 100):
            yield f"sub{sub} q{q}", encode(im, quality=q, subsampling=sub)
        yield f"sub{sub} optimize", encode(im, quality=85, subsampling=sub, optimize=True)
    for kw in ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
        for sub in (subs[0], subs[-1]):
            data = encode(im, quality=80, subsampling=sub, **kw)
            assert b"\xff\xdd" in data, "this Pillow does not write restart markers"
            yield f"sub{sub} {kw}", data
    for q in (10, 75, 100):
        yield f"grey q{q}", encode(im.convert("L"), quality=q)
    yield "grey restart", encode(im.convert("L"), quality=75, restart_marker_blocks=3)


@pytest.mark.parametrize("size", SIZES)
def test_parallel_route_is_byte_identical_to_pil_without_fallback(host, geometry, size):
    S0, span0, cap0 = geometry
    worst = 0
    for label, data in matrix(size):
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        geoms = [(S, span, BIG) for S in (4, 16, S0) for span in (2, span0)]
        geoms.append((S0, span0, cap0))                                    # the product geometry under the product cap
        for S, span, cap in geoms:
            st, stats, out = decode(host, data, S, span, cap, shape=ref.shape)
            assert st == 0, (size, label, S, span, st)
            assert stats[0] == 1 and stats[3] == 0, (size, label, S, span, "fell back", stats.tolist())
            assert stats[4] == 0, (size, label, S, span, "scan flag")
            assert np.array_equal(out, ref), (size, label, S, span)
            if cap == cap0:
                worst = max(worst, int(stats[1]))
    print(f"{size}: most cross-span rounds at the product geometry: {worst}")
    assert worst <= cap0


@pytest.mark.parametrize("S", [4, 16, "product"])
def test_boundary_cases_really_occur(host, geometry, S):
    """a subsequence boundary on a stuffed zero, on the 0xFF before one and inside an RSTn: found from the bytes, asserted, decoded"""
    product = S == "product"
    S = geometry[0] if product else S
    rng = np.random.default_rng(11)
    # files large enough for their subsequence size: a boundary hits a given byte pair once in S boundaries
    pw, ph = (504, 376) if product else (101, 77)
    plain = encode(natural_image(rng, ph, pw), quality=100, subsampling=0)
    assert plain.count(b"\xff\x00") > 50
    assert {"stuffed zero", "0xFF before a stuffed zero"} <= boundary_kinds(plain, S), (S, boundary_kinds(plain, S))
    rw, rh = (504, 376) if product else (64, 48)
    rst = encode(natural_image(rng, rh, rw), quality=95, subsampling=0, restart_marker_blocks=1)
    assert "inside RSTn" in boundary_kinds(rst, S), (S, boundary_kinds(rst, S))
    for data in (plain, rst):
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        for span in (2, geometry[1]):
            st, stats, out = decode(host, data, S, span, BIG, shape=ref.shape)
            assert st == 0 and stats[0] == 1 and np.array_equal(out, ref), (S, span, stats.tolist())


def test_symbols_longer_than_a_subsequence_occur(host):
    """at S = 4 some subsequence holds no symbol start at all (a 16-bit code + 15 extra bits spans it): its entry is its exit"""
    rng = np.random.default_rng(12)
    data = encode(Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)), quality=100, subsampling=0)
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    st, stats, out = decode(host, data, 2, 2, BIG, shape=ref.shape)     # 2-byte subsequences: every symbol above 16 bits spans one
    assert st == 0 and stats[0] == 1 and np.array_equal(out, ref)
    st, stats, out = decode(host, data, 4, 2, BIG, shape=ref.shape)
    assert st == 0 and stats[0] == 1 and np.array_equal(out, ref)


def test_forced_fallback_still_gives_pils_bytes(host, geometry):
    """round cap 1 over many spans cannot confirm the fixed point: route 2, reason 8 (round cap), the lane decoder's (= PIL's) bytes"""
    rng = np.random.default_rng(13)
    data = encode(natural_image(rng, 77, 101), quality=75, subsampling=2)
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    st, stats, out = decode(host, data, 16, 2, 1, shape=ref.shape)
    assert st == 0 and stats[0] == 2 and stats[3] == 8, stats.tolist()
    assert stats[4] == 0 and np.array_equal(out, ref)
    st, stats, out = decode(host, data, 16, 2, BIG, shape=ref.shape)
    assert st == 0 and stats[0] == 1 and np.array_equal(out, ref)


def seeds(rng):
    out = []
    for w, h in ((64, 48), (33, 17), (120, 90)):
        for sub in (0, 1, 2):
            for kw in ({}, {"optimize": True}, {"restart_marker_blocks": 2}):
                out.append(encode(natural_image(rng, h, w), quality=int(rng.integers(20, 98)), subsampling=sub, **kw))
        out.append(encode(natural_image(rng, h, w).convert("L"), quality=70))
    return out


def mutate(rng, f):
    """the mutation kinds of tests/helpers/jpeg_fuzz.cpp"""
    f = bytearray(f)
    kind = int(rng.integers(0, 6))
    r = lambda n: int(rng.integers(0, n))
    if kind == 0:
        for _ in range(1 + r(8)):
            f[r(len(f))] = r(256)
    elif kind == 1:
        for _ in range(1 + r(6)):
            f[r(min(len(f), 700))] = r(256)
    elif kind == 2:
        del f[1 + r(len(f)):]
    elif kind == 3:
        for _ in range(1 + r(6)):
            p = len(f) // 2 + r(len(f) // 2)
            f[p] = 0xFF
            if p + 1 < len(f) and r(2):
                f[p + 1] = 0xC0 + r(0x40)
    elif kind == 4:
        a, n = r(len(f)), r(300)
        f = f[:a] + f[a: a + n] + f[a:]
    else:
        for k in range(2, len(f)):
            if r(8) == 0:
                f[k] = r(256)
    return bytes(f)


def test_damaged_files_decode_like_the_lane_decoder(host, geometry):
    """parallel-with-fallback == the sequential host decode on status, scan flag and pixels, for every mutated file"""
    rng = np.random.default_rng(14)
    pool = seeds(rng)
    fell, clean, rejected, reasons = 0, 0, 0, set()
    cap_px = 1 << 20
    for it in range(1500):
        data = mutate(rng, pool[int(rng.integers(0, len(pool)))])
        S, span = [(4, 2), (16, 2), (4, geometry[1]), (geometry[0], geometry[1])][it % 4]
        a = np.zeros(cap_px * 3, np.uint8); b = np.zeros(cap_px * 3, np.uint8)
        sa, sb = np.zeros(6, np.int32), np.zeros(6, np.int32)
        st0 = host.jpeg_par_host_decode(data, len(data), S, span, BIG, 0, a.ctypes.data, a.size, sa.ctypes.data)
        st1 = host.jpeg_par_host_decode(data, len(data), S, span, BIG, 1, b.ctypes.data, b.size, sb.ctypes.data)
        assert st0 == st1, (it, st0, st1)
        if st0 != 0:
            rejected += 1
            continue
        assert sa[4] == sb[4], (it, "scan flag", sa.tolist(), sb.tolist())
        assert np.array_equal(a, b), (it, "pixels", sb.tolist())
        if sb[0] == 2:
            fell += 1
            reasons.add(int(sb[3]))
        else:
            assert sb[0] == 1 and sb[4] == 0, (it, sb.tolist())     # a file the parallel route keeps is one the lane decoder calls clean
            clean += 1
    print(f"rejected {rejected}, parallel {clean}, fell back {fell}, reasons {sorted(reasons)}")
    assert fell > 100 and clean > 20 and len(reasons) >= 4


def test_mutation_fuzz_of_the_parallel_core_under_address_sanitizer(tmp_path, geometry):
    """tests/helpers/jpeg_par_fuzz.cpp (a program of its own, -fsanitize=address,undefined) runs the same mutations through the parallel
    core at S = 4, S = 16 and the product value: no access outside a buffer whatever the bytes are, and the lane decoder's result"""
    exe = str(tmp_path / "jpeg_par_fuzz")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-o", exe,
                        os.path.join(HELPERS, "jpeg_par_fuzz.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-2000:]
    rng = np.random.default_rng(15)
    paths = []
    for k, data in enumerate(seeds(rng)):
        p = tmp_path / f"s{k}.jpg"
        p.write_bytes(data)
        paths.append(str(p))
    r = subprocess.run([exe, "3000"] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "iterations 3000" in r.stdout and "mismatches 0" in r.stdout, r.stdout
    assert int(r.stdout.split("parallel")[1].split(",")[0]) > 100, r.stdout      # (the parallel passes really ran to the end)
