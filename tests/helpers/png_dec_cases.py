"""Case lists shared by tests/test_png_dec_core_host.py (g++ build of csrc/png_dec_core.h) and tests/test_gpu_png_decode.py (the gfx950
kernels): files, each with the status the decoder must give it.  Pillow is the yardstick for pixels everywhere.

Also an INDEPENDENT writer (``huff_png``): a Python bit-writer that emits one final dynamic block of literals with code lengths that
are not the encoder's, a header that uses the code-length symbols 16 / 17 / 18, any HDIST, HCLEN minimal or 19."""
import ctypes
import functools
import io
import os
import struct
import subprocess
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIG = b"\x89PNG\r\n\x1a\n"
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- the g++ build -----------------------------------------------------------------------------------------------------
def build_host(tmpdir) -> ctypes.CDLL:
    so = os.path.join(str(tmpdir), "libpng_dec_host.so")
    h = os.path.join(ROOT, "tests", "helpers")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, os.path.join(h, "png_host.cpp"), os.path.join(h, "png_dec_host.cpp")],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.png_host_encode.restype = ctypes.c_int64
    lib.png_host_encode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]
    lib.png_dec_host_decode.restype = ctypes.c_int
    lib.png_dec_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_void_p]
    lib.png_dec_host_wrap.restype = ctypes.c_int64
    lib.png_dec_host_wrap.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]
    lib.png_dec_host_geometry.argtypes = [ctypes.c_void_p]
    return lib


def host_geometry(lib):
    g = np.zeros(4, np.int32)
    lib.png_dec_host_geometry(g.ctypes.data)
    return tuple(int(v) for v in g)            # S, span, round cap, band


def host_encode(lib, a: np.ndarray) -> bytes:
    """the encoder's file for ``a`` ([H, W, 3] or [H, W]): the serial composition of png_core.h"""
    a = np.ascontiguousarray(a)
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else a.shape[2]
    cap = 2 * a.size + 2 * h + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n = lib.png_host_encode(a.ctypes.data, h, w, c, out.ctypes.data, cap, 256)
    assert n > 0
    return out[:n].tobytes()


def host_wrap(lib, filt: np.ndarray, h: int, w: int, c: int) -> bytes:
    """filtered bytes [h, 1 + w * c] -> a file through png_core.h's own code construction, block header and bit packing"""
    filt = np.ascontiguousarray(filt, dtype=np.uint8)
    cap = 2 * filt.size + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n = lib.png_dec_host_wrap(filt.ctypes.data, h, w, c, out.ctypes.data, cap)
    assert n > 0
    return out[:n].tobytes()


def host_decode(lib, data: bytes, mode: str = "RGB", S: int = None, cap: int = None, span: int = None):
    """-> (status, reason, rounds, nsub, pixels or None); the output sits between guards that must survive"""
    geo = host_geometry(lib)
    S = geo[0] if S is None else S
    cap = geo[2] if cap is None else cap
    span = geo[1] if span is None else span
    info, stats = np.zeros(16, np.int32), np.zeros(4, np.int32)
    guard = 64
    buf = np.full(guard * 2 + (1 << 22), 0xA5, np.uint8)
    st = lib.png_dec_host_decode(data, len(data), S, span, cap, 1 if mode == "RGB" else 0, buf.ctypes.data + guard, buf.size - 2 * guard,
                                 info.ctypes.data, stats.ctypes.data)
    assert st == stats[0]
    h, w, c = int(info[2]), int(info[1]), int(info[3])
    if st != 0:
        assert (buf == 0xA5).all(), "a declined file wrote to the output"
        return st, int(stats[1]), int(stats[2]), int(stats[3]), None
    co = 3 if (c == 3 or mode == "RGB") else 1
    nb = h * w * co
    assert (buf[:guard] == 0xA5).all() and (buf[guard + nb:] == 0xA5).all(), "the decoder wrote outside its output"
    px = buf[guard: guard + nb].copy()
    return 0, 0, int(stats[2]), int(stats[3]), px.reshape((h, w, 3) if co == 3 else (h, w))


def pillow(data: bytes, mode: str = "RGB"):
    """-> (pixels, None) or (None, message): what Pillow makes of the file"""
    try:
        return np.asarray(Image.open(io.BytesIO(data)).convert(mode)), None
    except Exception as e:  # noqa: BLE001
        return None, f"{type(e).__name__}: {e}"


# ---- container helpers -----------------------------------------------------------------------------------------------
def chunk(ctype: bytes, data: bytes, bad_crc: bool = False) -> bytes:
    crc = zlib.crc32(ctype + data) ^ (1 if bad_crc else 0)
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", crc)


def ihdr(w, h, depth=8, ctype=2, interlace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def chunks_of(data: bytes):
    pos, out = 8, []
    while pos + 12 <= len(data):
        n = struct.unpack(">I", data[pos: pos + 4])[0]
        out.append((data[pos + 4: pos + 8], data[pos + 8: pos + 8 + n]))
        pos += 12 + n
    return out


def zstream_of(data: bytes) -> bytes:
    return b"".join(d for t, d in chunks_of(data) if t == b"IDAT")


def rebuild(data: bytes, idat_sizes=None, before=(), between=(), z=None, bad_idat_crc=False) -> bytes:
    """the file with its zlib stream (or ``z``) cut into IDAT chunks of ``idat_sizes`` (cycled; 0 = an empty chunk), ancillary chunks
    ``before`` the first IDAT and ``between`` the first and the second"""
    ch = chunks_of(data)
    z = zstream_of(data) if z is None else z
    out = [SIG, chunk(*ch[0])] + [chunk(t, d) for t, d in before]
    pos, k, first = 0, 0, True
    sizes = list(idat_sizes) if idat_sizes else [len(z)]
    while pos < len(z) or first:
        n = sizes[k % len(sizes)]
        k += 1
        out.append(chunk(b"IDAT", z[pos: pos + n], bad_crc=bad_idat_crc and first))
        pos += n
        if first:
            out += [chunk(t, d) for t, d in between]
            first = False
        if k > 4 * len(z) + 16:
            break
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


# ---- contents ---------------------------------------------------------------------------------------------------------
def photo(h, w, seed, c=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 37.0 + k) * np.cos(yy / 23.0 - k) for k in range(c)], axis=-1)
    a = np.clip(base + rng.normal(0, 6, (h, w, c)), 0, 255).astype(np.uint8)
    return a if c == 3 else a[..., 0].copy()


def content(kind, shape, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "photo":
        return photo(shape[0], shape[1], seed + 3, 3 if len(shape) == 3 else 1)
    if kind == "flat":
        return np.full(shape, 77, dtype=np.uint8)
    return (np.arange(int(np.prod(shape))) % 251).astype(np.uint8).reshape(shape)


ROUND_TRIP_SHAPES = [(1, 1, 3), (1, 7, 3), (5, 1, 3), (37, 53, 3), (64, 64, 3), (65, 130, 3), (200, 333, 3), (17, 19), (1, 1), (128, 96)]
KINDS = ("noise", "photo", "flat", "ramp")


def round_trip_cases(lib):
    """[(name, kind, file)]"""
    return [(f"{kind}{shape}", kind, host_encode(lib, content(kind, shape))) for shape in ROUND_TRIP_SHAPES for kind in KINDS]


# ---- filters (forward, vectorised: every predictor reads ORIGINAL pixels) ------------------------------------------------
def filter_rows(a: np.ndarray, ftypes) -> np.ndarray:
    """a: [H, W, C] uint8; ftypes[y] in 0..4 -> filtered bytes [H, 1 + W * C]"""
    h, w, c = a.shape
    x = a.reshape(h, w * c).astype(np.int32)
    left = np.zeros_like(x); left[:, c:] = x[:, :-c]
    up = np.zeros_like(x); up[1:] = x[:-1]
    ul = np.zeros_like(x); ul[1:, c:] = x[:-1, :-c]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    preds = [np.zeros_like(x), left, up, (left + up) >> 1, paeth]
    out = np.zeros((h, 1 + w * c), np.uint8)
    for y in range(h):
        f = int(ftypes[y])
        out[y, 0] = f
        out[y, 1:] = ((x[y] - preds[f if f < 5 else 0][y]) & 255).astype(np.uint8)
    return out


def tie_content(h, w, c, seed):
    """many Paeth ties: values in 0..3, runs where a = b = c, and wrap-around at 255 -> 0"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (h, w, c)).astype(np.uint8)
    a[::3] = 2                                         # whole rows equal: a = b = c below and beside
    a[:, ::4] = (a[:, ::4] + 253).astype(np.uint8)     # 253..255 and 0: sums wrap
    return a


FILTER_PATTERNS = ["all0", "all1", "all2", "all3", "all4", "cycle"]     # "all3" / "all4" put Average / Paeth on row 0, where up is zero
FILTER_WIDTHS = [1, 2, 3, 64, 65]


def filter_heights(band):
    return [1, 2, band - 1, band, band + 1, 2 * band + 1]


def forced_filter_cases(lib, band):
    """[(name, file)]: png_core.h's own block writer around chosen filter bytes"""
    out = []
    for c in (3, 1):
        for pat in FILTER_PATTERNS:
            for w in FILTER_WIDTHS:
                for h in filter_heights(band):
                    a = tie_content(h, w, c, h * 131 + w * 7 + c)
                    ft = [(y % 5) if pat == "cycle" else int(pat[3]) for y in range(h)]
                    out.append((f"{pat}-{h}x{w}x{c}", host_wrap(lib, filter_rows(a, ft), h, w, c)))
    return out


# ---- the independent writer --------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                               # LSB first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, n):                       # Huffman codes are packed starting with their most significant bit
        self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0
        return bytes(self.out)


def canonical(lens):
    codes, code = {}, 0
    for l in range(1, 16):
        for s, ls in enumerate(lens):
            if ls == l:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def fill_complete(prefix, n):
    """n code lengths: ``prefix`` for the first symbols, the rest 15 bits, shortened from the front until the code is complete"""
    lens = list(prefix) + [15] * (n - len(prefix))
    left = (1 << 15) - sum(1 << (15 - l) for l in lens)
    assert left >= 0
    for i in range(len(prefix), n):
        while lens[i] > 1 and left >= (1 << (15 - lens[i])):
            left -= 1 << (15 - lens[i])
            lens[i] -= 1
    assert left == 0
    return lens


def code_lengths(kind, filtered: bytes):
    """257 lengths by the rank of each byte value in ``filtered`` (most frequent first; the end-of-block symbol where ``kind`` puts it)"""
    cnt = np.bincount(np.frombuffer(filtered, np.uint8), minlength=256)
    rank = [int(s) for s in np.argsort(-cnt, kind="stable")]
    lens = [0] * 257
    if kind == "skew15":                               # 1..7 bits for the seven most frequent values, the tail at 14 / 15 bits; EOB last: 15 bits
        by_rank = fill_complete([1, 2, 3, 4, 5, 6, 7], 257)
        by_rank.sort()
        for l, s in zip(by_rank, rank + [256]):
            lens[s] = l
    elif kind == "flat89":                             # 255 symbols of 8 bits, the least frequent literal and EOB 9 bits
        for k, s in enumerate(rank + [256]):
            lens[s] = 8 if k < 255 else 9
    elif kind == "eob1":                               # EOB is the only 1-bit symbol; every literal 9 bits
        lens = [9] * 256 + [1]
    elif kind == "incomplete":                         # Kraft sum below 1
        lens = [9] * 256 + [2]
    else:
        raise ValueError(kind)
    return lens


def huff_png(a: np.ndarray, kind: str, ftypes=None, hdist_lens=(0,), rle=True, hclen_full=False, eob_at=None, emit_eob=True,
             trailing=b"", lens=None, pad_to=None) -> bytes:
    """one final dynamic block of literals around the filtered rows of ``a`` ([H, W, C] / [H, W]).  ``eob_at``: write the end-of-block symbol
    after that many literals (and stop); ``emit_eob`` False: none at all; ``trailing``: bytes between the block and the Adler-32"""
    a3 = a if a.ndim == 3 else a[..., None]
    h, w, c = a3.shape
    filt = filter_rows(a3, ftypes if ftypes is not None else [0] * h).tobytes()
    lens = code_lengths(kind, filt) if lens is None else lens
    codes = canonical(lens)
    bw = BitWriter()
    bw.put(0x78, 8); bw.put(0x01, 8)
    bw.put(1, 1); bw.put(2, 2)
    bw.put(0, 5); bw.put(len(hdist_lens) - 1, 5)
    seq = list(lens) + list(hdist_lens)
    # run-length symbols of the code-length alphabet
    syms, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if not rle:
            syms += [(v, 0, 0)] * run
        elif v == 0 and run >= 3:
            while run >= 3:
                r = min(run, 138)
                syms.append((18, r - 11, 7) if r >= 11 else (17, r - 3, 3))
                run -= r
            syms += [(0, 0, 0)] * run
        else:
            syms.append((v, 0, 0)); run -= 1
            while run >= 3:
                r = min(run, 6)
                syms.append((16, r - 3, 2)); run -= r
            syms += [(v, 0, 0)] * run
        i = j
    used = sorted({s for s, _, _ in syms})
    if len(used) == 1:
        used.append(0 if used[0] != 0 else 1)
    m = max(1, int(np.ceil(np.log2(len(used)))))
    short = (1 << m) - len(used)
    cl = [0] * 19
    for k, s in enumerate(used):
        cl[s] = m - 1 if k < short else m
    assert sum(1 << (7 - l) for l in cl if l) == 128
    last = max(k for k in range(19) if cl[ORDER[k]])
    hclen = 19 if hclen_full else max(4, last + 1)
    bw.put(hclen - 4, 4)
    for k in range(hclen):
        bw.put(cl[ORDER[k]], 3)
    clc = canonical(cl)
    for s, extra, nb in syms:
        bw.put_code(clc[s], cl[s])
        if nb:
            bw.put(extra, nb)
    rev = [int(format(codes[b], f"0{lens[b]}b")[::-1], 2) if lens[b] else 0 for b in range(256)]
    for b in (filt if eob_at is None else filt[:eob_at]):
        bw.put(rev[b], lens[b])
    if emit_eob:
        bw.put_code(codes[256], lens[256])
    body = bw.done() + trailing
    z = body + struct.pack(">I", zlib.adler32(filt))
    return SIG + ihdr(w, h, 8, 2 if c == 3 else 0) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def writer_cases():
    """[(name, file)]: the independent writer's files; every one must also be read by Pillow"""
    p = photo(23, 31, 5)
    g = photo(19, 40, 6, 1)
    n = np.random.default_rng(1).integers(0, 256, (16, 21, 3), dtype=np.uint8)
    out = []
    for kind in ("skew15", "flat89", "eob1"):
        for name, a in (("photo", p), ("grey", g), ("noise", n)):
            out.append((f"{kind}-{name}-rle-hdist0", huff_png(a, kind, hdist_lens=(0,), rle=True, hclen_full=False)))
            out.append((f"{kind}-{name}-rle-hdist1-hclen19", huff_png(a, kind, hdist_lens=(1,), rle=True, hclen_full=True)))
            out.append((f"{kind}-{name}-plain-hclen19", huff_png(a, kind, hdist_lens=(0,), rle=False, hclen_full=True)))
        out.append((f"{kind}-paeth", huff_png(p, kind, ftypes=[4] * p.shape[0], hdist_lens=(1,))))
    return out


def container_cases(lib):
    """[(name, file, expected status or None = ask Pillow)]: the same stream in other containers"""
    base = huff_png(photo(23, 31, 5), "skew15")
    enc = host_encode(lib, photo(37, 53, 2))
    text = (b"tEXt", b"Comment\x00hello"); phys = (b"pHYs", struct.pack(">IIB", 2835, 2835, 1)); gama = (b"gAMA", struct.pack(">I", 45455))
    return [
        ("one-byte-idats", rebuild(base, [1]), 0),
        ("split-inside-block-header", rebuild(enc, [2 + 1, 7, 50, 1, 0, 0, 100000]), 0),
        ("split-inside-zlib-header", rebuild(enc, [1, 1, 100000]), 0),
        ("empty-idats", rebuild(base, [0, 40, 0, 0, 13]), 0),
        ("ancillary-before", rebuild(enc, None, before=[text, phys, gama]), 0),
        ("ancillary-before-split", rebuild(enc, [300], before=[gama, text]), 0),
        ("ancillary-between-idats", rebuild(enc, [300], before=[phys], between=[text]), 12),    # IDATs must be consecutive: Pillow decides
    ]


# ---- declined files, one per status ------------------------------------------------------------------------------------
def _save(im, **kw) -> bytes:
    bio = io.BytesIO()
    im.save(bio, "PNG", **kw)
    return bio.getvalue()


def _png_from_z(w, h, z, ctype=2, depth=8, interlace=0, extra=()):
    return SIG + ihdr(w, h, depth, ctype, interlace) + b"".join(chunk(t, d) for t, d in extra) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def declined_cases(lib):
    """[(name, file, status)]"""
    tile = np.tile(photo(8, 8, 1), (8, 8, 1))          # repeats: zlib finds matches for certain
    raw = filter_rows(photo(20, 24, 4), [0] * 20).tobytes()
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    fixed = co.compress(raw) + co.flush()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    two = co.compress(raw[: len(raw) // 2]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[len(raw) // 2:]) + co.flush()
    jpg = io.BytesIO()
    Image.fromarray(photo(32, 32, 9)).save(jpg, "JPEG")
    ok = host_encode(lib, photo(20, 24, 4))
    exif = rebuild(ok, None, before=[(b"eXIf", b"MM\x00\x2a\x00\x00\x00\x08\x00\x00")])
    return [
        ("pillow-level-6", _save(Image.fromarray(tile), compress_level=6), 8),
        ("stored", _save(Image.fromarray(photo(20, 24, 4)), compress_level=0), 7),
        ("fixed-block", _png_from_z(24, 20, fixed), 7),
        ("two-blocks-huffman-only", _png_from_z(24, 20, two), 7),
        ("16-bit", _save(Image.fromarray((photo(9, 11, 1, 1).astype(np.uint16) * 257))), 4),
        ("palette", _save(Image.fromarray(photo(20, 24, 4)).convert("P")), 5),
        ("rgba", _save(Image.fromarray(photo(20, 24, 4)).convert("RGBA")), 5),
        ("interlaced", _png_from_z(1, 1, zlib.compress(b"\x00\x0a\x14\x1e"), interlace=1), 6),
        ("exif", exif, 10),
        ("xmp-orientation", rebuild(ok, None, before=[(b"iTXt", b"XML:com.adobe.xmp\x00\x00\x00\x00\x00<x:xmpmeta xmlns:x='adobe:ns:meta/'><rdf:RDF "
                                                       b"xmlns:rdf='http://www.w3.org/1999/02/22-rdf-syntax-ns#'><rdf:Description tiff:Orientation='6' "
                                                       b"xmlns:tiff='http://ns.adobe.com/tiff/1.0/'/></rdf:RDF></x:xmpmeta>")]), 10),
        ("too-large", SIG + ihdr(8192, 8192) + chunk(b"IDAT", b"\x78\x01\x03\x00\x00\x00\x00\x01") + chunk(b"IEND", b""), 11),
        ("unknown-critical-chunk", rebuild(ok, None, before=[(b"ABCD", b"")]), 12),
        ("jpeg", jpg.getvalue(), 1),
        ("garbage", b"this is not an image file at all", 1),
    ]


# ---- damaged files of the eligible class -------------------------------------------------------------------------------
def damaged_cases(lib):
    """[(name, file, set of allowed (status, reason), or None = any non-zero status)]: deterministic"""
    a = photo(23, 31, 5)
    good = huff_png(a, "skew15")
    z = zstream_of(good)
    flipped = bytearray(z); flipped[len(z) // 2] ^= 0x10
    bad5 = [0] * 23; bad5[7] = 5
    return [
        ("file-cut", good[:-30], {(2, 0)}),
        ("stream-cut", rebuild(good, None, z=z[: len(z) * 2 // 3]), {(15, 1), (15, 2)}),
        ("bit-flip", rebuild(good, None, z=bytes(flipped)), None),                            # any non-zero status: Adler-32, or a fallback
        ("idat-crc", rebuild(good, None, bad_idat_crc=True), {(3, 0)}),
        ("incomplete-table", huff_png(a, "incomplete"), {(9, 0)}),
        ("early-eob", huff_png(a, "skew15", eob_at=700), {(15, 3)}),
        ("missing-eob", huff_png(a, "flat89", emit_eob=False), {(15, 2)}),
        ("trailing-bytes", huff_png(a, "skew15", trailing=b"\x00\x00\x00"), {(15, 4)}),
        ("filter-byte-5", huff_png(a, "skew15", ftypes=bad5), {(14, 0)}),
    ]


# ---- subsequence / span edges --------------------------------------------------------------------------------------------
def data_bytes(lib, data: bytes, S: int) -> int:
    """compressed bytes of DEFLATE data, counted from the first data bit as the decoder counts its subsequences"""
    info, stats = np.zeros(16, np.int32), np.zeros(4, np.int32)
    buf = np.zeros(1 << 20, np.uint8)
    lib.png_dec_host_decode(data, len(data), S, 256, 1 << 20, 1, buf.ctypes.data, buf.size, info.ctypes.data, stats.ctypes.data)
    assert info[0] == 0
    return (int(info[6]) - int(info[5]) + 7) // 8


def file_with_data_bytes(lib, target: int, S: int, code: str = "flat89", seed: int = 0) -> bytes:
    """a grey file whose DEFLATE data is exactly ``target`` bytes long.  With the flat code every literal used is 8 bits long, so the
    length follows the pixel count; the few candidates around it are built and measured until one hits."""
    rng = np.random.default_rng(target + seed)
    for nf in range(max(2, target - 4), target + 2):
        w = next((w for w in range(7, 400) if nf % (1 + w) == 0), nf - 1)       # a divisor if there is one near, else one long row
        f = huff_png(rng.integers(0, 200, (nf // (1 + w), w), dtype=np.uint8), code)
        if data_bytes(lib, f, S) == target:
            return f
    raise AssertionError(f"no file with {target} data bytes found")


@functools.lru_cache(maxsize=2)
def no_sync_file(S: int, span: int, cap: int) -> bytes:
    """255 literals of 8 bits (0..254), literal 255 and end-of-block 9 bits; cap + 2 spans of data.  The subsequences are counted from
    the first data bit, so pure 8-bit data would make every guess right by accident: the FIRST pixel is the 9-bit literal, which puts
    every later symbol one bit off the guesses, and nothing after it uses a long code: a decoder one bit off stays one bit off."""
    n = (cap + 2) * span * S
    a = np.random.default_rng(5).integers(0, 200, (n // 256 + 1, 255), dtype=np.uint8)
    a[0, 0] = 255
    return huff_png(a, "flat89", lens=[8] * 255 + [9, 9])


@functools.lru_cache(maxsize=2)
def straddle_file(S: int, span: int):
    """(file, bit positions) — one grey row under a code whose value 0 (and so the filter byte) costs 1 bit and value 250 costs 15: a
    15-bit symbol starts 7 bits before the first subsequence boundary and another 7 bits before the first span boundary, both counted
    from the first data bit as the decoder counts"""
    lens = sorted(fill_complete([1, 2, 3, 4, 5, 6, 7], 257))
    assert lens[0] == 1 and lens[250] == 15
    b1, b2 = 8 * S, 8 * S * span
    p1 = b1 - 7 - 1                                    # pixels before it: the filter byte took bit 0
    p2 = p1 + 1 + (b2 - 7 - (b1 - 7 + 15))
    row = np.zeros((1, p2 + 40), np.uint8)
    row[0, p1] = row[0, p2] = 250
    return huff_png(row, "skew15", lens=lens), (b1 - 7, b2 - 7)


@functools.lru_cache(maxsize=1)
def spurious_eob_file(lib) -> bytes:
    """the encoder's file of a 1024 x 1024 photographic picture (60 spans) in which a decode from a wrong guess meets the end-of-block code
    in the middle of the stream.  While terminal states were handed on to the successors, that wiped the settled spans behind it one
    launch ahead of the repair, and this file ended at the round cap; with the rule of png_dec_core.h it settles in two rounds."""
    rng = np.random.default_rng(202)
    yy, xx = np.mgrid[0:1024, 0:1024]
    base = np.stack([128 + 80 * np.sin(xx / 37.0 + k) * np.cos(yy / 23.0 - k) for k in range(3)], axis=-1)
    return host_encode(lib, np.clip(base + rng.normal(0, 6, (1024, 1024, 3)), 0, 255).astype(np.uint8))
