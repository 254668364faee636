"""uint8 images on the GPU -> PNG files (``drag_png_encode``): the reference's ``image.save(path)`` of its large RGB results
(batch_generate_flux_kshot.py:480, outpainting_updown_sampling_redux.py:1262,1278) without the host's zlib.  SURVEY §8(f)-2.

A PNG is defined by the pixels it decodes to: the files differ from Pillow's bytes (one dynamic-Huffman block of literals
instead of zlib level 6 — within ~10 % of its size on photographic content) and decode to exactly the array handed in.

    files = encode(images)            # uint8 [n, H, W, 3] (or [n, H, W] / [n, H, W, 1] grey) on the device -> list of bytes
    save(images, paths)               # ... written to disk

and the way back (``drag_png_parse`` / ``drag_png_decode``): PNG files -> pixels on the GPU, exactly
``PIL.Image.open(f).convert(mode)``.  The device decodes the class of files ``encode`` writes (8-bit grey / RGB, one dynamic-Huffman
block of literals: csrc/png_dec_core.h); any other file is reported with a status and decoded by Pillow itself (same bytes by
definition), as ``retrieval.py`` does for the JPEGs its decoder declines.

    batch = decode_files([bytes, ...])     # or a jpeg.StagedFiles; mode="RGB" | "L"   -> DecodedPngBatch
    batch.images[i]                        # uint8 [H, W, 3] (mode "L": [H, W]) on the device, None if nothing could read the file
    batch.route[i], batch.status[i], batch.stats[i], batch.errors[i]
    decode_paths(paths)                    # files read by the library's reader threads (jpeg.stage_paths), then decode_files
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream, check

_scratch: dict = {}


def _buffers(device, ws_bytes: int, out_bytes: int):
    """scratch + output buffers, reused per device and grown geometrically (a stage writes thousands of same-size images)"""
    key = str(device)
    ws, out = _scratch.get(key, (None, None))
    if ws is None or ws.numel() < ws_bytes:
        ws = torch.empty(max(ws_bytes, 2 * (ws.numel() if ws is not None else 0)), dtype=torch.uint8, device=device)
    if out is None or out.numel() < out_bytes:
        out = torch.empty(max(out_bytes, 2 * (out.numel() if out is not None else 0)), dtype=torch.uint8, device=device)
    _scratch[key] = (ws, out)
    return ws, out


def encode(images: torch.Tensor) -> list:
    """``images``: uint8, on the GPU: ``[n, H, W, 3]`` / ``[H, W, 3]`` (RGB files) or ``[n, H, W, 1]`` / ``[n, H, W]`` (8-bit grey
    files).  A 3-D tensor whose last dimension is 1 or 3 is ONE image; any other 3-D tensor is a batch of grey images.
    Returns one ``bytes`` object (a whole .png file) per image."""
    lib = _lib.load()
    if images.dtype != torch.uint8:
        raise TypeError("png.encode: uint8 images expected")
    if images.device.type != "cuda":
        raise RuntimeError("png.encode: the PNG encoder is a GPU path (domain-rag_amd has no CPU fallback)")
    if images.dim() == 3 and images.shape[-1] in (1, 3):
        images = images[None]
    if images.dim() == 3:
        images = images[..., None]
    if images.dim() != 4 or images.shape[-1] not in (1, 3):
        raise ValueError(f"png.encode: [n, H, W, 3] or [n, H, W, 1] expected, got {tuple(images.shape)}")
    images = images.contiguous()
    n, H, W, C = (int(v) for v in images.shape)
    if n == 0:
        return []
    ws_bytes, stride = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.drag_png_plan(n, H, W, C, ctypes.byref(ws_bytes), ctypes.byref(stride)), "drag_png_plan")
    ws, out = _buffers(images.device, ws_bytes.value + 256, n * stride.value)
    pad = (-ws.data_ptr()) % 256
    sizes = torch.empty(n, dtype=torch.int64, device=images.device)
    check(lib.drag_png_encode(_p(images), n, H, W, C, ws.data_ptr() + pad, ws.numel() - pad, _p(out), stride.value, _p(sizes),
                              _stream()), "drag_png_encode")
    host_sizes = sizes.cpu().tolist()                      # the one synchronisation
    files = []
    for i, sz in enumerate(host_sizes):
        files.append(out[i * stride.value: i * stride.value + sz].cpu().numpy().tobytes())
    return files


def save(images: torch.Tensor, paths) -> None:
    files = encode(images)
    if len(files) != len(paths):
        raise ValueError("png.save: one path per image")
    for data, path in zip(files, paths):
        with open(path, "wb") as f:
            f.write(data)


INFO_WORDS = 16
STATUS_MODE = 16            # set by decode_files itself: mode "L" asked of an RGB file (Pillow's luma transform is not a device path)
DECODE_STATUS_TEXT = {0: "decoded on the device", 1: "not a PNG", 2: "truncated", 3: "chunk CRC", 4: "bit depth other than 8",
                      5: "colour type other than grey / RGB (palette, alpha, tRNS)", 6: "interlaced", 7: "stored / fixed / multi-block stream",
                      8: "HLIT > 257 (LZ77 matches possible)", 9: "bad code table", 10: "eXIf", 11: "too large",
                      12: "other (zlib header, unknown critical / APNG chunk, IDATs not consecutive, too many chunks)", 13: "Adler-32 mismatch",
                      14: "filter byte > 4", 15: "parallel Huffman decode fell back", STATUS_MODE: "mode L asked of an RGB file"}
FALLBACK_TEXT = {0: "", 1: "a window that is no code", 2: "a symbol needs bits past the stream (or no end-of-block)", 3: "end-of-block too early",
                 4: "data between end-of-block and the Adler-32", 5: "too many literals", 6: "round cap"}
FALLBACK_ROUND_CAP = 6


class DecodedPngBatch:
    """``images[i]``: device uint8 tensor or None; ``status[i]``: the device's verdict (DECODE_STATUS_TEXT); ``route[i]``: "device" or
    "pil"; ``stats[i]``: dict(subsequences, rounds, fallback, fallback_text); ``errors[i]``: None, or the message of the exception that
    kept Pillow (or the file reader) from delivering the file"""

    def __init__(self, images, status, route, stats, errors):
        self.images, self.status, self.route, self.stats, self.errors = images, status, route, stats, errors

    def __len__(self) -> int:
        return len(self.images)


def decode_geometry() -> tuple:
    """(bytes per subsequence S, subsequences per workgroup span, round cap, rows per un-filter band B) of the device decoder"""
    lib = _lib.load()
    g = (ctypes.c_int32 * 4)()
    check(lib.drag_png_decode_geometry(ctypes.byref(g, 0), ctypes.byref(g, 4), ctypes.byref(g, 8), ctypes.byref(g, 12)), "drag_png_decode_geometry")
    return int(g[0]), int(g[1]), int(g[2]), int(g[3])


_dec_scratch: dict = {}


def _dec_buffer(device, slot: str, nbytes: int) -> tuple:
    """(256-byte aligned address, usable bytes) of a scratch buffer reused per (device, slot), grown geometrically"""
    key = (str(device), slot)
    ws = _dec_scratch.get(key)
    if ws is None or ws.numel() < nbytes + 256:
        ws = torch.empty(max(nbytes + 256, 2 * (ws.numel() if ws is not None else 0)), dtype=torch.uint8, device=device)
        _dec_scratch[key] = ws
    pad = (-ws.data_ptr()) % 256
    return ws.data_ptr() + pad, ws.numel() - pad


def decode_files(blobs, device="cuda", mode: str = "RGB") -> DecodedPngBatch:
    """``blobs``: list of ``bytes`` (whole files) or a ``jpeg.StagedFiles``.  ``mode``: "RGB" (grey files are replicated) or "L".
    Files of the device's class are decoded by libdomainrag_hip.so (no CPU fallback for them); the others, and the ones the device
    falls back on, by ``Image.open(...).convert(mode)`` and uploaded.  Two synchronisations: the descriptors (to size the outputs) and
    the statuses (to know which files fell back)."""
    from . import jpeg
    if mode not in ("RGB", "L"):
        raise ValueError(f"png.decode_files: mode must be 'RGB' or 'L', got {mode!r}")
    lib = _lib.load()
    n = len(blobs)
    if n == 0:
        return DecodedPngBatch([], np.zeros(0, np.int32), [], [], [])
    if n > 65535:
        raise ValueError("png.decode_files: at most 65535 files per batch")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("png.decode_files: the PNG decoder is a GPU path (domain-rag_amd has no CPU fallback)")
    staged = blobs if isinstance(blobs, jpeg.StagedFiles) else None
    if staged is not None:
        offsets, data = staged.offsets, staged.device_blob(device)
    else:
        for b in blobs:
            if not isinstance(b, (bytes, bytearray, memoryview)):
                raise TypeError("png.decode_files: a list of bytes objects or a jpeg.StagedFiles expected")
        data, offsets = jpeg._upload(blobs, device)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    total = int(offsets[-1])
    want_rgb = 1 if mode == "RGB" else 0
    d_off = torch.from_numpy(offsets).to(device)
    d_info = torch.empty((n, INFO_WORDS), dtype=torch.int32, device=device)
    pws_bytes = ctypes.c_int64(0)
    check(lib.drag_png_parse_workspace(n, total, ctypes.byref(pws_bytes)), "drag_png_parse_workspace")
    pws, pws_len = _dec_buffer(device, "parse", pws_bytes.value)
    check(lib.drag_png_parse(_p(data), _p(d_off), n, total, pws, pws_len, _p(d_info), _stream()), "drag_png_parse")
    info = d_info.cpu().numpy()                        # synchronisation 1: geometry, to size the outputs
    if not want_rgb:
        rgb_files = (info[:, 0] == 0) & (info[:, 3] == 3)
        if rgb_files.any():
            info[rgb_files, 0] = STATUS_MODE
            d_info = torch.from_numpy(info).to(device)
    plan = np.zeros((n, 4), dtype=np.int64)
    totals = np.zeros(5, dtype=np.int64)
    ws_bytes = ctypes.c_int64(0)
    check(lib.drag_png_decode_plan(info.ctypes.data, n, want_rgb, plan.ctypes.data, totals.ctypes.data, ctypes.byref(ws_bytes)), "drag_png_decode_plan")
    ws, ws_len = _dec_buffer(device, "decode", ws_bytes.value)
    out = torch.empty(max(int(totals[2]), 1), dtype=torch.uint8, device=device)
    d_plan = torch.from_numpy(plan).to(device)
    d_stats = torch.empty((n, 4), dtype=torch.int32, device=device)
    check(lib.drag_png_decode(pws, _p(d_off), n, total, _p(d_info), _p(d_plan), totals.ctypes.data, want_rgb, ws, ws_len, _p(out), out.numel(),
                              _p(d_stats), _stream()), "drag_png_decode")
    st = d_stats.cpu().numpy()                         # synchronisation 2: which files the device delivered
    images, route, stats, errors = [], [], [], []
    for i in range(n):
        status, reason = int(st[i, 0]), int(st[i, 1])
        stats.append(dict(subsequences=int(st[i, 3]), rounds=int(st[i, 2]), fallback=reason, fallback_text=FALLBACK_TEXT.get(reason, "?")))
        if status == 0:
            h, w, c = int(info[i, 2]), int(info[i, 1]), int(info[i, 3])
            o = int(plan[i, 2])
            shape = (h, w, 3) if (c == 3 or want_rgb) else (h, w)
            images.append(out[o: o + int(plan[i, 3])].view(shape))
            route.append("device"); errors.append(None)
            continue
        route.append("pil")
        if staged is not None and i in staged.errors:
            images.append(None); errors.append(str(staged.errors[i]))
            continue
        try:
            import io
            from PIL import Image
            raw = staged.file_bytes(i) if staged is not None else bytes(blobs[i])
            arr = np.array(Image.open(io.BytesIO(raw)).convert(mode))          # a writable copy
            images.append(torch.from_numpy(arr).to(device)); errors.append(None)
        except Exception as e:  # noqa: BLE001  (whatever Pillow raises for a file it cannot read is the file's verdict)
            images.append(None); errors.append(f"{type(e).__name__}: {e}")
    return DecodedPngBatch(images, st[:, 0].copy(), route, stats, errors)


def decode_paths(paths, device="cuda", mode: str = "RGB", slot: int = 0, threads: int = 32) -> DecodedPngBatch:
    """``decode_files`` of files on disk, read into the pinned staging buffer by the library's reader threads (``jpeg.stage_paths``)"""
    from . import jpeg
    if len(paths) == 0:
        return DecodedPngBatch([], np.zeros(0, np.int32), [], [], [])
    return decode_files(jpeg.stage_paths(list(paths), device, slot=slot, threads=threads), device, mode)
