"""GPU PNG decoder (csrc/png_dec.hip) through the C ABI and through png.decode_files: the case lists of tests/helpers/png_dec_cases.py
(the ones tests/test_png_dec_core_host.py runs through the g++ build).  Pillow is the yardstick: np.asarray(Image.open(f).convert(mode))
must be exactly equal.  ``_raw`` calls the ABI with an output buffer filled with a sentinel and guarded on both sides: a file that
is declined, falls back or is damaged must leave every byte of it untouched."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import png_dec_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 4096, 0xA5


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cases.build_host(tmp_path_factory.mktemp("png_dec_host"))


def _aligned(t):
    pad = (-t.data_ptr()) % 256
    return t.data_ptr() + pad, t.numel() - pad


def _raw(gpu, files, mode="RGB"):
    """the ABI by hand -> (stats int32 [n, 4], images: list of arrays / None); asserts the guards and the regions of undelivered files"""
    from domain_rag_amd import _lib, jpeg
    from domain_rag_amd.ops import _p, _stream, check
    lib = _lib.load()
    n = len(files)
    data, offsets = jpeg._upload(files, gpu)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    total = int(offsets[-1])
    d_off = torch.from_numpy(offsets).to(gpu)
    d_info = torch.full((n, 16), -1, dtype=torch.int32, device=gpu)
    nb = ctypes.c_int64(0)
    check(lib.drag_png_parse_workspace(n, total, ctypes.byref(nb)), "parse_workspace")
    pws_t = torch.empty(nb.value + 256, dtype=torch.uint8, device=gpu)
    pws, pws_len = _aligned(pws_t)
    check(lib.drag_png_parse(_p(data), _p(d_off), n, total, pws, pws_len, _p(d_info), _stream()), "parse")
    info = d_info.cpu().numpy()
    want_rgb = 1 if mode == "RGB" else 0
    plan, totals = np.zeros((n, 4), np.int64), np.zeros(5, np.int64)
    check(lib.drag_png_decode_plan(info.ctypes.data, n, want_rgb, plan.ctypes.data, totals.ctypes.data, ctypes.byref(nb)), "plan")
    ws_t = torch.empty(nb.value + 256, dtype=torch.uint8, device=gpu)
    ws, ws_len = _aligned(ws_t)
    out_t = torch.full((int(totals[2]) + 2 * GUARD,), FILL, dtype=torch.uint8, device=gpu)
    d_plan = torch.from_numpy(plan).to(gpu)
    d_stats = torch.full((n, 4), -1, dtype=torch.int32, device=gpu)
    check(lib.drag_png_decode(pws, _p(d_off), n, total, _p(d_info), _p(d_plan), totals.ctypes.data, want_rgb, ws, ws_len,
                              out_t.data_ptr() + GUARD, int(totals[2]), _p(d_stats), _stream()), "decode")
    torch.cuda.synchronize()
    st = d_stats.cpu().numpy()
    out = out_t.cpu().numpy()
    assert (out[:GUARD] == FILL).all() and (out[GUARD + int(totals[2]):] == FILL).all(), "guards damaged"
    body = out[GUARD: GUARD + int(totals[2])]
    images, covered = [], np.zeros(body.size, bool)
    for i in range(n):
        o, nbytes = int(plan[i, 2]), int(plan[i, 3])
        if st[i, 0] != 0:
            images.append(None)                    # its region (if it had one) stays in `not covered`: must still be the sentinel
            continue
        h, w, c = int(info[i, 2]), int(info[i, 1]), int(info[i, 3])
        images.append(body[o: o + nbytes].reshape((h, w, 3) if (c == 3 or want_rgb) else (h, w)).copy())
        covered[o: o + nbytes] = True
    assert (body[~covered] == FILL).all(), "bytes written outside the delivered images (an undelivered file wrote, or padding was touched)"
    return st, images


def _check_against_pillow(st, images, files, names, mode="RGB"):
    for i, (f, name) in enumerate(zip(files, names)):
        want, err = cases.pillow(f, mode)
        assert err is None, (name, err)
        assert st[i, 0] == 0, (name, st[i].tolist())
        assert images[i].shape == want.shape and np.array_equal(images[i], want), name


def test_geometry(gpu, host):
    from domain_rag_amd import png
    assert png.decode_geometry() == cases.host_geometry(host) == (128, 256, 8, 64)


def test_round_trip_of_the_encoder_one_call_mixed_sizes_and_colour_types(gpu, host):
    from domain_rag_amd import png
    S, span, cap, band = png.decode_geometry()
    cs = cases.round_trip_cases(host)
    files, names = [c[2] for c in cs], [c[0] for c in cs]
    st, images = _raw(gpu, files)
    _check_against_pillow(st, images, files, names)               # every file on the device: none of them has more spans than the cap
    assert (st[:, 2] <= cap).all() and (st[:, 2] >= 1).all()
    # the files the GPU encoder writes itself, through the public call
    arrs = [cases.content(k, (65, 130, 3)) for k in cases.KINDS]
    own = png.encode(torch.from_numpy(np.stack(arrs)).to(gpu))
    grey = png.encode(torch.from_numpy(cases.content("photo", (128, 96))).to(gpu)[None])
    batch = png.decode_files(own + grey + files[:8], gpu)
    assert batch.route == ["device"] * len(batch) and all(e is None for e in batch.errors) and (batch.status == 0).all()
    for a, img in zip(arrs, batch.images):
        assert img.device.type == "cuda" and img.dtype == torch.uint8 and np.array_equal(img.cpu().numpy(), a)
    assert np.array_equal(batch.images[4].cpu().numpy()[..., 1], cases.content("photo", (128, 96)))
    for f, img in zip(files[:8], batch.images[5:]):
        assert np.array_equal(img.cpu().numpy(), cases.pillow(f)[0])
    assert all(s["rounds"] >= 1 and s["subsequences"] >= 1 and s["fallback"] == 0 for s in batch.stats)
    # mode "L": grey files on the device as [H, W]; an RGB file goes to Pillow (its luma transform is not a device path)
    bl = png.decode_files(grey + own[:1], gpu, mode="L")
    assert bl.route == ["device", "pil"] and bl.status.tolist() == [0, png.STATUS_MODE]
    assert np.array_equal(bl.images[0].cpu().numpy(), cases.pillow(grey[0], "L")[0]) and np.array_equal(bl.images[1].cpu().numpy(), cases.pillow(own[0], "L")[0])


def test_forced_filters(gpu, host):
    from domain_rag_amd import png
    band = png.decode_geometry()[3]
    cs = cases.forced_filter_cases(host, band)
    assert len(cs) == 2 * 6 * 5 * 6
    files, names = [c[1] for c in cs], [c[0] for c in cs]
    st, images = _raw(gpu, files)
    _check_against_pillow(st, images, files, names)
    grey = [f for f, nm in zip(files, names) if nm.endswith("x1")][:40]
    st, images = _raw(gpu, grey, "L")
    _check_against_pillow(st, images, grey, ["L"] * len(grey), "L")


def test_headers_and_containers(gpu, host):
    from domain_rag_amd import png
    w = cases.writer_cases()
    files, names = [c[1] for c in w], [c[0] for c in w]
    st, images = _raw(gpu, files)
    _check_against_pillow(st, images, files, names)
    cc = cases.container_cases(host)
    files = [c[1] for c in cc]
    st, images = _raw(gpu, files)
    assert st[:, 0].tolist() == [c[2] for c in cc]
    batch = png.decode_files(files, gpu)
    for i, (name, f, status) in enumerate(cc):
        want, err = cases.pillow(f)
        assert batch.route[i] == ("device" if status == 0 else "pil")
        if err is None:
            assert np.array_equal(batch.images[i].cpu().numpy(), want), name
            if status == 0:
                assert np.array_equal(images[i], want), name
        else:
            assert batch.images[i] is None and batch.errors[i], name


def test_subsequence_and_span_edges(gpu, host):
    from domain_rag_amd import png
    S, span, cap, band = png.decode_geometry()
    files, names = [], []
    for target in (S - 1, S, S + 1, span * S - 1, span * S, span * S + 1):
        f = cases.file_with_data_bytes(host, target, S)
        assert cases.data_bytes(host, f, S) == target                 # the length was hit
        files.append(f); names.append(f"flat-{target}")
    big = cases.host_encode(host, cases.photo(300, 400, 8))           # a photographic file of more than three spans
    noise = np.random.default_rng(3).integers(0, 256, (150, 200, 3), dtype=np.uint8)
    noise[:, :, 0] = 7
    long_codes = cases.huff_png(noise, "skew15")                      # two thirds of its symbols are 14 / 15 bits long: they straddle every boundary
    straddle, _ = cases.straddle_file(S, span)                        # a 15-bit symbol across the first subsequence boundary, another across the first span boundary
    files += [straddle, big, long_codes]; names += ["straddle", "photo-3-spans", "long-codes"]
    st, images = _raw(gpu, files)
    _check_against_pillow(st, images, files, names)
    for i, f in enumerate(files):
        hs = cases.host_decode(host, f)
        assert (st[i, 2], st[i, 3]) == (hs[2], hs[3]), names[i]       # rounds and subsequences: the serial driver's
    assert st[-2, 3] >= 3 * span and st[-1, 3] > span and (st[:, 2] <= cap).all()


def test_a_spurious_end_of_block_in_a_speculative_decode_does_not_cost_rounds(gpu, host):
    from domain_rag_amd import png
    S, span, cap, band = png.decode_geometry()
    f = cases.spurious_eob_file(host)
    st, images = _raw(gpu, [f])
    _check_against_pillow(st, images, [f], ["spurious-eob"])
    assert st[0, 3] > 50 * span and st[0, 2] <= 3


def test_declined_files_one_per_status(gpu, host):
    from domain_rag_amd import png
    dc = cases.declined_cases(host)
    files = [c[1] for c in dc]
    st, images = _raw(gpu, files)
    assert st[:, 0].tolist() == [c[2] for c in dc] and all(im is None for im in images)
    batch = png.decode_files(files, gpu)
    assert batch.status.tolist() == [c[2] for c in dc] and batch.route == ["pil"] * len(dc)
    for i, (name, f, status) in enumerate(dc):
        want, err = cases.pillow(f)
        if err is None:
            assert batch.errors[i] is None and np.array_equal(batch.images[i].cpu().numpy(), want), name
        else:
            assert batch.images[i] is None and err.split(":")[0] in batch.errors[i], name
    assert batch.images[-1] is None and batch.errors[-1]              # the unreadable file
    assert sum(im is not None for im in batch.images) >= len(dc) - 2


def test_no_self_synchronisation_ends_at_the_round_cap(gpu, host):
    from domain_rag_amd import png
    S, span, cap, band = png.decode_geometry()
    f = cases.no_sync_file(S, span, cap)
    st, images = _raw(gpu, [f])
    assert st[0].tolist()[:3] == [15, png.FALLBACK_ROUND_CAP, cap] and st[0, 3] > (cap + 1) * span and images[0] is None
    batch = png.decode_files([f], gpu)
    assert batch.route == ["pil"] and batch.stats[0]["fallback"] == png.FALLBACK_ROUND_CAP and batch.stats[0]["rounds"] == cap
    assert np.array_equal(batch.images[0].cpu().numpy(), cases.pillow(f)[0])


def test_damaged_eligible_files(gpu, host):
    dm = cases.damaged_cases(host)
    files = [c[1] for c in dm] + [cases.host_encode(host, cases.photo(37, 53, 2))]     # and one good file in the same call
    st, images = _raw(gpu, files)
    for i, (name, f, allowed) in enumerate(dm):
        assert st[i, 0] != 0 and images[i] is None, name
        if allowed is not None:
            assert (int(st[i, 0]), int(st[i, 1])) in allowed, (name, st[i].tolist())
        hs = cases.host_decode(host, f)
        assert (int(st[i, 0]), int(st[i, 1])) == (hs[0], hs[1]), name    # the serial driver's verdict
    assert st[-1, 0] == 0 and np.array_equal(images[-1], cases.pillow(files[-1])[0])
    # ... and through the public call: every damaged file takes the "pil" route and comes back as whatever Pillow makes of it
    from domain_rag_amd import png
    batch = png.decode_files(files, gpu)
    assert batch.route == ["pil"] * len(dm) + ["device"] and batch.status.tolist() == st[:, 0].tolist()
    for i, (name, f, allowed) in enumerate(dm):
        want, err = cases.pillow(f)
        if err is None:
            assert batch.errors[i] is None and np.array_equal(batch.images[i].cpu().numpy(), want), name
        else:
            assert batch.images[i] is None and err.split(":")[0] in batch.errors[i], name


def test_argument_errors(gpu, host):
    from domain_rag_amd import _lib, png
    from domain_rag_amd.ops import _p
    lib = _lib.load()
    f = cases.host_encode(host, cases.photo(20, 24, 4))
    with pytest.raises(RuntimeError, match="GPU path"):
        png.decode_files([f], "cpu")
    with pytest.raises(TypeError, match="bytes"):
        png.decode_files([np.frombuffer(f, np.uint8)], gpu)
    with pytest.raises(ValueError, match="mode"):
        png.decode_files([f], gpu, mode="RGBA")
    assert len(png.decode_files([], gpu)) == 0
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    p, _ = _aligned(buf)
    off = torch.tensor([0, len(f)], dtype=torch.int64, device=gpu)
    info = torch.zeros((1, 16), dtype=torch.int32, device=gpu)
    assert lib.drag_png_parse(None, _p(off), 1, len(f), p, 1 << 19, _p(info), None) != 0 and b"null" in lib.drag_last_error()
    assert lib.drag_png_parse(p, _p(off), 1, len(f), p, 1000, _p(info), None) != 0 and b"workspace smaller" in lib.drag_last_error()
    assert lib.drag_png_parse(p, _p(off), 1, len(f), p + 1, 1 << 19, _p(info), None) != 0 and b"aligned" in lib.drag_last_error()
    assert lib.drag_png_parse(p, _p(off), 0, len(f), p, 1 << 19, _p(info), None) != 0 and b"1 <= n" in lib.drag_last_error()
    hinfo = np.zeros((1, 16), np.int32); hinfo[0, :8] = [0, 24, 20, 3, 100, 1122, 1500, 1]
    plan, totals, nb = np.zeros((1, 4), np.int64), np.zeros(5, np.int64), ctypes.c_int64(0)
    assert lib.drag_png_decode_plan(hinfo.ctypes.data, 1, 1, plan.ctypes.data, totals.ctypes.data, ctypes.byref(nb)) == 0 and nb.value > 0
    stats = torch.zeros((1, 4), dtype=torch.int32, device=gpu)
    args = (p, _p(off), 1, len(f), _p(info), _p(info), totals.ctypes.data, 1)
    assert lib.drag_png_decode(*args, p, 64, p, 1 << 19, _p(stats), None) != 0 and b"workspace smaller" in lib.drag_last_error()
    assert lib.drag_png_decode(*args, p, 1 << 19, p, 10, _p(stats), None) != 0 and b"output buffer smaller" in lib.drag_last_error()
    bad = hinfo.copy(); bad[0, 2] = 1 << 30
    assert lib.drag_png_decode_plan(bad.ctypes.data, 1, 1, plan.ctypes.data, totals.ctypes.data, ctypes.byref(nb)) != 0
    assert b"cannot have written" in lib.drag_last_error()


def test_decode_paths_reads_files_and_reports_missing_ones(gpu, host, tmp_path):
    from domain_rag_amd import png
    a = cases.photo(70, 90, 12)
    good, other = tmp_path / "a.png", tmp_path / "b.png"
    good.write_bytes(cases.host_encode(host, a))
    from PIL import Image
    tiled = np.tile(cases.photo(8, 8, 1), (8, 8, 1))                   # repeats: Pillow's zlib finds matches, so its file is LZ77: the "pil" route
    Image.fromarray(tiled).save(other)                                 # (its file of a NOISY image can be match-free with HLIT = 257: that one is eligible)
    batch = png.decode_paths([str(good), str(tmp_path / "missing.png"), str(other)], gpu)
    assert batch.route == ["device", "pil", "pil"] and batch.images[1] is None and "No such file" in batch.errors[1]
    assert batch.status.tolist() == [0, 1, 8]
    assert np.array_equal(batch.images[0].cpu().numpy(), a) and np.array_equal(batch.images[2].cpu().numpy(), tiled)
