"""csrc/png_dec_core.h compiled for the HOST (tests/helpers/png_dec_host.cpp: the rounds run serially): the case lists of
tests/test_gpu_png_decode.py (tests/helpers/png_dec_cases.py) against Pillow, the files of an independent writer, and a stand-alone
damage run under the address and undefined-behaviour sanitizers (tests/helpers/png_dec_fuzz_main.cpp; nothing of it is loaded into
python)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import png_dec_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cases.build_host(tmp_path_factory.mktemp("png_dec_host"))


def _same_as_pillow(host, data, mode="RGB", **kw):
    st, reason, rounds, nsub, px = cases.host_decode(host, data, mode, **kw)
    want, err = cases.pillow(data, mode)
    assert err is None, err
    assert st == 0, (st, reason)
    assert px.shape == want.shape and np.array_equal(px, want)
    return rounds, nsub


def test_geometry_is_the_documented_one(host):
    S, span, cap, band = cases.host_geometry(host)
    assert (S, span, cap, band) == (128, 256, 8, 64)


def test_round_trip_of_the_encoder(host):
    S, span, cap, band = cases.host_geometry(host)
    for name, kind, data in cases.round_trip_cases(host):
        st, reason, rounds, nsub, px = cases.host_decode(host, data)
        want, err = cases.pillow(data)
        assert err is None
        assert st == 0, (name, st, reason)                 # every round-trip file takes the device route (none has more spans than the cap)
        assert np.array_equal(px, want), name
        assert rounds <= cap
        if st == 0 and name.count(",") == 1:              # a grey shape (H, W): also as "L"
            _same_as_pillow(host, data, "L")


def test_small_subsequences_give_the_same_pixels(host):
    """the rounds' result does not depend on S or the span: 16-byte subsequences in spans of 4 ... one subsequence for the whole file"""
    data = cases.host_encode(host, cases.photo(65, 130, 2))
    for S, span in ((16, 4), (16, 1), (40, 7), (128, 256), (1 << 20, 256)):
        rounds, nsub = _same_as_pillow(host, data, S=S, span=span, cap=1 << 20)
        assert nsub >= 1 and rounds <= (nsub + span - 1) // span + 1


def test_forced_filters(host):
    band = cases.host_geometry(host)[3]
    n = 0
    for name, data in cases.forced_filter_cases(host, band):
        _same_as_pillow(host, data)
        n += 1
    assert n == 2 * 6 * 5 * 6


def test_independent_writer(host):
    for name, data in cases.writer_cases():
        want, err = cases.pillow(data)
        assert err is None, (name, err)                  # Pillow reads the writer's file: that checks the writer
        _same_as_pillow(host, data)


def test_containers(host):
    for name, data, status in cases.container_cases(host):
        st, reason, _, _, px = cases.host_decode(host, data)
        assert st == status, (name, st, reason)
        if st == 0:
            want, err = cases.pillow(data)
            assert err is None and np.array_equal(px, want), name


def test_declined_files_one_per_status(host):
    seen = set()
    for name, data, status in cases.declined_cases(host):
        st, reason, _, _, px = cases.host_decode(host, data)
        assert (st, px) == (status, None), (name, st, reason)
        seen.add(st)
    assert seen >= {1, 4, 5, 6, 7, 8, 10, 11, 12}


def test_damaged_files(host):
    for name, data, allowed in cases.damaged_cases(host):
        st, reason, _, _, px = cases.host_decode(host, data)
        assert st != 0 and px is None, name
        if allowed is not None:
            assert (st, reason) in allowed, (name, st, reason)


def test_too_large_and_hlit_statuses(host):
    import struct
    big = cases.SIG + cases.ihdr(8192, 8192) + cases.chunk(b"IDAT", b"\x78\x01\x03\x00\x00\x00\x00\x01") + cases.chunk(b"IEND", b"")
    assert cases.host_decode(host, big)[0] == 11
    assert cases.host_decode(host, cases.SIG)[0] == 2 and cases.host_decode(host, cases.SIG[:5])[0] == 2 and cases.host_decode(host, b"")[0] == 1
    crit = cases.SIG + cases.ihdr(1, 1) + cases.chunk(b"ABCD", b"") + cases.chunk(b"IEND", b"")
    assert cases.host_decode(host, crit)[0] == 12
    bad_zlib = cases.SIG + cases.ihdr(1, 1) + cases.chunk(b"IDAT", struct.pack(">H", 0x7802) + b"\x00" * 8) + cases.chunk(b"IEND", b"")
    assert cases.host_decode(host, bad_zlib)[0] == 12


def test_subsequence_and_span_edges(host):
    S, span, cap, band = cases.host_geometry(host)
    for target in (S - 1, S, S + 1, span * S - 1, span * S, span * S + 1):
        data = cases.file_with_data_bytes(host, target, S)
        assert cases.data_bytes(host, data, S) == target             # the length was hit
        st, reason, rounds, nsub, px = cases.host_decode(host, data)
        assert nsub == (target + S - 1) // S
        want, _ = cases.pillow(data)
        assert st == 0 and np.array_equal(px, want)                  # at most two spans: settled within the cap whatever the code
        assert 1 <= rounds <= cap


def test_photographic_files_stay_below_the_cap_and_long_codes_straddle_boundaries(host):
    S, span, cap, band = cases.host_geometry(host)
    a = cases.photo(300, 400, 8)                                      # > 3 spans of encoder output
    data = cases.host_encode(host, a)
    rounds, nsub = _same_as_pillow(host, data)
    assert nsub >= 3 * span and rounds <= cap
    # the skewed code's 14/15-bit symbols are frequent in noise: one starts in the last bits of many subsequences and of every span
    n = np.random.default_rng(3).integers(0, 256, (150, 200, 3), dtype=np.uint8)
    n[:, :, 0] = 7                                                    # one very frequent value keeps the code self-synchronising
    data = cases.huff_png(n, "skew15")
    rounds, nsub = _same_as_pillow(host, data)
    assert nsub > span and rounds <= cap
    # ... and placed by hand: a 15-bit symbol that starts 7 bits before the first subsequence boundary, one 7 bits before the first span boundary
    data, (b1, b2) = cases.straddle_file(S, span)
    assert b1 < 8 * S < b1 + 15 and b2 < 8 * S * span < b2 + 15
    rounds, nsub = _same_as_pillow(host, data)
    assert nsub > span


def test_a_spurious_end_of_block_in_a_speculative_decode_does_not_cost_rounds(host):
    S, span, cap, band = cases.host_geometry(host)
    rounds, nsub = _same_as_pillow(host, cases.spurious_eob_file(host))
    assert nsub > 50 * span and rounds <= 3


def test_no_self_synchronisation_ends_at_the_round_cap(host):
    """255 literals of 8 bits, data that after its first symbol never uses the two 9-bit codes: a decoder one bit off stays one bit off, so
    each cross-span round settles exactly one more span and a file of more spans than the cap cannot reach the fixed point"""
    S, span, cap, band = cases.host_geometry(host)
    data = cases.no_sync_file(S, span, cap)
    st, reason, rounds, nsub, px = cases.host_decode(host, data)
    assert nsub > (cap + 1) * span and (st, reason, rounds) == (15, 6, cap) and px is None
    # with enough rounds the same file decodes: the cap is the only obstacle
    rounds, nsub = _same_as_pillow(host, data, cap=1 << 20)
    assert rounds == (nsub + span - 1) // span


def test_damage_run_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "png_dec_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "png_dec_fuzz_main.cpp")], check=True)
    alt = tmp_path / "alt"
    alt.mkdir()
    r = subprocess.run([exe, str(alt)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "png_dec_fuzz:" in r.stdout
    # damaged streams that kept their Adler-32 are valid other files: the pixels the program got must be Pillow's
    for f in sorted(glob.glob(str(alt / "*.png"))):
        want, err = cases.pillow(open(f, "rb").read(), "RGB")
        assert err is None, (f, err)
        got = np.fromfile(f[:-4] + ".raw", dtype=np.uint8)
        want = want if got.size == want.size else want[..., 0]
        assert np.array_equal(got, want.reshape(-1)), f
