"""The host restatement of the MXFP8 quantiser (domain_rag_amd.mx, plain torch on the CPU): hand-checked blocks.  The HIP quantiser is held
to these functions byte for byte in tests/test_gpu_mxfp8.py; here the functions themselves are held to values worked out by hand."""
import torch

from domain_rag_amd import mx


def _block(values, fill=0.0):
    """one row of one 32-block: `values` first, the rest `fill`"""
    x = torch.full((1, 32), fill, dtype=torch.float32)
    x[0, : len(values)] = torch.tensor(values, dtype=torch.float32)
    xb = x.bfloat16()
    assert torch.equal(xb.float(), x), "the hand-picked inputs must be bf16 values"
    return xb


def _roundtrip(values, fill=0.0):
    q, s = mx.quantize_ref(_block(values, fill))
    return q, s, mx.dequantize_ref(q, s)[0, : len(values)].tolist()


def test_amax_mantissa_exactly_1_75_and_just_above():
    # 14 = 1.75 * 2^3: E = 3, m = 1.75 -> e = E - 8 = -5; 14 * 2^5 = 448 = e4m3fn's largest value (byte 0x7e), exact
    q, s, d = _roundtrip([14.0, -14.0, 1.0])
    assert s.tolist() == [[127 - 5]] and q[0, :3].tolist() == [0x7E, 0xFE, 0x60] and d == [14.0, -14.0, 1.0]       # 1 * 32 = 2^5: byte (5 + 7) << 3
    # the next bf16 (ulp 2^-4 at 2^3): m > 1.75 -> e = E - 7 = -4; 14.0625 * 16 = 225 -> the grid of [128, 256) has step 16: 224
    q, s, d = _roundtrip([14.0625, 1.0])
    assert s.tolist() == [[127 - 4]] and q[0, :2].tolist() == [0x76, 0x58] and d == [14.0, 1.0]                    # 224 = 1.75 * 2^7; 16 = 2^4
    # with E - 8 the second block would have had to clamp: 14.0625 * 32 = 450 > 448


def test_all_zero_block_and_signed_zero():
    q, s = mx.quantize_ref(torch.zeros(2, 64, dtype=torch.bfloat16))
    assert s.tolist() == [[127, 127]] * 2 and int(q.max()) == 0
    q, s, d = _roundtrip([-0.0, 0.0])
    assert s.tolist() == [[127]] and q[0, :2].tolist() == [0x80, 0x00] and d == [0.0, 0.0]


def test_values_on_e4m3_ties_round_to_even():
    # amax = 256: E = 8, m = 1 -> e = 0: the elements are rounded as they are
    # [16, 32) has step 2: 17 lies between 16 (mantissa 000) and 18 (001) -> 16; 19 between 18 (001) and 20 (010) -> 20
    # [2, 4) has step 0.25: 2.125 -> 2.0 (000 | 001), 2.375 -> 2.5 (001 | 010); negative values mirror
    q, s, d = _roundtrip([256.0, 17.0, 19.0, 2.125, 2.375, -17.0, -19.0, 21.0, 23.0])
    assert s.tolist() == [[127]]
    assert d == [256.0, 16.0, 20.0, 2.0, 2.5, -16.0, -20.0, 20.0, 24.0]


def test_e4m3_subnormals():
    # e = 0 again; below 2^-6 the grid is the multiples of 2^-9
    p = lambda k: 2.0 ** k
    q, s, d = _roundtrip([256.0, p(-9), p(-10), 3 * p(-10), 5 * p(-9), 7 * p(-10), p(-11), p(-6) - p(-10), -3 * p(-10)])
    assert s.tolist() == [[127]]
    # 2^-10: tie between 0 and 1 * 2^-9 -> 0 (even); 3 * 2^-10: tie between 1 and 2 -> 2; 7 * 2^-10: tie between 3 and 4 -> 4;
    # 2^-6 - 2^-10 = 7.5 * 2^-9: tie between 7 and 8 -> 8 = 2^-6, the smallest normal
    assert d == [256.0, p(-9), 0.0, 2 * p(-9), 5 * p(-9), 4 * p(-9), 0.0, p(-6), -2 * p(-9)]
    assert q[0, 1:9].tolist() == [0x01, 0x00, 0x02, 0x05, 0x04, 0x00, 0x08, 0x82]


def test_clamped_exponents():
    # amax = 2^-125: E - 8 = -133 -> clamped to -127 (byte 0); elements x * 2^127: 4, 2, 1.5 — exact; dequantised with 2^-127
    p = lambda k: 2.0 ** k
    q, s, d = _roundtrip([p(-125), p(-126), 1.5 * p(-127)])
    assert s.tolist() == [[0]] and q[0, :3].tolist() == [0x48, 0x40, 0x3C] and d == [p(-125), p(-126), 1.5 * p(-127)]
    # a bf16 subnormal amax (2^-130): still byte 0; 2^-130 * 2^127 = 2^-3 and 2^-133 * 2^127 = 2^-6, both on the grid
    q, s, d = _roundtrip([p(-130), p(-133)])
    assert s.tolist() == [[0]] and q[0, :2].tolist() == [0x20, 0x08] and d == [p(-130), p(-133)]
    # bf16's largest value 255 * 2^120: E = 127, m > 1.75 -> e = 120 (byte 247): the upper clamp cannot be reached from bf16.
    # 255 lies between 240 and 256 on the grid of [128, 256): 256 = byte 0x78 (whose value, 2^128, no float32 holds: bytes only)
    big = torch.finfo(torch.bfloat16).max
    q, s = mx.quantize_ref(_block([big, -big, big / 2]))
    assert s.tolist() == [[247]] and q[0, :3].tolist() == [0x78, 0xF8, 0x70]


def test_no_element_is_clamped_under_an_unclamped_exponent_and_e_is_minimal():
    g = torch.Generator().manual_seed(0)
    # magnitudes across bf16's whole exponent range, mantissas dense around 1.75
    x = (torch.randn(512, 256, generator=g) * torch.exp2(torch.randint(-120, 120, (512, 256), generator=g).float())).bfloat16()
    x[:, ::7] = (x[:, ::7].float() * 0 + 1.75 * torch.exp2(torch.randint(-100, 100, (512, 37), generator=g).float())).bfloat16()
    e = mx.block_exponents(x).double()
    amax = x.double().abs().view(512, -1, 32).amax(dim=2)
    unclamped = e > -127
    assert bool(unclamped.all()) and bool((e < 127).all())
    assert bool((amax * torch.exp2(-e) <= 448).all()), "an element would have to be clamped"
    assert bool((amax * torch.exp2(-(e - 1)) > 448).all()), "e is not the smallest exponent that fits"
    q, s = mx.quantize_ref(x)
    d = mx.dequantize_ref(q, s)
    assert bool(torch.isfinite(d).all())
    # e4m3's half-ulp: 2^-4 of a normal value, and never more than half a subnormal step (2^-10) of the block's scale
    err = (d.double() - x.double()).abs()
    bound = torch.maximum(x.double().abs() * 2.0 ** -4, torch.exp2(e - 10).repeat_interleave(32, dim=1))
    assert bool((err <= bound).all())
