"""OCP MX formats as this library stores them, and a host restatement of the MXFP8 quantiser (plain torch, CPU).

Storage (``drag_quantize_mxfp8`` / ``drag_gemm_mxfp8``, include/domainrag_hip.h):

* elements: e4m3fn bytes, dense ``[rows, K]``, ``K % 128 == 0``;
* scales: e8m0 bytes, dense ``[rows, K / 32]``: one per block of 32 consecutive K elements, byte ``b`` = ``2^(b - 127)``;
* both travel as ``uint8`` tensors (torch's ``float8_e4m3fn`` / ``float8_e8m0fnu`` are views of the same bytes).

Scale rule.  ``amax`` = max |x| of the block (exact: the inputs are bf16); ``e`` = the smallest integer with
``amax * 2^-e <= 448``: with ``amax = m * 2^E``, ``1 <= m < 2``, that is ``E - 8`` for ``m <= 1.75`` and ``E - 7`` otherwise — taken from
the bits, never from ``log2`` — clamped to [-127, 127].  An all-zero block stores byte 127 and zero elements.  Elements are
``x * 2^-e`` rounded to nearest-even to e4m3fn and saturated at +-448 (reachable only when ``e`` was clamped).  (The MX document's floor
rule ``E - 8`` clamps 0.9 % of N(0, 1) elements by up to 12 %; on a row with one x30 outlier channel this rule gave 3.8 % rms GEMM error
against 4.7 %.)  Non-finite inputs are outside the contract.

``quantize_ref`` / ``dequantize_ref`` are what the tests hold the HIP quantiser and the MX GEMM against; no product path calls them.

MXFP8 attention (``drag_qkv_prep_mxfp8`` / ``drag_attention_mxfp8``; opt-in, head_dim 128).  All blocks are MX blocks under the rule above,
dense per (batch, head), ``s_pad`` = S rounded up to a multiple of 128 (one KV tile of the kernel):

* q, k: the values ``drag_qk_norm_rope_vt_bf16`` would write (RMSNorm and RoPE, rounded to bf16), quantised along head_dim: bytes
  ``[B, H, s_pad, 128]`` + scales ``[B, H, s_pad, 4]``.  Rows >= S hold zero bytes and scale byte 127.
* V^T: bytes ``[B, H, 128, s_pad]`` + scales ``[B, H, 128, s_pad / 32]``, quantised along the key axis in blocks of the 32 keys
  ``[32 j, 32 j + 32)``, keys >= S as zeros.  Keys stand in NATURAL order inside a block: the kernel computes the scores of a 128-key tile
  in the order its P registers need (csrc/attention_mxfp8.h), so the image is not permuted.
* P: ``p = exp(s - m)`` with ``m`` the running row maximum, so ``p <= 1``; the matrix operand is ``e4m3(p * 2^8)`` under the constant scale
  byte 119 (= 2^-8).  The row sum ``l`` adds the float32 ``p`` before that rounding; accumulators, rescales and ``1 / l`` are float32.
* Scores are ``(q^ . k^) * scale`` in float32: the softmax scale is not folded into the quantised q.  Keys >= S are masked to -inf; a zero
  k row inside S scores 0, not -inf.

``attention_ref`` restates that on the host for one head (with the final row maximum instead of the running one, and float64 products); the
tests hold the kernel to its distance from exact attention.  No product path calls it.
"""
from __future__ import annotations

import torch

BLOCK = 32
E4M3_MAX = 448.0


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """exact float32 2^e for integer e in [-126, 127], from the exponent bits"""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def block_exponents(x: torch.Tensor) -> torch.Tensor:
    """the shared exponent ``e`` (int32 ``[rows, K / 32]``) of every 32-block of a bf16 ``[rows, K]`` matrix, from the bits"""
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.shape[1] % BLOCK:
        raise ValueError("mx: expected a bf16 [rows, K] matrix with K % 32 == 0")
    bits = x.contiguous().view(torch.int16).to(torch.int32) & 0x7FFF
    amax = bits.view(x.shape[0], -1, BLOCK).amax(dim=2)             # bf16 magnitudes order like their bit patterns
    E = (amax >> 7) - 127                                           # (a subnormal amax reads E = -127: clamped below either way)
    e = E - 8 + ((amax & 0x7F) > 0x60).to(torch.int32)              # mantissa above 1.75 = 1.1100000b
    e = e.clamp(-127, 127)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def quantize_ref(x: torch.Tensor):
    """bf16 ``[rows, K]`` (CPU) -> (e4m3fn bytes ``[rows, K]``, e8m0 bytes ``[rows, K / 32]``), both uint8"""
    x = x.detach().cpu()
    e = block_exponents(x)
    inv = _pow2(-e).repeat_interleave(BLOCK, dim=1)                 # -e in [-127, 127]; 2^-127 never occurs (e <= 120 for bf16 inputs)
    # the clamp is required: torch's cast returns NaN from 465 up instead of saturating
    q = (x.float() * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), (e + 127).to(torch.uint8)


def dequantize_ref(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(e4m3fn bytes, e8m0 bytes) -> float32 ``[rows, K]``; exact (a product with a power of two)"""
    q, s = q.detach().cpu(), s.detach().cpu()
    e = s.to(torch.int32) - 127
    v = q.contiguous().view(torch.float8_e4m3fn).float()
    # two exact factors: 2^-127 alone is not a normal float32
    half = torch.div(e, 2, rounding_mode="floor")
    return v * _pow2(half).repeat_interleave(BLOCK, dim=1) * _pow2(e - half).repeat_interleave(BLOCK, dim=1)


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> torch.Tensor:
    """MXFP8 attention of one head on the host: prepared bf16 ``q``, ``k``, ``v`` ``[S, 128]`` (CPU) -> bf16 ``[S, 128]``.

    q and k are quantised along head_dim, V^T along the keys (zero-padded to a multiple of 32); scores ``(q^ . k^) * scale`` and both
    products in float64; ``p = exp(s - m)`` with ``m`` the final row maximum; ``P^ = e4m3(p * 256) / 256``; ``out = bf16(P^ . V^ / sum p)``
    (the sum of the unrounded ``p``)."""
    q, k, v = (t.detach().cpu() for t in (q, k, v))
    if not all(t.dtype == torch.bfloat16 and t.dim() == 2 and t.shape == q.shape and t.shape[1] == 128 for t in (q, k, v)):
        raise ValueError("mx.attention_ref: bf16 [S, 128] q, k and v of one head expected")
    S = q.shape[0]
    qh = dequantize_ref(*quantize_ref(q)).double()
    kh = dequantize_ref(*quantize_ref(k)).double()
    vt = torch.zeros((128, (S + BLOCK - 1) // BLOCK * BLOCK), dtype=torch.bfloat16)
    vt[:, :S] = v.t()
    vh = dequantize_ref(*quantize_ref(vt)).double()[:, :S]          # [128, S]
    s = (qh @ kh.t()) * float(scale)
    p = torch.exp(s - s.amax(dim=1, keepdim=True))
    ph = (p * 256.0).float().to(torch.float8_e4m3fn).double() / 256.0      # p * 256 <= 256 < 448: no saturation
    return ((ph @ vh.t()) / p.sum(dim=1, keepdim=True)).float().to(torch.bfloat16)
