"""float64 restatements of the kernels of csrc/textenc.hip with the kernels' own rounding points, and the inputs that
tests/test_gpu_textenc_kernels.py feeds the kernels.  tests/test_textenc_restatements_host.py holds all of it, without a GPU, to the upstream
modules run on CPU bf16 tensors (T5LayerNorm, NewGELUActivation, CLIP's x * sigmoid(1.702 x), an embedding lookup) and shows that the
exact-answer attention inputs give exactly the V rows they promise."""
import math

import torch

from elementwise_ref import BF16_MAX, FLT_MAX, all_bf16_patterns, round_bf16, to_bf16  # noqa: F401  (re-exported for the tests)

EW_GRID_CAP = 8192                       # ew_blocks() of csrc/textenc.hip: at most this many workgroups of 256 lanes, 8 elements per lane
N8_FIRST_TRIP = EW_GRID_CAP * 256        # 2 097 152 vectors of 8: one more and a grid-stride loop runs its body a second time
C_NEW_GELU = float(torch.tensor(0.044715, dtype=torch.float32))                  # the kernels' float32 constants, as float64
C_SQRT_2_PI = float(torch.tensor(0.7978845608028654, dtype=torch.float32))
C_QUICK = float(torch.tensor(1.702, dtype=torch.float32))


def _bf(x):
    return x.float().bfloat16()


def _f32_range(s):
    """what a float32 holds of a float64 value's range: past FLT_MAX it is inf"""
    return torch.where(s.abs() > FLT_MAX, torch.copysign(torch.full_like(s, math.inf), s), s)


def patterns_by_high_byte() -> torch.Tensor:
    """the 65 536 bf16 values as [256, 256]: row = sign and the exponent's upper seven bits, so a row spans two binades and its largest
    output says something about every element of it (rows 127 and 255 hold the infs and the NaNs)"""
    return all_bf16_patterns().view(256, 256)


# ------------------------------------------------------------------ attention
def attention_f64(qkv, B, S, H, rel, causal, eager, scale):
    """the kernel's function with its rounding points, in float64 on the host; qkv [B, S, 3 * H * 64] = [q | k | v], rel [H, 2S-1] or None"""
    D = H * 64
    x = qkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)             # [3, B, H, S, 64]
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2)
    qi, ki = torch.arange(S)[:, None], torch.arange(S)[None, :]
    bias = rel.double()[:, ki - qi + S - 1][None] if rel is not None else 0.0       # [1, H, S, S]
    if eager:
        s = _bf(s).double()
        if scale != 1.0:
            s = _bf(s * scale).double()
        if rel is not None:
            s = _bf(s + bias).double()
    else:
        s = s * scale + bias
    if causal:
        s = s.masked_fill(ki > qi, float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    if eager:
        o = _bf(e / e.sum(-1, keepdim=True)).double() @ v
    else:
        o = (_bf(e).double() @ v) / e.sum(-1, keepdim=True)
    return _bf(o).permute(0, 2, 1, 3).reshape(B, S, D)


def row_index(B, S, D, ld, batch_stride):
    """[B, S, D] element offsets of D-wide rows of stride ld, S per batch, batches batch_stride apart"""
    return (torch.arange(B)[:, None, None] * batch_stride + torch.arange(S)[None, :, None] * ld + torch.arange(D)[None, None, :])


def attention_strided(buf, q_off, k_off, v_off, B, S, H, ld, batch_stride, rel, causal, eager, scale, out, ld_o, o_batch_stride):
    """attention_f64 on q / k / v rows picked out of the flat storage ``buf`` (row s of batch b at offset + b * batch_stride + s * ld) and
    written into a copy of the flat destination ``out`` at b * o_batch_stride + s * ld_o: (the destination as it must look, the [B, S, D] rows)"""
    D = H * 64
    idx = row_index(B, S, D, ld, batch_stride)
    qkv = torch.cat([buf[q_off + idx], buf[k_off + idx], buf[v_off + idx]], dim=-1)
    rows = attention_f64(qkv, B, S, H, rel, causal, eager, scale)
    full = out.clone()
    full[row_index(B, S, D, ld_o, o_batch_stride).reshape(-1)] = rows.reshape(-1)
    return full, rows


def onehot_alpha(scale: float) -> float:
    """the key code's amplitude: the best logit beats the runner-up by 2 alpha scale = 128, past 104 where expf gives 0 in float32"""
    alpha = 64.0 / scale
    assert math.frexp(alpha)[0] == 0.5 and 2 * alpha * scale >= 128          # a power of two: every q.k is an integer multiple of 2 alpha
    return alpha


def onehot_perms(S, causal, seed):
    """the maps pi of the one-hot test: identity, a seeded random one with pi(i) <= i, and (without the causal mask) the reversal"""
    g = torch.Generator().manual_seed(seed)
    perms = {"identity": torch.arange(S), "lower": (torch.rand(S, generator=g) * (torch.arange(S) + 1)).long()}
    assert bool((perms["lower"] <= torch.arange(S)).all())
    if not causal:
        perms["reversal"] = torch.arange(S - 1, -1, -1)
    return perms


def onehot_inputs(S, B, H, pi, scale, seed):
    """(qkv [B, S, 3 * H * 64], expected [B, S, H * 64]): key j carries the +-alpha binary code of j in its first 10 head dims, query i the
    +-1 code of pi(i): q_i . k_j = alpha (10 - 2 hamming(pi(i), j)), largest at j = pi(i) by 2 alpha.  v is random: the output is v[pi(i)]."""
    assert S <= 1024
    alpha = onehot_alpha(scale)
    g = torch.Generator().manual_seed(seed)
    bits = ((torch.arange(S)[:, None] >> torch.arange(10)[None, :]) & 1).double() * 2 - 1          # [S, 10]
    x = torch.zeros(B, S, 3, H, 64, dtype=torch.float64)
    x[:, :, 0, :, :10] = bits[pi][None, :, None, :]
    x[:, :, 1, :, :10] = alpha * bits[None, :, None, :]
    x[:, :, 2] = torch.randn(B, S, H, 64, generator=g, dtype=torch.float64)
    x = x.float().bfloat16()
    return x.view(B, S, 3 * H * 64), x[:, pi, 2].reshape(B, S, H * 64).clone()


def toeplitz_offsets(S):
    return (-(S - 1), -1, 0, 1, S - 1)


def toeplitz_inputs(S, B, seed):
    """(qkv, rel [5, 2S-1], expected [B, S, 5 * 64], exact [5, S]): q = 0; head h's table is 0 at key - query = d_h and -128 elsewhere, so
    query i sees key i + d_h alone where that key exists (exact[h, i]; expected holds v[i + d_h] there) and all keys alike where not"""
    offs = toeplitz_offsets(S)
    H = len(offs)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, H, 64, generator=g)
    x[:, :, 0] = 0.0
    x = x.bfloat16()
    rel = torch.full((H, 2 * S - 1), -128.0)
    expected = torch.zeros(B, S, H, 64, dtype=torch.bfloat16)
    exact = torch.zeros(H, S, dtype=torch.bool)
    i = torch.arange(S)
    for h, d in enumerate(offs):
        rel[h, d + S - 1] = 0.0
        ok = (i + d >= 0) & (i + d < S)
        exact[h] = ok
        expected[:, i[ok], h] = x[:, i[ok] + d, 2, h]
    return x.view(B, S, 3 * H * 64), rel.bfloat16(), expected.view(B, S, H * 64), exact


def dyadic(x, step=0.125, clip=2.0):
    """x on the grid of multiples of ``step`` within +-clip, as bf16 (exact).  Products of two such values are multiples of step^2 and a
    head's 64 of them sum exactly in float32 in any order, so the kernel's q.k and the restatement's are the same number and round to the
    same bf16 logit: with logits in the thousands one bf16 ulp of a logit is a factor e^16 in its weight, no matter for a tolerance"""
    return (torch.round(x / step).clamp(-clip / step, clip / step) * step).bfloat16()


# ------------------------------------------------------------------ T5LayerNorm
def t5_layernorm(x, w, eps):
    """t5_rmsnorm_kernel: var = mean(x^2), not rounded, with float32's range (a sum past FLT_MAX is inf, rsqrt 0); n = bf16(x * rsqrt(var +
    eps)), eps the float32 the kernel is handed; out = bf16(w * n).  x [M, D] bf16, w [D] bf16"""
    xd = x.double()
    var = _f32_range((xd * xd).sum(-1, keepdim=True)) / x.shape[-1]
    r = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32).double())
    return to_bf16(w.double() * round_bf16(xd * r))


RMS_BLOCK_KINDS = ("gaussian", "zero", "subnormal", "one hot 3e4", "all 3e38", "nan at column 0", "+inf at the last column")


def rms_block(D, seed):
    """(x [12, D] bf16, kinds): three workgroups of four rows; every special row has a finite neighbour in its own workgroup"""
    g = torch.Generator().manual_seed(seed)
    x = (3.0 * torch.randn(12, D, generator=g)).bfloat16()
    kinds = ["gaussian"] * 12
    for r, kind in ((1, "zero"), (2, "subnormal"), (3, "one hot 3e4"), (5, "all 3e38"), (6, "nan at column 0"), (9, "+inf at the last column"),
                    (10, "zero")):
        kinds[r] = kind
        x[r] = 0.0
        if kind == "subnormal":
            x[r] = 2.0 ** -133
        elif kind == "one hot 3e4":
            x[r, D // 3] = 3e4
        elif kind == "all 3e38":
            x[r] = 3e38
        elif kind == "nan at column 0":
            x[r] = (3.0 * torch.randn(D, generator=g)).bfloat16()
            x[r, 0] = math.nan
        elif kind == "+inf at the last column":
            x[r] = (3.0 * torch.randn(D, generator=g)).bfloat16()
            x[r, D - 1] = math.inf
    return x, kinds


def rms_weight(D, seed):
    """weights around 1 with negative and zero entries among them"""
    w = 1.0 + 0.3 * torch.randn(D, generator=torch.Generator().manual_seed(seed))
    w[0::5] = -w[0::5]
    w[3::7] = 0.0
    return w.bfloat16()


# ------------------------------------------------------------------ activations
def new_gelu_chain(x):
    """new_gelu_bf16_chain: NewGELUActivation as torch evaluates it on a bf16 tensor, eight roundings, as float64"""
    x = x.double()
    x3 = round_bf16(round_bf16(x * x) * x)
    a = round_bf16(C_NEW_GELU * x3)
    s = round_bf16(x + a)
    t = round_bf16(C_SQRT_2_PI * s)
    th = round_bf16(torch.tanh(t))
    one = round_bf16(1.0 + th)
    hx = round_bf16(0.5 * x)
    return round_bf16(hx * one)


def quick_gelu_chain(x):
    """quick_gelu_kernel: bf16(x * bf16(sigmoid(bf16(1.702 x)))); the float32 exp is inf past FLT_MAX (sigmoid 0, not a subnormal)"""
    x = x.double()
    z = round_bf16(C_QUICK * x)
    return to_bf16(x * round_bf16(1.0 / (1.0 + _f32_range(torch.exp(-z)))))


_LUT = {}


def _lut(name, fn):
    if name not in _LUT:
        _LUT[name] = fn(all_bf16_patterns())
    return _LUT[name]


def _pattern(x):
    return x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def new_gelu_chain_lut(x):
    """new_gelu_chain through a table over the 65 536 inputs there are (the chain is a function of one bf16 value): the millions of
    elements of a second-trip case cost one lookup each"""
    return _lut("new_gelu", new_gelu_chain)[_pattern(x)]


def gated_new_gelu(h, lut=False):
    """gated_new_gelu_kernel: h [M, 2F] = [a | b] -> bf16(NewGELU chain(a) * b) [M, F].  ``lut``: the chain from the table, and the product
    in float32, where two bf16 values multiply exactly (16 bits of 24), so that its one rounding to bf16 is the same rounding"""
    F = h.shape[1] // 2
    a, b = h[:, :F], h[:, F:]
    if lut:
        return (new_gelu_chain_lut(a).float() * b.float()).bfloat16()
    return to_bf16(new_gelu_chain(a) * b.double())


GATES = (1.0, -1.0, 0.3, 3e38, 0.0)


def gated_all_values():
    """h [5, 2 * 65536]: every bf16 value as the GELU operand, one gate per row"""
    a = all_bf16_patterns()
    return torch.cat([torch.cat([a, torch.full((65536,), gate).bfloat16()])[None] for gate in GATES])


def quick_gelu(x, lut=False):
    return _lut("quick_gelu", quick_gelu_chain)[_pattern(x)] if lut else quick_gelu_chain(x)


# ------------------------------------------------------------------ embedding gather
GATHER_BAD_IDS = (-1, None, 2 ** 40, -2 ** 63)            # None stands for V, the first id past the table


def embed_gather(ids, table, pos=None):
    """embed_gather_kernel: out[b, s] = table[ids[b, s]], a zero row for an id outside [0, V); + pos[s] in one bf16 addition.  [B * S, D]"""
    V, D = table.shape
    B, S = ids.shape
    ok = (ids >= 0) & (ids < V)
    rows = torch.where(ok[..., None], table[ids.clamp(0, V - 1)], torch.zeros((), dtype=table.dtype)).double()
    if pos is not None:
        rows = rows + pos.view(-1, D)[:S].double()[None]
    return to_bf16(rows).view(B * S, D)


def gather_ids(B, S, V, seed):
    """valid ids with 0, V - 1 and every kind of out-of-range id mixed in; (ids [B, S] int64, bad [B, S] bool)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, S), generator=g)
    flat = ids.view(-1)
    spots = torch.randperm(B * S, generator=g)[:16]
    vals = [0, V - 1] + [V if v is None else v for v in GATHER_BAD_IDS]
    for j, p in enumerate(spots.tolist()):
        flat[p] = vals[j % len(vals)]
    flat[0], flat[-1] = -1, V                              # the first and the last row of the launch among them
    return ids, (ids < 0) | (ids >= V)
