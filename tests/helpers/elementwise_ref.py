"""float64 restatements of the kernels of csrc/elementwise.hip with the kernels' own rounding points (csrc/elementwise.hip, the
activations of csrc/drag_common.h), the inputs that tests/test_gpu_elementwise_exact.py feeds the kernels, and the bounds it holds them to.
tests/test_elementwise_restatements_host.py checks all of it without a GPU: the restatements against torch's CPU operators and against
mpmath, and the same restatements evaluated in float32 against the caps on the very inputs the GPU tests use."""
import math
from collections import namedtuple

import torch

ACT_NONE, ACT_GELU_TANH, ACT_SILU, ACT_QUICK_GELU, ACT_GELU_ERF = 0, 1, 2, 3, 4      # domain_rag_amd.ops / include/domainrag_hip.h
ACT_NAMES = {ACT_NONE: "identity", ACT_GELU_TANH: "gelu_tanh", ACT_SILU: "silu", ACT_QUICK_GELU: "quick_gelu", ACT_GELU_ERF: "gelu_erf"}
FLT_MAX = 3.4028234663852886e38
BF16_MAX = 3.3895313892515355e38
EW_GRID_CAP = 2048                       # ew_grid() of csrc/elementwise.hip: at most this many workgroups of 256 lanes
N_SECOND_TRIP_8 = EW_GRID_CAP * 256 * 8 + 8 * 300 + 3     # act / add / flow_euler_step: 8 elements per lane, 300 lanes on a second trip, a tail of 3
N_SECOND_TRIP_1 = EW_GRID_CAP * 256 + 300                 # the casts: one element per lane


# ------------------------------------------------------------------ bf16 rounding of a float64 value, in one step
def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """x (any float dtype) rounded to the nearest bf16 value, ties to even, as float64.  One rounding from float64: torch's own
    double -> bfloat16 goes through float32 and rounds twice.  Past bf16 max the result is inf; below 2^-126 the grid is the subnormals'."""
    x = x.double()
    _, e = torch.frexp(x)                                   # |x| = m * 2^e, m in [0.5, 1): 8 significant bits end at 2^(e-8)
    e = torch.clamp(e, min=-125)                            # subnormals: the grid of the smallest normals, 2^-133
    q = torch.ldexp(torch.ones_like(x), e - 8)
    r = torch.round(x / q) * q                              # torch.round: half to even
    r = torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(x, math.inf), x), r)
    return torch.where(torch.isfinite(x), r, x)


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """round_bf16 as a bfloat16 tensor (both further casts are exact)"""
    return round_bf16(x).float().bfloat16()


def all_bf16_patterns() -> torch.Tensor:
    """the 65 536 bf16 values, element i = bit pattern i"""
    i = torch.arange(65536, dtype=torch.int32)
    return torch.where(i >= 32768, i - 65536, i).to(torch.int16).view(torch.bfloat16)


# ------------------------------------------------------------------ LayerNorm
def layernorm(x, form, *, scale=None, shift=None, gamma=None, beta=None, eps=1e-6, dtype=torch.float64):
    """layernorm_modulate_kernel: x [M, D] bf16 rows; scale / shift [M, D] (each row's own batch already picked), gamma / beta [D].
    The mean and the two-pass variance are not rounded; eps is the float32 the kernel is handed.  What the kernel holds in float32
    has float32's RANGE: a sum past FLT_MAX is inf there (one bf16-max element: the squares' sum is inf, rstd 0, every n a signed zero).
      modulate: bf16(bf16(bf16(n) * bf16(1 + scale)) + shift)      affine: bf16(n * gamma + beta)      plain: bf16(n)
    dtype = float32 evaluates the same statement in the kernel's own precision (in torch's summation order, not the kernel's)."""
    w = x.to(dtype)
    D = w.shape[-1]
    inf = torch.full((), math.inf, dtype=dtype)

    def f32_range(s):
        return torch.where(s.abs() > FLT_MAX, torch.copysign(inf, s), s)
    mean = f32_range(w.sum(-1, keepdim=True)) / D
    d = w - mean
    var = f32_range((d * d).sum(-1, keepdim=True)) / D
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32).to(dtype))
    n = d * rstd
    if form == "plain":
        return to_bf16(n)
    if form == "affine":
        return to_bf16(n * gamma.to(dtype) + beta.to(dtype))
    assert form == "mod"
    nb = round_bf16(n).to(dtype)
    t = round_bf16(1.0 + scale.to(dtype)).to(dtype)
    return to_bf16(round_bf16(nb * t).to(dtype) + shift.to(dtype))


LN_WIDTHS = (8, 64, 504, 512, 520, 768, 1152, 3072, 4088, 4096)
LN_FORMS = ("mod", "affine", "plain")
LnCase = namedtuple("LnCase", "group form D M rpb ldx x_bs ldy ld_mod kind eps seed")


def ln_cases():
    """every LayerNorm launch of the GPU test.  rpb = rows per batch (0: one batch), x_bs = batch stride of x, ld_mod = row stride of the
    modulation buffer (2 D: [shift | scale]; 6 D: a double block's [. . . shift scale .], as flux.py lays it out)"""
    cases = []

    def add(group, form, D, M, kind="normal", rpb=0, ldx=None, x_bs=None, ldy=None, ld_mod=None, eps=1e-6):
        ldx = D if ldx is None else ldx
        x_bs = (rpb if rpb else M) * ldx if x_bs is None else x_bs
        cases.append(LnCase(group, form, D, M, rpb, ldx, x_bs, D if ldy is None else ldy, 2 * D if ld_mod is None else ld_mod, kind, eps,
                            len(cases) + 1))
    for D in LN_WIDTHS:                                     # 8: one lane; 504 / 520 / 4088: a partly filled 512-column pass; 4096: the limit
        for form in LN_FORMS:
            add("widths", form, D, 5, rpb=2)                # three batches, the last one short; the last workgroup has three idle waves
    for M, rpb in ((1, 0), (3, 2), (37, 10)):
        for D in (520, 3072):
            for form in ("mod", "affine"):
                add("rows", form, D, M, rpb=rpb)
    for D in (768, 3072):                                   # rows inside a wider buffer: row stride > D, batch stride > rows_per_batch * ldx
        for form in ("mod", "plain"):
            add("rows", form, D, 15, rpb=5, ldx=D + 8, x_bs=5 * (D + 8) + 64)
    for form in ("affine", "plain"):                        # vit.py's pooled form: row b = token 0 of image b, ldx = T * D, M = B
        add("rows", form, 1152, 5, ldx=7 * 1152)
    for D in (504, 3072, 4088):                             # ldy > D: the columns behind a row keep what they held
        for form in ("mod", "affine"):
            add("rows", form, D, 5, rpb=2, ldy=D + 8)
    for D in (512, 3072):
        add("rows", "mod", D, 7, rpb=3, ld_mod=6 * D)
    for kind, eps in (("offset", 1e-6), ("outlier", 1e-6), ("constant", 1e-6), ("small", 1e-6), ("small", 1e-5), ("extreme", 1e-6)):
        for D in (520, 3072):
            for form in LN_FORMS:
                add("inputs", form, D, 5, kind=kind, rpb=2, eps=eps)
    return cases


def ln_rows(kind, M, D, g):
    """M input rows of one kind, bf16 [M, D]"""
    z = torch.randn(M, D, generator=g)
    if kind == "normal":
        x = 2.0 * z
    elif kind == "offset":                                  # mean = 100 x spread: x - mean cancels seven of bf16's eight bits
        x = 100.0 + z
    elif kind == "outlier":                                 # one element carries nearly all of the variance
        x = z.clone()
        x[torch.arange(M), torch.randint(0, D, (M,), generator=g)] = 1e3
    elif kind == "constant":                                # zero variance: rstd = 1 / sqrt(eps), n = 0
        x = torch.tensor([3.0, -0.1, 0.0, 100.5, -1e-3])[torch.arange(M) % 5, None].expand(M, D)
    elif kind == "small":                                   # variance 1e-6: next to eps = 1e-6 and below eps = 1e-5
        x = 1e-3 * z
    elif kind == "extreme":
        x = z.bfloat16()
        x[0::3, :] = (torch.randint(1, 128, (M, D), generator=g) * torch.where(z > 0, 1.0, -1.0) * 2.0 ** -133).bfloat16()[0::3]   # subnormals
        x[1::3, (D // 3) & ~1] = BF16_MAX                    # the squares' sum leaves float32's range: every output a signed zero
        x[2::3, D - 1] = -BF16_MAX
        return x.contiguous()
    else:
        raise ValueError(kind)
    return x.bfloat16().contiguous()


def ln_case_tensors(c: LnCase):
    """the host side of one case: ``xbuf`` (flat bf16 storage; 777 wherever no row lies), ``rows`` [M, D], ``modbuf`` [batches, ld_mod] with
    ``shift_off`` / ``scale_off`` (the columns of a batch's shift / scale), ``scale`` / ``shift`` [M, D] as row r sees them,
    ``gamma`` / ``beta`` [D], and ``want`` [M, D] bf16, the float64 restatement"""
    g = torch.Generator().manual_seed(1000 + c.seed)
    rows = ln_rows(c.kind, c.M, c.D, g)
    rpb = c.rpb if c.rpb else c.M
    r = torch.arange(c.M)
    b, s = r // rpb, r % rpb
    start = b * c.x_bs + s * c.ldx
    xbuf = torch.full((int(start.max()) + c.D,), 777.0).bfloat16()
    xbuf[(start[:, None] + torch.arange(c.D)[None, :]).reshape(-1)] = rows.reshape(-1)
    nb = int(b.max()) + 1
    t = dict(case=c, xbuf=xbuf, rows=rows, batch=b)
    kw = {}
    if c.form == "mod":
        t["modbuf"] = (0.3 * torch.randn(nb, c.ld_mod, generator=g)).bfloat16()      # every batch its own modulation: a wrong b moves every element
        t["shift_off"], t["scale_off"] = (0, c.D) if c.ld_mod == 2 * c.D else (3 * c.D, 4 * c.D)
        kw = dict(scale=t["modbuf"][b, t["scale_off"]:t["scale_off"] + c.D], shift=t["modbuf"][b, t["shift_off"]:t["shift_off"] + c.D])
    elif c.form == "affine":
        t["gamma"] = (1.0 + 0.3 * torch.randn(c.D, generator=g)).bfloat16()
        t["beta"] = (0.3 * torch.randn(c.D, generator=g)).bfloat16()
        kw = dict(gamma=t["gamma"], beta=t["beta"])
    t["kw"] = kw
    t["want"] = layernorm(rows, c.form, eps=c.eps, **kw)
    return t


# ------------------------------------------------------------------ activations
def act(x: torch.Tensor, kind: int) -> torch.Tensor:
    """the activation's DEFINITION at the bf16 inputs x, in float64, not rounded.  Where a definition subtracts nearly equal numbers
    (1 + tanh u for u < 0, 1 + erf z for z < 0) its exact complement stands in: 1 + tanh u = e^u / cosh u, 1 + erf z = erfc(-z)
    (tests/test_elementwise_restatements_host.py holds both against mpmath).  At -inf every form is -inf * 0 = NaN by its definition
    (torch's own operators say the same); at +inf it is +inf; a NaN stays one; -0 gives -0."""
    x = x.double()
    if kind == ACT_NONE:
        return x
    if kind == ACT_SILU:
        return x * (1.0 / (1.0 + torch.exp(-x)))
    if kind == ACT_QUICK_GELU:
        return x * (1.0 / (1.0 + torch.exp(-1.702 * x)))
    if kind == ACT_GELU_TANH:
        u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)
        un = torch.clamp(u, max=0.0)
        return 0.5 * x * torch.where(u < 0, torch.exp(un) / torch.cosh(un), 1.0 + torch.tanh(u))
    if kind == ACT_GELU_ERF:
        z = x * math.sqrt(0.5)
        return 0.5 * x * torch.where(z < 0, torch.special.erfc(-z), 1.0 + torch.special.erf(z))
    raise ValueError(kind)


def act_floor(x: torch.Tensor, kind: int) -> torch.Tensor:
    """the absolute part of an activation's bound, from the kernel's rounding points (csrc/drag_common.h).
    Sigmoid forms (SiLU, QuickGELU, tanh-GELU = x * sigmoid(2u)): sigmoid is v_rcp_f32(1 + v_exp_f32(..)) on the raw instructions, which flush
    a subnormal result to zero, and 2^(..) past 2^128 is inf with rcp(inf) = 0: a sigmoid under 2^-126 comes out as 0, an absolute error
    under 2^-126 that the product with x scales to |x| * 2^-126.  erf form: erff is within 2 ulp of a value in [0.5, 1], 2 * 2^-24, and
    1 + erff adds no error of its own (both are multiples of 2^-24), so 1 + erff is off by at most 2^-23 absolute; times 0.5 |x|
    that is |x| * 2^-24, and |x| * 2^-23 leaves the product's own two roundings room."""
    ax = x.double().abs()
    if kind == ACT_NONE:
        return torch.zeros_like(ax)
    return ax * (2.0 ** -23 if kind == ACT_GELU_ERF else 2.0 ** -126)


def act_bound(x: torch.Tensor, ref: torch.Tensor, kind: int) -> torch.Tensor:
    """|kernel - ref| <= 2^-8 * max(|ref|, 2^-126) + act_floor(x).  The first term is the output's own rounding, half a bf16 ulp, doubled:
    half an ulp is between 2^-9 |ref| and 2^-8 |ref| for a normal result.  Under 2^-126 the results are bf16 subnormals, whose ulp no
    longer shrinks with |ref| (2^-133, half of it doubled is 2^-8 * 2^-126): there the term stands at that, since a correctly rounded
    result already misses 2^-8 |ref| (the host test shows it)."""
    return 2.0 ** -8 * torch.clamp(ref.abs(), min=2.0 ** -126) + act_floor(x, kind)


def act_check(x: torch.Tensor, got: torch.Tensor, kind: int, what: str, bound=None, normal_too: bool = False):
    """hold bf16 outputs ``got`` of the bf16 inputs ``x`` to the bound; returns max err / bound over the finite references (with
    ``normal_too`` a pair: that, and the same over the references of 2^-126 and more: among the subnormal results a tie, half an ulp of
    2^-133 off, sits at 1.000 of the bound by construction).
    NaN exactly where the definition gives NaN, the same inf where it gives inf, a zero of the same sign where it gives zero."""
    x, got = x.cpu().reshape(-1), got.cpu().reshape(-1)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape, f"{what}: output {got.dtype} {tuple(got.shape)}"
    ref = act(x, kind)
    g = got.double()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(g), nan), f"{what}: NaN outputs differ from the definition's at x = {x[torch.isnan(g) != nan][:8].tolist()}"
    inf = torch.isinf(ref)
    assert bool((g[inf] == ref[inf]).all()), f"{what}: infinite results differ at x = {x[inf][g[inf] != ref[inf]][:8].tolist()}"
    zero = ref == 0
    assert bool(((g[zero] == 0) & (torch.signbit(g[zero]) == torch.signbit(ref[zero]))).all()), f"{what}: a zero of the definition is not that zero"
    fin = ~nan & ~inf
    if kind == ACT_NONE:
        assert torch.equal(g[fin], ref[fin]), f"{what}: the identity changed a value"
        return (0.0, 0.0) if normal_too else 0.0
    bnd = act_bound(x, ref, kind) if bound is None else bound
    ratio = (g[fin] - ref[fin]).abs() / bnd[fin]
    worst = int(ratio.argmax())
    assert float(ratio[worst]) <= 1.0, (f"{what}: err / bound = {float(ratio[worst]):.3f} at x = {float(x[fin][worst])!r}: got {float(g[fin][worst])!r}, "
                                        f"definition {float(ref[fin][worst])!r}; {int((ratio > 1).sum())} inputs past the bound")
    if normal_too:
        normal = ratio[ref[fin].abs() >= 2.0 ** -126]
        return float(ratio[worst]), float(normal.max()) if normal.numel() else 0.0
    return float(ratio[worst])


def act_special_inputs() -> torch.Tensor:
    """n = 7 worth of inputs no launch should go without"""
    return torch.tensor([math.nan, math.inf, -math.inf, -0.0, -88.0, 2.0 ** -130, -3.0]).bfloat16()


# ------------------------------------------------------------------ timestep embedding
TIMESTEPS = (0.0, 1e-3, 1.0, 356.25, 999.9, 1000.0, -7.0)
TIMESTEP_DIMS = (2, 6, 256, 258)
TIMESTEP_K = 12


def timestep_embedding(t: torch.Tensor, dim: int):
    """(ref, angle): [cos(t f_j) | sin(t f_j)], f_j = 10000^(-j / half), in float64 of the float32 times t, not rounded, and |t f_j| twice"""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = t.double()[:, None] * f[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=1), torch.cat([a, a], dim=1).abs()


def timestep_bound(ref, angle):
    """|err| <= 2^-9 |ref| * 2 + k |t f_j| 2^-23 with k = 12, from the float32 steps of timestep_embedding_kernel:
    f = expf(-9.210340371976184f * j / half), a = t * f.  The exponent's argument is at most ln 10000 = 9.2104 and takes two roundings of
    2^-24 each (the product with j, the quotient by half): 9.2104 * 2^-23 absolute.  The constant itself is 9.21034049987793 as a float32,
    1.39e-8 = 0.117 * 2^-23 off in relative terms: another 1.08 * 2^-23 absolute.  An absolute error of the argument is a relative one of
    f.  expf is within 1 ulp, 2^-23 relative; the product t * f rounds once, 0.5 * 2^-23.  9.21 + 1.08 + 1 + 0.5 = 11.8 -> k = 12
    units of 2^-23 relative to the angle a, and cos / sin move by at most the angle's absolute error.  (cosf / sinf's own 2 ulp, 2^-22 |ref|,
    fit the first term: that one is never closer than 2^-16 |ref| to half an ulp.)"""
    return 2.0 ** -9 * ref.abs() * 2 + TIMESTEP_K * angle * 2.0 ** -23


# ------------------------------------------------------------------ add, Euler step
def euler(x: torch.Tensor, v: torch.Tensor, dt: float) -> torch.Tensor:
    """bf16(x + dt * v), dt the float32 that the kernel is handed: rounded once (the kernel's float32 x + dt * v is one fma or two
    roundings, the compiler's choice; either is within 2^-24 of this before the bf16 rounding)"""
    return to_bf16(x.double() + torch.tensor(dt, dtype=torch.float32).double() * v.double())


def euler_f32(x: torch.Tensor, v: torch.Tensor, dt: float) -> torch.Tensor:
    """the two-rounding float32 evaluation (torch has no fused multiply-add to offer): the kernel's other possible self"""
    return (x.float() + torch.tensor(dt, dtype=torch.float32) * v.float()).bfloat16()


def second_trip_inputs(n: int, seed: int):
    """two bf16 vectors of n normal deviates (std 2 and 1); built once per n and seed"""
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.randn(n, generator=g)).bfloat16(), torch.randn(n, generator=g).bfloat16()


def second_trip_spots(n: int, per_lane: int):
    """index ranges worth a look of their own when n elements take a second trip of the grid-stride loop: the end of the first trip, the
    start of the second, the last vector of the second, the scalar tail"""
    first = EW_GRID_CAP * 256 * per_lane
    body = n // per_lane * per_lane
    return {"end of the first trip": (first - 2 * per_lane, first), "start of the second trip": (first, first + 2 * per_lane),
            "end of the second trip": (body - 2 * per_lane, body), "tail": (body if per_lane > 1 else n - 3, n)}


# ------------------------------------------------------------------ casts
def cast_f32_inputs() -> torch.Tensor:
    """float32 inputs of to_bf16: for every bf16 value b, b itself, the tie halfway to the next pattern and that tie's two float32
    neighbours (so: every rounding decision there is, overflow to inf past bf16 max, the float32 subnormals, both infs, and NaNs of
    many payloads), and a few values far above bf16 max"""
    hi = torch.arange(65536, dtype=torch.int64)[:, None] << 16
    lo = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001], dtype=torch.int64)[None, :]
    bits = (hi | lo).reshape(-1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    extra = torch.tensor([FLT_MAX, -FLT_MAX, 3.39e38, -3.39e38, 3.4e38, 1e-45, -1e-45, 1.1754942e-38], dtype=torch.float32)
    return torch.cat([bits.view(torch.float32), extra])
