"""drag_quantize_mxfp8 and drag_gemm_mxfp8 on the GPU: the quantiser byte for byte against the host restatement (domain_rag_amd.mx), the
scaled MFMA's operand map on exact data, the epilogue bit for bit against drag_gemm_bf16's, random data within a derived bound.

"gemm_mx_kernel" selects the kernel; this library builds one (1 = the 128x128 kernel, which the policy, 0, also picks), so every GEMM case
runs under KERNELS = (1,): a second kernel joins the tuple and must then give the same bits on every case of this file."""
import pytest
import torch

pytestmark = pytest.mark.gpu
KERNELS = (1,)            # values of "gemm_mx_kernel" that name a kernel this library builds (2, the wide kernel, is not built)


# ---------------------------------------------------------------------------------------------------------------- quantiser
def _quant_input(kind, rows, K, g):
    if kind == "normal":
        x = torch.randn(rows, K, generator=g)
    elif kind == "outlier":            # one channel 30 x the rest
        x = torch.randn(rows, K, generator=g)
        x[:, 5] *= 30.0
    elif kind == "special":
        # the hand-checked blocks of tests/test_mx_host.py, tiled: amax mantissa exactly 1.75 / just above, all-zero blocks, ties,
        # e4m3 subnormals, clamped exponents
        p = lambda k: 2.0 ** k
        blocks = [[14.0, -14.0, 1.0], [14.0625, 1.0, -3.5], [], [-0.0, 0.0],
                  [256.0, 17.0, 19.0, 2.125, 2.375, -17.0, -19.0, 21.0, 23.0],
                  [256.0, p(-9), p(-10), 3 * p(-10), 5 * p(-9), 7 * p(-10), p(-11), p(-6) - p(-10), -3 * p(-10)],
                  [p(-125), p(-126), 1.5 * p(-127)], [p(-130), p(-133)], [1.75 * p(-119), p(-126)], [1.7578125 * p(-119), p(-125)]]
        x = torch.zeros(rows, K)
        nb = K // 32
        for r in range(rows):
            for b in range(nb):
                vals = blocks[(r * 3 + b) % len(blocks)]
                pos = (r + b) % (32 - 9)                      # the values sit at varying offsets inside the block
                x[r, b * 32 + pos: b * 32 + pos + len(vals)] = torch.tensor(vals)
    elif kind == "extremes":           # bf16's largest values, its subnormals, and everything between by exponent
        big = torch.finfo(torch.bfloat16).max
        x = torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-133, 128, (rows, K), generator=g).float())
        x = x.clamp(-big, big)
        x[:, 0::64] = big
        x[:, 1::64] = -big
        x[:, 40::64] = 2.0 ** -133
    else:
        raise AssertionError(kind)
    return x.bfloat16()


@pytest.mark.parametrize("rows,K", [(1, 128), (1, 1280), (300, 128), (300, 1280)])
@pytest.mark.parametrize("kind", ["special", "normal", "outlier", "extremes"])
def test_quantiser_equals_the_host_restatement_byte_for_byte(gpu, kind, rows, K):
    from domain_rag_amd import mx, ops
    g = torch.Generator().manual_seed(rows * 7 + K)
    x = _quant_input(kind, rows, K, g)
    q_ref, s_ref = mx.quantize_ref(x)
    # through a batched row map: batches of 100 rows, 120 rows apart, row stride K + 8 (the gaps hold NaN bits: never to be read)
    rpb, ld = (100, K + 8) if rows > 1 else (0, K + 8)
    nb = (rows + 99) // 100
    buf = torch.full((nb, 120, ld), float("nan"), dtype=torch.bfloat16)
    for b in range(nb):
        n = min(100, rows - b * 100)
        buf[b, :n, :K] = x[b * 100: b * 100 + n]
    q, s = ops.quantize_mxfp8(buf.to(gpu), M=rows, K=K, lda=ld, rows_per_batch=rpb, batch_stride=120 * ld)
    torch.cuda.synchronize()
    assert q.shape == (rows, K) and s.shape == (rows, K // 32) and q.dtype == s.dtype == torch.uint8
    assert torch.equal(s.cpu(), s_ref), f"scales differ at {(s.cpu() != s_ref).nonzero()[:5].tolist()}"
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} element bytes differ, first at {bad[:5].tolist()}"
    # the dense default form gives the same bytes
    q2, s2 = ops.quantize_mxfp8(x.to(gpu))
    assert torch.equal(q2, q) and torch.equal(s2, s)


# ---------------------------------------------------------------------------------------------------------------- operand map
def _exact_operands(M, K, g):
    """small integers (|v| <= 4) as e4m3 bytes under random per-row, per-block scales 2^-3 .. 2^3"""
    v = torch.randint(-4, 5, (M, K), generator=g).float()
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    s = torch.randint(127 - 3, 127 + 4, (M, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


@pytest.mark.parametrize("M,N,K", [(16, 16, 128),            # one MFMA
                                   (256, 256, 128),          # one K-step: prologue = tail
                                   (300, 264, 384),          # ragged M, edge columns, an odd number of K-steps
                                   (4352, 4096, 256)])       # 1088 tiles (272 of 256 x 256: a persistent kernel's workgroup would walk a second tile)
def test_layout_on_exact_data(gpu, M, N, K):
    """A and W are different random matrices with scales that differ per row and per block, M != N where the shape allows: a swapped
    operand, a transposed output, a wrong block -> lane assignment or a misplaced scale byte all change integers.  Every partial sum is a
    multiple of 2^-6 below 2^18 in magnitude (asserted), so float32 holds each exactly in any order: the result must equal the bf16
    rounding of the float32 CPU product of the dequantised operands bit for bit."""
    from domain_rag_amd import mx, ops
    g = torch.Generator().manual_seed(M + N + K)
    aq, asc = _exact_operands(M, K, g)
    wq, wsc = _exact_operands(N, K, g)
    a, w = mx.dequantize_ref(aq, asc), mx.dequantize_ref(wq, wsc)
    assert float((a.abs() @ w.abs().t()).max()) < 2.0 ** 18
    ref = (a @ w.t()).bfloat16()
    dev = [t.to(gpu) for t in (aq, asc, wq, wsc)]
    outs = []
    for kern in KERNELS:
        with ops.options(gemm_mx_kernel=kern):
            out = ops.gemm_mxfp8(*dev)
        torch.cuda.synchronize()
        bad = (out.cpu().view(torch.int16) != ref.view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"gemm_mx_kernel={kern}: {bad.shape[0]} of {M * N} elements differ, first at {bad[:5].tolist()}: " \
                                 f"{out.cpu()[tuple(bad[0])].item()} vs {ref[tuple(bad[0])].item()}"
        outs.append(out)
    assert all(torch.equal(o, outs[0]) for o in outs)


# ---------------------------------------------------------------------------------------------------------------- epilogue
@pytest.mark.parametrize("form", ["plain", "bias", "bias_gelu_n0", "resid", "gate_resid_batched"])
def test_epilogue_equals_the_bf16_kernels(gpu, form):
    """Integer-valued operands that bf16 and e4m3 both hold (mostly zeros, so the sums stay where GELU bends), unit scales: both GEMMs'
    accumulators are exact and equal, so any difference is an epilogue or addressing bug."""
    from domain_rag_amd import ops
    M, N, K = 600, 264, 256                  # 5 row tiles (the last ragged), 3 column tiles (the last 8 columns wide)
    g = torch.Generator().manual_seed(11)

    def sparse(rows):
        v = torch.randint(-2, 3, (rows, K), generator=g).float()
        return v * (torch.rand(rows, K, generator=g) < 0.15)
    a, w = sparse(M), sparse(N)
    aq, wq = (t.to(torch.float8_e4m3fn).view(torch.uint8).to(gpu) for t in (a, w))
    asc, wsc = (torch.full((r, K // 32), 127, dtype=torch.uint8, device=gpu) for r in (M, N))
    ab, wb = a.bfloat16().to(gpu), w.bfloat16().to(gpu)
    kw = {}
    rows_alloc, ldc = M, N
    if form in ("bias", "bias_gelu_n0"):
        kw["bias"] = torch.randn(N, generator=g).bfloat16().to(gpu)
    if form == "bias_gelu_n0":
        kw.update(act=ops.ACT_GELU_TANH, act_n0=136)        # the activation starts inside the second column tile
    if form == "resid":
        kw["resid"] = torch.randn(M, N, generator=g).bfloat16().to(gpu)
    if form == "gate_resid_batched":
        # two batches of 300 rows, 320 rows apart: the tile of rows 256 .. 383 straddles the batch boundary
        rows_alloc, ldc = 640, N + 8
        kw.update(bias=torch.randn(N, generator=g).bfloat16().to(gpu), gate=torch.randn(2, N + 16, generator=g).bfloat16().to(gpu), ldg=N + 16,
                  resid=torch.randn(rows_alloc, ldc, generator=g).bfloat16().to(gpu), c_rows_per_batch=300, c_batch_stride=320 * ldc)
    fill = torch.full((rows_alloc, ldc), -7.0, dtype=torch.bfloat16, device=gpu)       # untouched elements must stay as they were
    for narrow in (0, 1):                    # the staged 16-byte epilogue, and the fragment-layout one ("gemm_narrow")
        with ops.options(gemm_narrow=narrow):
            ref = fill.clone()
            ops.gemm(ab, wb, out=ref, M=M, ldc=ldc, **kw)
            assert not torch.equal(ref, fill)
            for kern in KERNELS:
                out = fill.clone()
                with ops.options(gemm_mx_kernel=kern):
                    ops.gemm_mxfp8(aq, asc, wq, wsc, out, M=M, ldc=ldc, **kw)
                torch.cuda.synchronize()
                bad = (out.view(torch.int16) != ref.view(torch.int16)).nonzero()
                assert bad.numel() == 0, f"gemm_mx_kernel={kern}, gemm_narrow={narrow}, {form}: {bad.shape[0]} elements differ, first at {bad[:5].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- random data
def _student_t3(shape, g):
    z = torch.randn(*shape, generator=g)
    c = torch.randn(3, *shape, generator=g).pow(2).mean(dim=0)
    return z / c.sqrt()


@pytest.mark.parametrize("M,N,K", [(513, 768, 1280), (1024, 1024, 3072)])
@pytest.mark.parametrize("dist", ["normal", "student_t3"])
def test_random_data_within_the_derived_bound(gpu, dist, M, N, K):
    """Against the float64 product of the dequantised operands: |err| <= 2^-8 |ref| + K 2^-23 sum |a_i w_i| — half a bf16 ulp, doubled, plus
    the worst-case bound of a sequential float32 accumulation (K u sum |a_i w_i| with u = 2^-24), doubled.  Derived, not tuned."""
    from domain_rag_amd import mx, ops
    g = torch.Generator().manual_seed(K + (dist == "normal"))
    draw = (lambda *s: torch.randn(*s, generator=g)) if dist == "normal" else (lambda *s: _student_t3(s, g))
    a, w = draw(M, K).bfloat16(), draw(N, K).bfloat16()
    aq, asc = ops.quantize_mxfp8(a.to(gpu))
    wq, wsc = ops.quantize_mxfp8(w.to(gpu))
    ad, wd = mx.dequantize_ref(aq, asc).double(), mx.dequantize_ref(wq, wsc).double()
    ref = ad @ wd.t()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (ad.abs() @ wd.abs().t())
    outs = []
    for kern in KERNELS:
        with ops.options(gemm_mx_kernel=kern):
            out = ops.gemm_mxfp8(aq, asc, wq, wsc)
        torch.cuda.synchronize()
        err = (out.cpu().double() - ref).abs()
        worst = float((err / bound).max())
        print(f"gemm_mx_kernel={kern} {dist} {(M, N, K)}: max err / bound = {worst:.4f}")
        assert worst <= 1.0, f"gemm_mx_kernel={kern}: error is {worst:.3f} x the bound"
        outs.append(out)
    assert all(torch.equal(o, outs[0]) for o in outs)


def test_argument_checks(gpu):
    from domain_rag_amd import ops
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.quantize_mxfp8(torch.zeros(4, 96, dtype=torch.bfloat16, device=gpu))               # K % 128
    with pytest.raises(ValueError):
        ops.gemm_mxfp8(u8(16, 128), u8(16, 4), u8(16, 128), u8(16, 8))                       # scale shape
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.gemm_mxfp8(u8(16, 128), u8(16, 4), u8(12, 128), u8(12, 4))                       # N % 8
    with ops.options(gemm_mx_kernel=2):
        with pytest.raises(RuntimeError, match="not built"):
            ops.gemm_mxfp8(u8(16, 128), u8(16, 4), u8(16, 128), u8(16, 4))
    out = torch.zeros(16, 16, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="gemm_mxfp8.out"):                                   # a batched row map that leaves the destination
        ops.gemm_mxfp8(u8(16, 128), u8(16, 4), u8(16, 128), u8(16, 4), out, c_rows_per_batch=8, c_batch_stride=512, ldc=16)
    with pytest.raises(ValueError, match="gemm_mxfp8.resid"):
        ops.gemm_mxfp8(u8(16, 128), u8(16, 4), u8(16, 128), u8(16, 4), out, resid=torch.zeros(8, 16, dtype=torch.bfloat16, device=gpu))
    with pytest.raises(ValueError, match="2-D"):
        ops.quantize_mxfp8(torch.zeros(2, 4, 128, dtype=torch.bfloat16, device=gpu))


def test_a_short_last_batch_is_checked_against_the_full_batch_before_it(gpu):
    """K = 128, five rows in batches of four that lie 8 elements apart: the last row ends at element 136, row 3 of batch 0 at 512"""
    from domain_rag_amd import ops
    short = torch.zeros(136 + 8, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match=r"quantize_mxfp8\.x"):
        ops.quantize_mxfp8(short, M=5, K=128, lda=128, rows_per_batch=4, batch_stride=8)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=gpu)
    operands = (u8(5, 128), u8(5, 4), u8(128, 128), u8(128, 4))
    with pytest.raises(ValueError, match=r"gemm_mxfp8\.out"):
        ops.gemm_mxfp8(*operands, short, M=5, ldc=128, c_rows_per_batch=4, c_batch_stride=8)
    with pytest.raises(ValueError, match=r"gemm_mxfp8\.resid"):
        ops.gemm_mxfp8(*operands, torch.zeros(512, dtype=torch.bfloat16, device=gpu), resid=short, M=5, ldc=128, c_rows_per_batch=4, c_batch_stride=8)
    assert not short.any()
