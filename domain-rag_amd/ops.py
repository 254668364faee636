"""Thin Python wrappers over the C ABI (include/domainrag_hip.h).

Tensors are torch CUDA(ROCm) tensors used only as device-memory handles: every wrapper hands raw
pointers + sizes to libdomainrag_hip.so on torch's current stream.  No arithmetic is done by torch
here, and nothing falls back to torch when the library is missing (``_lib.load()`` raises).
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch

from . import _lib
from ._lib import GemmArgs, GemmMxArgs, check

ACT_NONE, ACT_GELU_TANH, ACT_SILU, ACT_QUICK_GELU, ACT_GELU_ERF = 0, 1, 2, 3, 4


class GemmRecorder:
    """Per-launch timing of the GEMM kernel with events on the launch stream (bench.py's roofline).  ``every`` = n
    samples the denoise loop: the GEMMs of every n-th DiT step are bracketed (all steps launch the same shapes), the
    other steps run the way the product does (hipGraph replay, no events) so the timed region is not slowed by ~16k
    event records."""

    def __init__(self, every: int = 1, f32: bool = False):
        self.every = max(1, int(every))
        self.f32 = f32              # also bracket the float32 matrix-core launches (conv2d_f32_kernel: the CLIP tower, LaMa)
        self.events = []
        self.shapes = []
        self.is_conv = []
        self.attn = []              # (start, end, flops, kernel name) of the bf16 attention launches of the sampled steps

    def totals(self):
        torch.cuda.synchronize()
        flops = sum(f for _, _, f in self.events)
        ms = sum(s.elapsed_time(e) for s, e, _ in self.events)
        return flops, ms, len(self.events)

    @staticmethod
    def kernel_of(shape, conv=False):
        """the kernel drag_gemm_bf16 / drag_gemm_bf16_pair / drag_conv3x3_bf16 dispatch this launch to (``drag_gemm_bf16_choice``:
        the library's own tile policy); ``conv`` = ("pair", M1, M2) for a merged pair launch"""
        if conv == "f32":
            return "conv2d_f32_kernel"
        if conv == "mx":                                     # drag_gemm_mxfp8: one kernel so far
            return "gemm_mxfp8_simple"
        M, N, K = shape
        if isinstance(conv, tuple) and conv[0] == "splitk":  # drag_gemm_bf16 as stacked K slices + the reduce pass (one recorded interval)
            return "gemm_bf16_w4p + splitk_reduce_kernel"
        M1, M2 = (conv[1], conv[2]) if isinstance(conv, tuple) else (M, 0)
        lib = _lib.load()
        if conv is True:                                     # the 3x3 convolutions take t256 or t128 only, by their own predicate
            code, form = lib.drag_conv3x3_bf16_choice(M, N, K // 9), 2
        else:
            code, form = lib.drag_gemm_bf16_choice(M1, M2, N, K), int(M2 > 0)
        # the name from the library's kernel table; a merged pair runs the rows kernel where the code has no pair kernel of its own
        name = lib.drag_gemm_bf16_kernel_name(code, form) or lib.drag_gemm_bf16_kernel_name(code, 0)
        if name is None:
            raise RuntimeError(f"gemm kernel code {code} is not built (drag_gemm_bf16_kernel_code enumerates the codes that are)")
        return name.decode()

    def by_kernel(self):
        """{kernel name: (launches, total_ms, flops)}"""
        torch.cuda.synchronize()
        agg: dict = {}
        for (s, e, f), shp, cv in zip(self.events, self.shapes, self.is_conv):
            a = agg.setdefault(self.kernel_of(shp, cv), [0, 0.0, 0.0])
            a[0] += 1; a[1] += s.elapsed_time(e); a[2] += f
        return agg

    def attention_by_kernel(self):
        """{kernel name: (launches, total_ms, flops)} of the recorded drag_attention*_bf16 launches"""
        torch.cuda.synchronize()
        agg: dict = {}
        for s, e, f, name in self.attn:
            a = agg.setdefault(name, [0, 0.0, 0.0])
            a[0] += 1; a[1] += s.elapsed_time(e); a[2] += f
        return agg

    def by_shape(self):
        """{(M, N, K): (launches, total_ms, TFLOP/s)} sorted by total time"""
        torch.cuda.synchronize()
        agg: dict = {}
        for (s, e, f), shp in zip(self.events, self.shapes):
            a = agg.setdefault(shp, [0, 0.0, 0.0])
            a[0] += 1; a[1] += s.elapsed_time(e); a[2] += f
        return sorted(((k, v[0], v[1], v[2] / (v[1] * 1e-3) / 1e12 if v[1] > 0 else 0.0) for k, v in agg.items()), key=lambda r: -r[2])


_recorder: GemmRecorder | None = None


def set_recorder(rec: GemmRecorder | None) -> None:
    global _recorder
    _recorder = rec


def set_option(name: str, value: int) -> None:
    """Set one of the library's measurement switches (``drag_set_option``) for the whole process, from the next launch on.  The comment of
    ``drag_set_option`` in include/domainrag_hip.h is the list of names, values and defaults (``drag_option_name`` enumerates the names);
    an unknown name, or a value that only an experiment build carries, raises RuntimeError.  Tests and A/B scripts switch with
    ``options(...)``, which puts the previous values back."""
    check(_lib.load().drag_set_option(name.encode(), int(value)), "drag_set_option")


def get_option(name: str) -> int:
    """current value of a measurement switch (``drag_get_option``)"""
    v = ctypes.c_int32()
    check(_lib.load().drag_get_option(name.encode(), ctypes.byref(v)), "drag_get_option")
    return v.value


@contextlib.contextmanager
def options(**values: int):
    """``with ops.options(gemm_kernel=1, gemm_pair=2): ...`` — set switches for the block and put back what they held before it (in reverse
    order, also when the block raises or a later switch of the list is refused)"""
    old = []
    try:
        for name, v in values.items():
            prev = get_option(name)
            set_option(name, v)
            old.append((name, prev))
        yield
    finally:
        for name, prev in reversed(old):
            set_option(name, prev)


def experiments_built() -> bool:
    """True when libdomainrag_hip.so was built with DRAG_EXPERIMENTS=1 (csrc/drag_common.h): only then does it carry the kernels behind
    "attn_persist", "attn_sched" = 3 and "topk_qt" — measured non-improvements kept for their A/B records, not product code"""
    return bool(_lib.load().drag_experiments_built())        # a pure query: no option is read or written


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _need(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (domain-rag_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _room(t: torch.Tensor) -> int:
    """elements of ``t``'s storage from its first element on"""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _batches(M: int, rows_per_batch: int) -> int:
    """batches that the M rows of a batched-row map fall into (``_rows_reach``)"""
    return -(-M // rows_per_batch) if 0 < rows_per_batch < M else 1


def _rows_reach(M: int, cols: int, ld: int, rows_per_batch: int = 0, batch_stride: int = 0) -> int:
    """elements, counted from an operand's first one, that M logical rows of ``cols`` elements address under the library's batched-row map
    (``drag_gemm_bf16``, ``drag_quantize_mxfp8``, ``drag_layernorm_modulate_bf16``): row r at (r // rpb) * batch_stride + (r % rpb) * ld with
    rpb = ``rows_per_batch`` if 0 < ``rows_per_batch`` < M, else M (one batch).  One more than the largest offset for strides >= 0 (a negative
    one is the caller's to refuse); pure integers, tests/test_rows_reach_host.py enumerates the addresses."""
    if M <= 0 or cols <= 0:
        return 0
    rpb = rows_per_batch if 0 < rows_per_batch < M else M
    b, s = divmod(M - 1, rpb)                               # the last row's batch and row in it
    last = b * batch_stride + s * ld
    if b > 0:                                               # a short last batch: the full batch before it may reach further
        last = max(last, (b - 1) * batch_stride + (rpb - 1) * ld)
    return last + cols


def _fit(t: torch.Tensor, reach: int, what: str, *row_map: int) -> None:
    """the ``reach`` elements that a launch addresses from ``t``'s first one must lie inside its storage: a wrong stride is an error here,
    not a memory fault in the kernel.  ``row_map``: ``_rows_reach``'s arguments, for the message."""
    if reach > _room(t):
        how = f" ({row_map[0]} rows of {row_map[1]}; row stride, rows per batch, batch stride: {row_map[2:]})" if row_map else ""
        raise ValueError(f"{what}: the launch addresses {reach} elements from its start{how}, the tensor holds {_room(t)}")


def _linear_fit(what: str, M: int, N: int, cols: int, out, resid, bias, gate, ldc: int, rows_per_batch: int, batch_stride: int, ldg: int) -> None:
    """the destination side of a Linear (``gemm``, ``gemm_mxfp8``): ``out`` and ``resid`` hold M rows of ``cols`` under the destination's row
    map, ``bias`` N elements, ``gate`` one row of N per batch, ``ldg`` apart"""
    reach = _rows_reach(M, cols, ldc, rows_per_batch, batch_stride)
    _fit(out, reach, what + ".out", M, cols, ldc, rows_per_batch, batch_stride)
    if resid is not None:
        _fit(resid, reach, what + ".resid", M, cols, ldc, rows_per_batch, batch_stride)
    if bias is not None:
        _fit(bias, N, what + ".bias")
    if gate is not None:
        nb = _batches(M, rows_per_batch)
        _fit(gate, _rows_reach(nb, N, ldg), what + ".gate", nb, N, ldg)


def _gemm_args(a, w, out=None, *, bias=None, act=ACT_NONE, act_n0=0, gate=None, resid=None, out_f32=False, M=None, a_rows_per_batch=0,
               a_batch_stride=0, lda=None, c_rows_per_batch=0, c_batch_stride=0, ldc=None, ldg=0, out2=None, ldc2=0, n_split=0):
    """(GemmArgs, out, (M, N, K)) of one Linear (argument meaning: ``gemm``)"""
    _need(a, torch.bfloat16, "gemm.a")
    _need(w, torch.bfloat16, "gemm.w")
    N, K = w.shape
    if not w.is_contiguous():
        raise ValueError("gemm.w must be contiguous [N, K]")
    if M is None:
        M = a.numel() // K
        if lda is None:
            if a.dim() < 2 or a.stride(-1) != 1:
                raise ValueError("gemm.a must have unit inner stride")
            lda = a.stride(-2) if a.dim() >= 2 else K
    if lda is None:
        lda = K
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32 if out_f32 else torch.bfloat16, device=a.device)
    if ldc is None:
        # a 2-D destination carries its own row stride (a two-destination launch writes n_split columns into `out`, not N: defaulting to N
        # there wrote past the tensor — round 5, found as a GPU memory fault by a test that forgot ldc)
        ldc = out.stride(-2) if out.dim() >= 2 and out.stride(-1) == 1 else N
    _fit(a, _rows_reach(M, K, lda, a_rows_per_batch, a_batch_stride), "gemm.a", M, K, lda, a_rows_per_batch, a_batch_stride)
    if out2 is None:
        _linear_fit("gemm", M, N, N, out, resid, bias, gate, ldc, c_rows_per_batch, c_batch_stride, ldg)
    elif 0 < n_split < N and n_split % 256 == 0:            # (an invalid n_split is the library's to report)
        _linear_fit("gemm", M, N, n_split, out, resid, bias, gate, ldc, c_rows_per_batch, c_batch_stride, ldg)
        _fit(out2, _rows_reach(M, N - n_split, ldc2), "gemm.out2", M, N - n_split, ldc2)
    args = GemmArgs()
    args.A, args.W, args.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    args.bias = bias.data_ptr() if bias is not None else None
    args.gate = gate.data_ptr() if gate is not None else None
    args.resid = resid.data_ptr() if resid is not None else None
    args.M, args.N, args.K = M, N, K
    args.lda, args.a_rows_per_batch, args.a_batch_stride = lda, a_rows_per_batch, a_batch_stride
    args.ldc, args.c_rows_per_batch, args.c_batch_stride = ldc, c_rows_per_batch, c_batch_stride
    args.ldg, args.act, args.act_n0, args.out_f32 = ldg, act, act_n0, int(out_f32)
    if out2 is not None:        # columns >= n_split go to out2 (dense rows of ldc2 elements)
        _need(out2, torch.bfloat16, "gemm.out2")
        args.C2, args.ldc2, args.n_split = out2.data_ptr(), ldc2, n_split
    return args, out, (M, N, K)


def _bracketed(call, f32: bool = False):
    """run ``call``; with a recorder installed (for a float32 launch: one that takes those) between two timing events on the launch stream,
    and return the pair"""
    if _recorder is None or (f32 and not _recorder.f32):
        call()
        return None
    s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s_ev.record()
    call()
    e_ev.record()
    return s_ev, e_ev


def _recorded(call, shape, kind=False):
    """run one matrix-core launch of 2 M N K flops (``shape``), recorded when a recorder is installed; ``kind``: ``GemmRecorder.kernel_of``"""
    ev = _bracketed(call, kind == "f32")
    if ev is not None:
        M, N, K = shape
        _recorder.events.append((*ev, 2.0 * M * N * K))
        _recorder.shapes.append(shape)
        _recorder.is_conv.append(kind)


def _recorded_attention(call, B, S, H, qprep, vrow, mx=False):
    """run one head_dim-128 attention launch, recorded when a recorder is installed (4 S^2 128 flops per batch and head: q k^T and p v;
    the kernel name from the library's own dispatch, ``drag_attention_bf16_kernel_name``)"""
    if _recorder is not None:   # the name before the launch: what the launch is about to read is what gets reported
        lib = _lib.load()
        name = (lib.drag_attention_mxfp8_kernel_name(S) if mx else lib.drag_attention_bf16_kernel_name(S, int(vrow), int(qprep))).decode()
    ev = _bracketed(call)
    if ev is not None:
        _recorder.attn.append((*ev, 4.0 * S * S * 128 * H * B, name))


_gemm_workspaces: dict[int, torch.Tensor] = {}
_retired_workspaces: list[torch.Tensor] = []      # replaced workspaces stay alive: captured graphs may still hold their addresses
_workspace_stream: dict[int, int] = {}            # device -> the stream whose launches last used the workspace


def _workspace_guard(a: torch.Tensor) -> None:
    """the library picks the workspace of hipGetDevice() and one buffer serves every stream of a device: refuse a launch whose operands
    live on another device than the current one, and order a launch on a NEW stream behind the previous stream's work (split launches
    on two streams would otherwise race on the partial sums).  Nothing is recorded during capture: a graph is one stream's work."""
    idx = a.device.index
    if idx != torch.cuda.current_device():
        raise RuntimeError(f"gemm: operands on cuda:{idx} but the current device is cuda:{torch.cuda.current_device()} "
                           "(the library launches on — and takes the split-K workspace of — the current device)")
    if torch.cuda.is_current_stream_capturing():
        return
    st = torch.cuda.current_stream()
    last = _workspace_stream.get(idx)
    if last is not None and last != st.cuda_stream:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.ExternalStream(last, device=a.device) if last != 0 else torch.cuda.default_stream(a.device))
        st.wait_event(ev)
    _workspace_stream[idx] = st.cuda_stream


def gemm_workspace(device: torch.device, mbytes: int | None = None) -> None:
    """register this device's split-K workspace with the library (``drag_gemm_set_workspace``): ``gemm`` does it once per device with
    $DRAG_GEMM_WORKSPACE_MB (default 64; 0 = none, no launch is split) — a Linear of few output tiles and a long K (batch-1 proj_out /
    ff down-projections) then runs as stacked K slices + one reduce pass.  Not taken during stream capture (the buffer must outlive the
    graph: call this before capturing)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if mbytes is None:
        mbytes = int(os.environ.get("DRAG_GEMM_WORKSPACE_MB", "64"))
    lib = _lib.load()
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("gemm_workspace: not during stream capture (the buffer must outlive the graph: register it before capturing)")
    old = _gemm_workspaces.get(idx)
    if old is not None and old.numel() > 0:
        # a hipGraph captured while `old` was registered replays launches that hold its address (flux.forward_graphed): the buffer is
        # retired, not freed — a re-registration costs memory, never a use-after-free on replay
        _retired_workspaces.append(old)
    with torch.cuda.device(idx):
        if mbytes <= 0:
            _gemm_workspaces[idx] = torch.empty(0, dtype=torch.uint8, device=device)
            check(lib.drag_gemm_set_workspace(None, 0), "drag_gemm_set_workspace")
            return
        ws = torch.empty(mbytes << 20, dtype=torch.uint8, device=device)
        check(lib.drag_gemm_set_workspace(ctypes.c_void_p(ws.data_ptr()), ws.numel()), "drag_gemm_set_workspace")
        _gemm_workspaces[idx] = ws


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None, *, bias=None, act: int = ACT_NONE,
         act_n0: int = 0, gate=None, resid=None, out_f32: bool = False, M: int | None = None,
         a_rows_per_batch: int = 0, a_batch_stride: int = 0, lda: int | None = None,
         c_rows_per_batch: int = 0, c_batch_stride: int = 0, ldc: int | None = None, ldg: int = 0,
         out2: torch.Tensor | None = None, ldc2: int = 0, n_split: int = 0) -> torch.Tensor:
    """out = epi(a @ w.T) (``out2``: output columns >= ``n_split`` are written there instead, as dense rows of ``ldc2``
    elements).  ``a`` / ``out`` may be views into larger buffers: pass the logical row
    count ``M`` and the batched-row addressing (rows_per_batch, batch_stride, ld) explicitly; by
    default ``a`` is a dense [M, K] matrix and ``out`` a dense [M, N] one."""
    lib = _lib.load()
    if a.is_cuda and a.device.index not in _gemm_workspaces and not torch.cuda.is_current_stream_capturing():
        gemm_workspace(a.device)
    if a.is_cuda:
        _workspace_guard(a)
    args, out, shape = _gemm_args(a, w, out, bias=bias, act=act, act_n0=act_n0, gate=gate, resid=resid, out_f32=out_f32, M=M,
                                  a_rows_per_batch=a_rows_per_batch, a_batch_stride=a_batch_stride, lda=lda, c_rows_per_batch=c_rows_per_batch,
                                  c_batch_stride=c_batch_stride, ldc=ldc, ldg=ldg, out2=out2, ldc2=ldc2, n_split=n_split)
    slices = lib.drag_gemm_bf16_splitk_slices(ctypes.byref(args)) if _recorder is not None else 0
    _recorded(lambda: check(lib.drag_gemm_bf16(ctypes.byref(args), _stream()), "drag_gemm_bf16"), shape, ("splitk", slices) if slices else False)
    return out


def gemm_cost(M: int, N: int, K: int, M2: int = 0) -> int:
    """the tile policy's cost of one launch (``drag_gemm_bf16_cost``: tile rounds on the busiest CU x (tile rows + columns)) —
    comparable between launches of equal K; used to choose between one fused launch and two"""
    return int(_lib.load().drag_gemm_bf16_cost(M, M2, N, K))


def gemm_pair(first: dict, second: dict):
    """Two Linears with their own operands and the same N, K, activation and output type (``drag_gemm_bf16_pair``): ``first`` /
    ``second`` are the keyword arguments of ``gemm`` (``a``, ``w``, ``out`` included).  One launch unless both problems fill the chip
    alone; bit-identical to ``gemm(**first); gemm(**second)`` either way.  A FluxTransformerBlock's image-stream / text-stream
    pairs (to_q|k|v + add_q|k|v_proj, to_out + to_add_out, ff + ff_context)."""
    lib = _lib.load()
    two_dest = {"out2", "ldc2", "n_split"} & (first.keys() | second.keys())
    if two_dest:
        raise TypeError(f"gemm_pair: unexpected arguments {sorted(two_dest)} (a pair has no two-destination form)")
    (a1, o1, s1), (a2, o2, s2) = _gemm_args(**first), _gemm_args(**second)
    if s1[1:] != s2[1:]:
        raise ValueError(f"gemm_pair: the two problems must share N and K (got {s1} and {s2})")
    if (a1.act, a1.act_n0, a1.out_f32) != (a2.act, a2.act_n0, a2.out_f32):
        raise ValueError("gemm_pair: the two problems must share activation, act_n0 and output type")
    if first["a"].is_cuda and first["a"].device.index not in _gemm_workspaces and not torch.cuda.is_current_stream_capturing():
        gemm_workspace(first["a"].device)
    if first["a"].is_cuda:
        _workspace_guard(first["a"])
    slices = lib.drag_gemm_bf16_pair_splitk_slices(ctypes.byref(a1), ctypes.byref(a2))
    if slices:                   # one partial launch over both problems' rows + a reduce pass each (one recorded interval)
        _recorded(lambda: check(lib.drag_gemm_bf16_pair(ctypes.byref(a1), ctypes.byref(a2), _stream()), "drag_gemm_bf16_pair"),
                  (s1[0] + s2[0], s1[1], s1[2]), ("splitk", slices))
    elif lib.drag_gemm_bf16_pair_merges(s1[0], s2[0], s1[1], s1[2]):
        _recorded(lambda: check(lib.drag_gemm_bf16_pair(ctypes.byref(a1), ctypes.byref(a2), _stream()), "drag_gemm_bf16_pair"),
                  (s1[0] + s2[0], s1[1], s1[2]), ("pair", s1[0], s2[0]))
    else:       # two launches (what the library would issue itself), accounted one by one
        for args_i, s_i in ((a1, s1), (a2, s2)):
            sl = lib.drag_gemm_bf16_splitk_slices(ctypes.byref(args_i)) if _recorder is not None else 0
            _recorded(lambda: check(lib.drag_gemm_bf16(ctypes.byref(args_i), _stream()), "drag_gemm_bf16"), s_i, ("splitk", sl) if sl else False)
    return o1, o2


def quantize_mxfp8(x: torch.Tensor, *, M: int | None = None, K: int | None = None, lda: int | None = None, rows_per_batch: int = 0,
                   batch_stride: int = 0, out=None):
    """bf16 rows -> OCP MXFP8 ``(q, s)`` (``drag_quantize_mxfp8``): ``q`` uint8 [M, K] e4m3fn bytes, ``s`` uint8 [M, K / 32] e8m0 bytes,
    both dense.  ``x`` may be a view into a larger buffer: pass the logical row count ``M``, the width ``K`` and the batched-row
    addressing (``lda``, ``rows_per_batch``, ``batch_stride``) as for ``gemm``'s ``a``; by default ``x`` is a dense [M, K] matrix.
    ``out`` = (q, s) buffers to write into (at least M * K and M * K / 32 bytes).  The rule: :mod:`.mx`."""
    _need(x, torch.bfloat16, "quantize_mxfp8.x")
    if K is None:
        K = x.shape[-1]
    if M is None:
        if x.dim() != 2 or x.stride(-1) != 1 or x.shape[1] != K:
            raise ValueError("quantize_mxfp8.x: without M, a 2-D [M, K] matrix with unit inner stride is expected (pass M and the row map for a view)")
        M = x.shape[0]
        if lda is None:
            lda = x.stride(0)
    if lda is None:
        lda = K
    if K % 128:
        raise ValueError(f"quantize_mxfp8: K = {K} must be a multiple of 128")
    _fit(x, _rows_reach(M, K, lda, rows_per_batch, batch_stride), "quantize_mxfp8.x", M, K, lda, rows_per_batch, batch_stride)
    if out is None:
        q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
        s = torch.empty((M, K // 32), dtype=torch.uint8, device=x.device)
    else:
        q, s = out
        _need(q, torch.uint8, "quantize_mxfp8.out[0]")
        _need(s, torch.uint8, "quantize_mxfp8.out[1]")
        if not (q.is_contiguous() and s.is_contiguous()) or q.numel() < M * K or s.numel() < M * (K // 32):
            raise ValueError("quantize_mxfp8.out: contiguous buffers of at least M * K and M * K / 32 bytes")
    check(_lib.load().drag_quantize_mxfp8(_p(x), M, K, lda, rows_per_batch, batch_stride, _p(q), _p(s), _stream()), "drag_quantize_mxfp8")
    return q, s


def lora_merge(w0: torch.Tensor, w: torch.Tensor, up: torch.Tensor, down: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``w <- bf16(f32(w0) + sum_r scale[r] * up[:, r] * down[r, :])`` (``drag_lora_merge_bf16``; the rule: :func:`.lora.merge_ref`):
    ``w0`` / ``w`` bf16 [N, K], ``up`` bf16 [N, R], ``down`` bf16 [R, K], ``scale`` float32 [R], one factor per rank column.  Every matrix
    may be a row-strided view with unit inner stride (a row slice of a stacked weight); ``w is w0`` (same address and row stride) merges in
    place, otherwise the two must not overlap.  Not during stream capture: the launch changes weights that captured graphs only read."""
    for t, name in ((w0, "w0"), (w, "w"), (up, "up"), (down, "down")):
        _need(t, torch.bfloat16, "lora_merge." + name)
        if t.dim() != 2 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"lora_merge.{name}: a 2-D matrix with unit inner stride and non-overlapping rows expected")
    _need(scale, torch.float32, "lora_merge.scale")
    N, K = w.shape
    R = down.shape[0]
    if tuple(w0.shape) != (N, K) or tuple(up.shape) != (N, R) or down.shape[1] != K or R < 1:
        raise ValueError(f"lora_merge: w0 {tuple(w0.shape)}, w {tuple(w.shape)}, up {tuple(up.shape)}, down {tuple(down.shape)} do not fit "
                         "[N, K], [N, K], [N, R], [R, K]")
    if scale.dim() != 1 or scale.numel() != R or not scale.is_contiguous():
        raise ValueError(f"lora_merge.scale: a dense vector of R = {R} factors expected, got {tuple(scale.shape)}")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("lora_merge: not during stream capture (a merge belongs between forwards, not into a graph)")
    # (a single row has no stride of its own: the width, rounded up to the 16-byte pieces the kernel moves)
    ldw0, ldw, ldup, lddown = (t.stride(0) if t.shape[0] > 1 else -(-t.shape[1] // 8) * 8 for t in (w0, w, up, down))
    _fit(w0, _rows_reach(N, K, ldw0), "lora_merge.w0", N, K, ldw0)
    _fit(w, _rows_reach(N, K, ldw), "lora_merge.w", N, K, ldw)
    _fit(up, _rows_reach(N, R, ldup), "lora_merge.up", N, R, ldup)
    _fit(down, _rows_reach(R, K, lddown), "lora_merge.down", R, K, lddown)
    if not (w.data_ptr() == w0.data_ptr() and ldw == ldw0):
        a0, a1 = w0.data_ptr(), w0.data_ptr() + 2 * _rows_reach(N, K, ldw0)
        b0, b1 = w.data_ptr(), w.data_ptr() + 2 * _rows_reach(N, K, ldw)
        if a0 < b1 and b0 < a1:
            raise ValueError("lora_merge: w and w0 overlap (only the in-place form, same address and row stride, may share memory)")
    check(_lib.load().drag_lora_merge_bf16(_p(w0), ldw0, _p(w), ldw, N, K, _p(up), ldup, _p(down), lddown, _p(scale), R, _stream()),
          "drag_lora_merge_bf16")
    return w


def gemm_mxfp8(aq: torch.Tensor, ascale: torch.Tensor, wq: torch.Tensor, wscale: torch.Tensor, out: torch.Tensor | None = None, *,
               bias=None, act: int = ACT_NONE, act_n0: int = 0, gate=None, resid=None, M: int | None = None,
               c_rows_per_batch: int = 0, c_batch_stride: int = 0, ldc: int | None = None, ldg: int = 0) -> torch.Tensor:
    """out = epi(dequant(aq, ascale) @ dequant(wq, wscale).T), bf16 (``drag_gemm_mxfp8``): operands as ``quantize_mxfp8`` writes them
    (``wq`` [N, K], ``wscale`` [N, K / 32]; ``aq`` / ``ascale`` may be larger scratch buffers holding ``M`` dense rows), the epilogue
    arguments as ``gemm``'s."""
    for t, name in ((aq, "aq"), (ascale, "ascale"), (wq, "wq"), (wscale, "wscale")):
        _need(t, torch.uint8, "gemm_mxfp8." + name)
        if not t.is_contiguous():
            raise ValueError(f"gemm_mxfp8.{name} must be contiguous")
    if wq.dim() != 2 or wscale.dim() != 2:
        raise ValueError("gemm_mxfp8: wq [N, K] and wscale [N, K / 32] expected")
    N, K = wq.shape
    if K % 128 or tuple(wscale.shape) != (N, K // 32):
        raise ValueError(f"gemm_mxfp8: K = {K} must be a multiple of 128 and wscale [N, K / 32] (got {tuple(wscale.shape)})")
    if M is None:
        M = aq.numel() // K
    if aq.numel() < M * K or ascale.numel() < M * (K // 32):
        raise ValueError(f"gemm_mxfp8: aq / ascale hold fewer than M = {M} rows of K = {K}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=aq.device)
    _need(out, torch.bfloat16, "gemm_mxfp8.out")
    if ldc is None:
        ldc = out.stride(-2) if out.dim() >= 2 and out.stride(-1) == 1 else N
    for t, name in ((resid, "resid"), (bias, "bias"), (gate, "gate")):
        if t is not None:
            _need(t, torch.bfloat16, "gemm_mxfp8." + name)
    _linear_fit("gemm_mxfp8", M, N, N, out, resid, bias, gate, ldc, c_rows_per_batch, c_batch_stride, ldg)
    args = GemmMxArgs()
    args.Aq, args.Ascale, args.Wq, args.Wscale, args.C = aq.data_ptr(), ascale.data_ptr(), wq.data_ptr(), wscale.data_ptr(), out.data_ptr()
    args.bias = bias.data_ptr() if bias is not None else None
    args.gate = gate.data_ptr() if gate is not None else None
    args.resid = resid.data_ptr() if resid is not None else None
    args.M, args.N, args.K = M, N, K
    args.ldc, args.c_rows_per_batch, args.c_batch_stride = ldc, c_rows_per_batch, c_batch_stride
    args.ldg, args.act, args.act_n0 = ldg, act, act_n0
    _recorded(lambda: check(_lib.load().drag_gemm_mxfp8(ctypes.byref(args), _stream()), "drag_gemm_mxfp8"), (M, N, K), "mx")
    return out


def _attention_reach(kind: str, B: int, S: int, H: int, ld: int = 0, batch_stride: int = 0) -> int:
    """elements, counted from an operand's first one, that the head_dim-128 attention path addresses (one more than the largest offset; pure
    integers, tests/test_attention_room_host.py enumerates the addresses).  ``kind``: "rows" = q, k, row-major v or ``out`` (row s of batch b at
    b * batch_stride + s * ld, head h at + 128 h); "vt" = the V^T image; "prep" = the prep pass's qkv (batch b at b * S * ld, q | k | v side by
    side in a row); "rope" = one RoPE table (f32); "norm" = one RMSNorm weight; the dense MXFP8 images (bytes, s_pad = S rounded up to 128):
    "mx_rows" = q or k elements [B, H, s_pad, 128], "mx_row_scales" = their scales [B, H, s_pad, 4], "mx_vt" = V^T elements [B, H, 128, s_pad],
    "mx_vt_scales" = its scales [B, H, 128, s_pad / 32]"""
    if kind == "rows":
        return _rows_reach(B * S, H * 128, ld, S, batch_stride)
    if kind == "vt":
        return B * H * 128 * ((S + 63) // 64 * 64)
    if kind == "prep":
        return _rows_reach(B * S, 3 * H * 128, ld)
    if kind in ("mx_rows", "mx_row_scales", "mx_vt", "mx_vt_scales"):
        s_pad = (S + 127) // 128 * 128                     # the MXFP8 images' padding: S rounded up to a whole 128-key tile
        return B * H * {"mx_rows": s_pad * 128, "mx_row_scales": s_pad * 4, "mx_vt": 128 * s_pad, "mx_vt_scales": 128 * (s_pad // 32)}[kind]
    if kind == "rope":
        return S * 64
    if kind == "norm":
        return 128
    raise KeyError(kind)


_MX_IMAGE_KINDS = ("mx_rows", "mx_row_scales", "mx_rows", "mx_row_scales", "mx_vt", "mx_vt_scales")      # (qq, qs, kq, ks, vq, vs)


def _attention_room(what: str, B: int, S: int, H: int, rows=(), vt=None, prep=None, ropes=(), norms=(), mx=None) -> None:
    """the operands of one of the five head_dim-128 attention wrappers before the launch: every optional one a GPU tensor of its dtype, no
    negative stride, output rows that do not overlap, and the last element each operand's addressing reaches (``_attention_reach``) inside
    its storage — a wrong stride is an error here, not a memory fault in the kernel (shapes the library refuses — ld % 8, ld_o % 4, the
    2 GiB K span, B / S / H <= 0 — stay the library's to report).  ``rows``: (name, tensor, ld, batch_stride); ``prep``: (tensor, ld);
    ``ropes`` / ``norms``: (name, tensor or None); ``mx``: the six MXFP8 images (qq, qs, kq, ks, vq, vs), GPU uint8"""
    if mx is not None:
        if len(mx) != 6:
            raise ValueError(f"{what}.images: the six MXFP8 images (qq, qs, kq, ks, vq, vs) expected, got {len(mx)}")
        for name, t in zip(("qq", "qs", "kq", "ks", "vq", "vs"), mx):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
                raise ValueError(f"{what}.images.{name}: expected a GPU uint8 tensor, got {getattr(t, 'dtype', type(t))}")
    for group, dtype in ((ropes, torch.float32), (norms, torch.bfloat16)):
        for name, t in group:
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype):
                raise ValueError(f"{what}.{name}: expected a GPU {dtype} tensor, got {getattr(t, 'dtype', type(t))}"
                                 f"{'' if getattr(t, 'is_cuda', True) else ' on the host'}")
    if B <= 0 or S <= 0 or H <= 0:
        return
    for name, t, ld, bs in rows:
        if ld < 0 or bs < 0:
            raise ValueError(f"{what}.{name}: negative stride (row stride {ld}, batch stride {bs})")
        if name == "out" and ld < H * 128:
            raise ValueError(f"{what}.out: rows of stride {ld} overlap ({H} heads x 128 = {H * 128} elements each)")
        _fit(t, _attention_reach("rows", B, S, H, ld, bs), f"{what}.{name}", B * S, H * 128, ld, S, bs)
    if vt is not None:
        _fit(vt, _attention_reach("vt", B, S, H), what + ".vt (dense [B, H, 128, s_pad], s_pad = S rounded up to 64)")
    if prep is not None:
        t, ld = prep
        if ld < 0:
            raise ValueError(f"{what}.qkv: negative row stride {ld}")
        _fit(t, _attention_reach("prep", B, S, H, ld), what + ".qkv", B * S, 3 * H * 128, ld)
    for group, kind in ((ropes, "rope"), (norms, "norm")):
        for name, t in group:
            if t is not None:
                _fit(t, _attention_reach(kind, B, S, H), f"{what}.{name}")
    if mx is not None:
        for name, t, kind in zip(("qq", "qs", "kq", "ks", "vq", "vs"), mx, _MX_IMAGE_KINDS):
            _fit(t, _attention_reach(kind, B, S, H), f"{what}.images.{name} (a dense image, s_pad = S rounded up to 128)")


def qk_norm_rope_vt(qkv: torch.Tensor, vt: torch.Tensor, wq_txt, wk_txt, wq_img, wk_img, rope_cos, rope_sin,
                    B: int, S: int, H: int, ld: int, s_txt: int, eps: float = 1e-6) -> None:
    """The pass in front of ``attention`` (``drag_qk_norm_rope_vt_bf16``): per-head RMSNorm (weights ``w*_txt`` [128] for rows < ``s_txt``,
    ``w*_img`` after; all four or none) and RoPE (``rope_cos`` / ``rope_sin`` f32 [S, 64]; both or neither) of q and k IN PLACE, and V -> V^T.

    ``qkv`` is a view whose first element is q of token 0 of batch 0, 16-byte aligned: token s of batch b lies at (b * S + s) * ld, its q | k | v
    at + 0 | H*128 | 2*H*128 (``ld`` >= 3*H*128, a multiple of 8; the columns beyond belong to the caller and are not touched, nor is v).  The
    pass has NO batch-stride argument: batch b starts at b * S * ld from the view's start, whatever lies between the rows.

    ``vt`` is the dense [B, H, 128, s_pad] image, s_pad = S rounded up to a multiple of 64, every element of which is written: inside each
    group of 16 keys, position 16g + w of row d holds V[16g + 8*((w >> 2) & 1) + 4*(w >> 3) + (w & 3)][d] (the order in which a lane of the
    attention kernels holds its P registers), and positions whose key is >= S hold +0.0."""
    lib = _lib.load()
    _need(qkv, torch.bfloat16, "qkv")
    _need(vt, torch.bfloat16, "vt")
    _attention_room("qk_norm_rope_vt", B, S, H, vt=vt, prep=(qkv, ld), ropes=(("rope_cos", rope_cos), ("rope_sin", rope_sin)),
                    norms=(("wq_txt", wq_txt), ("wk_txt", wk_txt), ("wq_img", wq_img), ("wk_img", wk_img)))
    check(lib.drag_qk_norm_rope_vt_bf16(_p(qkv), _p(vt), _p(wq_txt), _p(wk_txt), _p(wq_img), _p(wk_img),
                                        _p(rope_cos), _p(rope_sin), B, S, H, ld, s_txt, eps, _stream()),
          "drag_qk_norm_rope_vt_bf16")


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int,
              ld_qk: int, qk_batch_stride: int, ld_o: int, o_batch_stride: int, scale: float) -> None:
    """head_dim-128 attention over prepared q and k and the V^T image of ``qk_norm_rope_vt`` (``drag_attention_bf16``).  The layout contract of
    the attention wrappers (``attention_qprep`` and ``attention_v`` share it):

    - ``q`` / ``k`` (and ``attention_v``'s row-major ``v``) are views whose first element is head 0 of token 0 of batch 0, each 16-byte aligned:
      token s of batch b at b * qk_batch_stride + s * ld_qk, head h at + 128 h; ``ld_qk`` >= H*128 and a multiple of 8; one (batch, head)'s k
      rows span less than 2 GiB.  The three share the row and batch stride; whatever lies between the rows is not read.
    - ``out`` [B, S, H*128]: token s of batch b at b * o_batch_stride + s * ld_o, 8-byte aligned, ``ld_o`` >= H*128 and a multiple of 4; only
      those B * S * H*128 elements are written.  The epilogue stores 16 bytes at a time when every output row is 16-byte aligned (``out``
      16-byte aligned, ``ld_o`` and ``o_batch_stride`` multiples of 8, and "attn_tune" bit 2 set, the default) and 8 bytes at a time otherwise:
      the same bits either way.
    - ``vt`` is the dense [B, H, 128, s_pad] image, s_pad = S rounded up to a multiple of 64, in the key order ``qk_norm_rope_vt`` documents.
    - RoPE tables are f32 [S, 64], norm weights bf16 [128].

    An operand whose addressing would leave its storage, a negative stride or overlapping output rows raise ValueError before anything is
    launched."""
    lib = _lib.load()
    _need(q, torch.bfloat16, "q")
    _need(k, torch.bfloat16, "k")
    _need(vt, torch.bfloat16, "vt")
    _need(out, torch.bfloat16, "out")
    _attention_room("attention", B, S, H, rows=(("q", q, ld_qk, qk_batch_stride), ("k", k, ld_qk, qk_batch_stride), ("out", out, ld_o, o_batch_stride)),
                    vt=vt)
    _recorded_attention(lambda: check(lib.drag_attention_bf16(_p(q), _p(k), _p(vt), _p(out), B, S, H, ld_qk, qk_batch_stride, ld_o,
                                                              o_batch_stride, scale, _stream()), "drag_attention_bf16"), B, S, H, False, False)


def k_norm_rope_vt(qkv: torch.Tensor, vt: torch.Tensor, wk_txt, wk_img, rope_cos, rope_sin, B: int, S: int, H: int, ld: int,
                   s_txt: int, eps: float = 1e-6) -> None:
    """k RMSNorm + RoPE in place and V -> V^T; q is left as projected (``attention_qprep`` prepares it on load).  ``qkv``'s layout (batch b at
    b * S * ld from the view's start: the pass has no other batch stride), ``vt``'s size and its key order are ``qk_norm_rope_vt``'s; with
    ``vt`` None only k is prepared and v is not read."""
    lib = _lib.load()
    _need(qkv, torch.bfloat16, "qkv")
    if vt is not None:              # None: k only (``attention_v`` reads v row-major)
        _need(vt, torch.bfloat16, "vt")
    _attention_room("k_norm_rope_vt", B, S, H, vt=vt, prep=(qkv, ld), ropes=(("rope_cos", rope_cos), ("rope_sin", rope_sin)),
                    norms=(("wk_txt", wk_txt), ("wk_img", wk_img)))
    check(lib.drag_k_norm_rope_vt_bf16(_p(qkv), _p(vt), _p(wk_txt), _p(wk_img), _p(rope_cos), _p(rope_sin), B, S, H, ld, s_txt,
                                       eps, _stream()), "drag_k_norm_rope_vt_bf16")


def attention_qprep(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int, ld_qk: int,
                    qk_batch_stride: int, ld_o: int, o_batch_stride: int, scale: float, wq_txt, wq_img, rope_cos, rope_sin,
                    s_txt: int, eps: float = 1e-6) -> None:
    """attention over the RAW q projection: norm_q + RoPE are applied to each query row as its fragments are loaded (weights ``wq_txt`` for
    rows < ``s_txt``, ``wq_img`` after).  Layout contract: ``attention``'s."""
    lib = _lib.load()
    _need(q, torch.bfloat16, "q")
    _need(k, torch.bfloat16, "k")
    _need(vt, torch.bfloat16, "vt")
    _need(out, torch.bfloat16, "out")
    _attention_room("attention_qprep", B, S, H,
                    rows=(("q", q, ld_qk, qk_batch_stride), ("k", k, ld_qk, qk_batch_stride), ("out", out, ld_o, o_batch_stride)), vt=vt,
                    ropes=(("rope_cos", rope_cos), ("rope_sin", rope_sin)), norms=(("wq_txt", wq_txt), ("wq_img", wq_img)))
    _recorded_attention(lambda: check(lib.drag_attention_qprep_bf16(_p(q), _p(k), _p(vt), _p(out), B, S, H, ld_qk, qk_batch_stride, ld_o,
                                                                    o_batch_stride, scale, _p(wq_txt), _p(wq_img), _p(rope_cos), _p(rope_sin),
                                                                    s_txt, eps, _stream()), "drag_attention_qprep_bf16"), B, S, H, True, False)


def attention_v(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int, ld_qk: int,
                qk_batch_stride: int, ld_o: int, o_batch_stride: int, scale: float, wq_txt=None, wq_img=None, rope_cos=None,
                rope_sin=None, s_txt: int = 0, eps: float = 1e-6) -> None:
    """attention over q | k | v as the Linears wrote them: v is read row-major (no V^T pass / buffer); the q preparation
    (norm weights + RoPE tables) is optional: all four or none.  Layout contract: ``attention``'s, ``v`` sharing q's and k's row stride and
    batch stride (and their 16-byte alignment)."""
    lib = _lib.load()
    _need(q, torch.bfloat16, "q")
    _need(k, torch.bfloat16, "k")
    _need(v, torch.bfloat16, "v")
    _need(out, torch.bfloat16, "out")
    _attention_room("attention_v", B, S, H, rows=(("q", q, ld_qk, qk_batch_stride), ("k", k, ld_qk, qk_batch_stride),
                                                  ("v", v, ld_qk, qk_batch_stride), ("out", out, ld_o, o_batch_stride)),
                    ropes=(("rope_cos", rope_cos), ("rope_sin", rope_sin)), norms=(("wq_txt", wq_txt), ("wq_img", wq_img)))
    _recorded_attention(lambda: check(lib.drag_attention_v_bf16(_p(q), _p(k), _p(v), _p(out), B, S, H, ld_qk, qk_batch_stride, ld_o, o_batch_stride,
                                                                scale, _p(wq_txt), _p(wq_img), _p(rope_cos), _p(rope_sin), s_txt, eps, _stream()),
                                      "drag_attention_v_bf16"), B, S, H, wq_txt is not None, True)


def attention_mxfp8_supported(B: int, S: int, H: int) -> bool:
    """does the MXFP8 attention path take this shape (``drag_attention_mxfp8_supported``: B, H in 1 .. 65535, S in 1 .. 2^23)?  A pure query:
    callers that fall back to the bf16 launches (FluxTransformerHIP) ask before they launch."""
    return bool(_lib.load().drag_attention_mxfp8_supported(B, S, H))


def attention_mxfp8_images(B: int, S: int, H: int, device) -> tuple:
    """uninitialised buffers for the six MXFP8 attention images (qq, qs, kq, ks, vq, vs) of ``qkv_prep_mxfp8`` / ``attention_mxfp8``:
    uint8 [B, H, s_pad, 128], [B, H, s_pad, 4], the same two for k, [B, H, 128, s_pad], [B, H, 128, s_pad / 32]; s_pad = S rounded up to 128"""
    sp = (S + 127) // 128 * 128
    shapes = ((sp, 128), (sp, 4), (sp, 128), (sp, 4), (128, sp), (128, sp // 32))
    return tuple(torch.empty((B, H) + shp, dtype=torch.uint8, device=device) for shp in shapes)


def qkv_prep_mxfp8(qkv: torch.Tensor, images, wq_txt, wk_txt, wq_img, wk_img, rope_cos, rope_sin, B: int, S: int, H: int, ld: int,
                   s_txt: int, eps: float = 1e-6) -> None:
    """The pass in front of ``attention_mxfp8`` (``drag_qkv_prep_mxfp8``): reads ``qkv`` under ``qk_norm_rope_vt``'s layout contract and leaves it
    UNTOUCHED; writes every byte of the six dense images ``images`` = (qq, qs, kq, ks, vq, vs) (``attention_mxfp8_images``; format:
    :mod:`.mx`): q and k are the values ``qk_norm_rope_vt`` would store, quantised along head_dim; V^T is quantised along the keys in natural
    key order, keys >= S as zeros; q / k rows >= S are zero bytes under scale byte 127."""
    lib = _lib.load()
    _need(qkv, torch.bfloat16, "qkv")
    _attention_room("qkv_prep_mxfp8", B, S, H, prep=(qkv, ld), ropes=(("rope_cos", rope_cos), ("rope_sin", rope_sin)),
                    norms=(("wq_txt", wq_txt), ("wk_txt", wk_txt), ("wq_img", wq_img), ("wk_img", wk_img)), mx=images)
    check(lib.drag_qkv_prep_mxfp8(_p(qkv), _p(wq_txt), _p(wk_txt), _p(wq_img), _p(wk_img), _p(rope_cos), _p(rope_sin), B, S, H, ld, s_txt, eps,
                                  *[_p(t) for t in images], _stream()), "drag_qkv_prep_mxfp8")


def attention_mxfp8(images, out: torch.Tensor, B: int, S: int, H: int, ld_o: int, o_batch_stride: int, scale: float) -> None:
    """head_dim-128 attention over the MXFP8 images of ``qkv_prep_mxfp8`` (``drag_attention_mxfp8``; e4m3 operands on the block-scaled matrix
    instruction for both products, float32 softmax).  ``out`` under ``attention``'s contract (token s of batch b at b * o_batch_stride +
    s * ld_o, 8-byte aligned, ``ld_o`` >= H*128 and a multiple of 4; only the B * S * H*128 owned elements are written).  Short images, a
    negative stride or overlapping output rows raise ValueError before anything is launched; a shape the kernel does not take
    (``attention_mxfp8_supported``) or a non-positive ``scale`` is the library's error."""
    lib = _lib.load()
    _need(out, torch.bfloat16, "out")
    _attention_room("attention_mxfp8", B, S, H, rows=(("out", out, ld_o, o_batch_stride),), mx=images)
    _recorded_attention(lambda: check(lib.drag_attention_mxfp8(*[_p(t) for t in images], _p(out), B, S, H, ld_o, o_batch_stride, scale, _stream()),
                                      "drag_attention_mxfp8"), B, S, H, False, False, mx=True)


def layernorm(x: torch.Tensor, y: torch.Tensor, M: int, D: int, *, scale=None, shift=None, gamma=None, beta=None,
              ldx: int | None = None, rows_per_batch: int = 0, x_batch_stride: int = 0, ldy: int | None = None,
              ld_mod: int = 0, eps: float = 1e-6) -> torch.Tensor:
    """``y`` [M, D] rows of ``ldy`` = LayerNorm of M rows of ``x`` (``drag_layernorm_modulate_bf16``): row r is row r % rows_per_batch of batch
    b = r // rows_per_batch (0 = one batch of M rows), at b * x_batch_stride + (r % rows_per_batch) * ldx.  With ``scale`` / ``shift`` (batch b's D
    values at b * ld_mod) the AdaLN modulation, with ``gamma`` / ``beta`` [D] the affine form, with neither the bare normalisation."""
    lib = _lib.load()
    _need(x, torch.bfloat16, "x")
    _need(y, torch.bfloat16, "y")
    ldx = D if ldx is None else ldx
    ldy = D if ldy is None else ldy
    _layernorm_room(x, y, {"scale": scale, "shift": shift}, {"gamma": gamma, "beta": beta}, M, D, ldx, rows_per_batch, x_batch_stride, ldy,
                    ld_mod)
    check(lib.drag_layernorm_modulate_bf16(_p(x), _p(y), _p(scale), _p(shift), _p(gamma), _p(beta), M, D, ldx, rows_per_batch,
                                           x_batch_stride, ldy, ld_mod, eps, _stream()),
          "drag_layernorm_modulate_bf16")
    return y


def _layernorm_room(x: torch.Tensor, y: torch.Tensor, mods: dict, vecs: dict, M: int, D: int, ldx: int, rows_per_batch: int,
                    x_batch_stride: int, ldy: int, ld_mod: int) -> None:
    """``layernorm``'s operands before the launch: every optional one a GPU bf16 tensor, and the last element that the row addressing
    reaches inside each operand's storage — a wrong stride is an error here, not a memory fault in the kernel (the shapes that the library
    refuses, a bad D or a stride that is no multiple of 8, stay the library's to report)"""
    for name, t in (*mods.items(), *vecs.items()):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16):
            raise ValueError(f"layernorm.{name}: expected a GPU bfloat16 tensor, got {getattr(t, 'dtype', type(t))}")
    if M <= 0 or D <= 0:
        return
    for name, v in (("ldx", ldx), ("ldy", ldy), ("ld_mod", ld_mod), ("x_batch_stride", x_batch_stride)):
        if v < 0:
            raise ValueError(f"layernorm.{name}: {v} is negative")
    _fit(x, _rows_reach(M, D, ldx, rows_per_batch, x_batch_stride), "layernorm.x", M, D, ldx, rows_per_batch, x_batch_stride)
    _fit(y, _rows_reach(M, D, ldy), "layernorm.y", M, D, ldy)
    nb = _batches(M, rows_per_batch)
    for name, t in mods.items():
        if t is not None:
            _fit(t, _rows_reach(nb, D, ld_mod), "layernorm." + name, nb, D, ld_mod)
    for name, t in vecs.items():
        if t is not None:
            _fit(t, D, "layernorm." + name)


def _stepcache_room(x: torch.Tensor, dense: dict, B: int, rows_per_batch: int, cols: int, x_batch_stride: int, what: str) -> None:
    """the last element each operand's addressing reaches must lie inside its storage: a wrong stride is an error here, not a memory fault
    in the kernel (shapes the library refuses are the library's to report)"""
    if B <= 0 or rows_per_batch <= 0 or cols <= 0 or x_batch_stride < rows_per_batch * cols:
        return
    n = rows_per_batch * cols
    _fit(x, _rows_reach(B * rows_per_batch, cols, cols, rows_per_batch, x_batch_stride), what + ".x", B * rows_per_batch, cols, cols, rows_per_batch,
         x_batch_stride)
    for name, t in dense.items():
        if t is not None and (not t.is_contiguous() or t.numel() < B * n):
            raise ValueError(f"{what}.{name}: expected a contiguous tensor of at least {B * n} elements")


def stepcache_workspace_bytes(B: int, rows_per_batch: int, cols: int) -> int:
    """bytes of the partial-sum workspace ``stepcache_delta`` needs for this shape (``drag_stepcache_workspace_bytes``); launches nothing"""
    return int(_lib.load().drag_stepcache_workspace_bytes(B, rows_per_batch, cols))


def stepcache_delta(x: torch.Tensor, e: torch.Tensor, f: torch.Tensor | None, ratios: torch.Tensor | None, workspace: torch.Tensor | None,
                    B: int, rows_per_batch: int, cols: int, x_batch_stride: int) -> None:
    """in place ``e <- bf16(f32(x) - f32(e))``; with ``f`` also ``ratios[b] = sum |e - f| / sum |f|`` per image in float64
    (``drag_stepcache_delta_bf16``).  ``x`` addresses image rows as ``layernorm`` does (``rows_per_batch`` rows of ``cols`` elements from
    ``x`` on, ``x_batch_stride`` between images); ``e`` / ``f`` are dense [B, rows_per_batch, cols]; ``ratios`` float64 [B]; ``workspace``
    uint8, ``stepcache_workspace_bytes`` long.  With ``f`` None no ratio is written."""
    lib = _lib.load()
    _need(x, torch.bfloat16, "stepcache_delta.x")
    _need(e, torch.bfloat16, "stepcache_delta.e")
    if f is not None:
        _need(f, torch.bfloat16, "stepcache_delta.f")
        if ratios is None or workspace is None:
            raise ValueError("stepcache_delta: f given, so ratios and workspace are required")
        _need(ratios, torch.float64, "stepcache_delta.ratios")
        _need(workspace, torch.uint8, "stepcache_delta.workspace")
        if ratios.numel() < B or not ratios.is_contiguous():
            raise ValueError(f"stepcache_delta.ratios: expected a contiguous float64 tensor of at least {B} elements")
        if workspace.numel() < stepcache_workspace_bytes(B, rows_per_batch, cols):
            raise ValueError(f"stepcache_delta.workspace: {workspace.numel()} bytes, {stepcache_workspace_bytes(B, rows_per_batch, cols)} needed")
    _stepcache_room(x, dict(e=e, f=f), B, rows_per_batch, cols, x_batch_stride, "stepcache_delta")
    check(lib.drag_stepcache_delta_bf16(_p(x), _p(e), _p(f), _p(ratios) if f is not None else None, _p(workspace) if f is not None else None,
                                        B, rows_per_batch, cols, x_batch_stride, _stream()), "drag_stepcache_delta_bf16")


def stepcache_apply(x: torch.Tensor, r: torch.Tensor, B: int, rows_per_batch: int, cols: int, x_batch_stride: int, sign: int) -> None:
    """``sign`` = +1: ``x <- bf16(f32(x) + f32(r))``; -1, the capture form: ``r <- bf16(f32(x) - f32(r))`` (``drag_stepcache_apply_bf16``).
    ``x`` addressed as in ``stepcache_delta``, ``r`` dense [B, rows_per_batch, cols]."""
    lib = _lib.load()
    _need(x, torch.bfloat16, "stepcache_apply.x")
    _need(r, torch.bfloat16, "stepcache_apply.r")
    _stepcache_room(x, dict(r=r), B, rows_per_batch, cols, x_batch_stride, "stepcache_apply")
    check(lib.drag_stepcache_apply_bf16(_p(x), _p(r), B, rows_per_batch, cols, x_batch_stride, sign, _stream()), "drag_stepcache_apply_bf16")


def _index_list(values) -> tuple:
    """a host list of image indices as the C array the list forms take (the library validates range, order and length), and its length"""
    v = [int(i) for i in values]
    return (ctypes.c_int32 * max(1, len(v)))(*v), len(v)


def stepcache_swap(x: torch.Tensor, B: int, rows_per_batch: int, cols: int, x_batch_stride: int, pairs) -> None:
    """exchange in place the ``rows_per_batch`` x ``cols`` elements of image ``a`` with those of image ``b`` for every ``(a, b)`` of
    ``pairs`` (host integers, disjoint, at most 32 pairs), one launch (``drag_stepcache_swap_bf16``); ``x`` addressed as in
    ``stepcache_delta``.  No pairs: nothing is launched."""
    lib = _lib.load()
    _need(x, torch.bfloat16, "stepcache_swap.x")
    flat = []
    for pair in pairs:
        a, b = pair
        flat += [a, b]
    arr, n = _index_list(flat)
    _stepcache_room(x, {}, B, rows_per_batch, cols, x_batch_stride, "stepcache_swap")
    check(lib.drag_stepcache_swap_bf16(_p(x), B, rows_per_batch, cols, x_batch_stride, arr, n // 2, _stream()), "drag_stepcache_swap_bf16")


def stepcache_apply_images(x: torch.Tensor, r: torch.Tensor, B: int, rows_per_batch: int, cols: int, x_batch_stride: int, sign: int,
                           images) -> None:
    """``stepcache_apply`` on the images listed in ``images`` only (host integers, strictly increasing, at most 64): the same arithmetic
    per element, ``r`` indexed by image (``drag_stepcache_apply_images_bf16``).  An empty list launches nothing."""
    lib = _lib.load()
    _need(x, torch.bfloat16, "stepcache_apply_images.x")
    _need(r, torch.bfloat16, "stepcache_apply_images.r")
    arr, n = _index_list(images)
    _stepcache_room(x, dict(r=r), B, rows_per_batch, cols, x_batch_stride, "stepcache_apply_images")
    check(lib.drag_stepcache_apply_images_bf16(_p(x), _p(r), B, rows_per_batch, cols, x_batch_stride, sign, arr, n, _stream()),
          "drag_stepcache_apply_images_bf16")


def stepcache_copy_images(dst: torch.Tensor, src: torch.Tensor, src_batch_stride: int, B: int, rows_per_batch: int, cols: int,
                          images) -> None:
    """``dst[b] <- src[b]`` for the images listed in ``images`` (as in ``stepcache_apply_images``): ``dst`` dense [B, rows_per_batch, cols],
    image ``b`` of ``src`` at ``src + b * src_batch_stride`` (``drag_stepcache_copy_images_bf16``)."""
    lib = _lib.load()
    _need(dst, torch.bfloat16, "stepcache_copy_images.dst")
    _need(src, torch.bfloat16, "stepcache_copy_images.src")
    arr, n = _index_list(images)
    _stepcache_room(src, dict(dst=dst), B, rows_per_batch, cols, src_batch_stride, "stepcache_copy_images")
    check(lib.drag_stepcache_copy_images_bf16(_p(dst), _p(src), src_batch_stride, B, rows_per_batch, cols, arr, n, _stream()),
          "drag_stepcache_copy_images_bf16")


def stepcache_forecast_images(x: torch.Tensor, r: torch.Tensor, p: torch.Tensor, B: int, rows_per_batch: int, cols: int, x_batch_stride: int,
                              images, coefs) -> None:
    """the first-order forecast of a reused step on the images listed in ``images`` (as in ``stepcache_apply_images``), image ``images[i]``
    with the coefficient ``coefs[i]`` (host floats, passed as float32, all finite): per element ``d = f32(r) - f32(p); m = c * d;
    f = m + f32(r); x <- bf16(f32(x) + f)``, four individually rounded float32 operations, no FMA
    (``drag_stepcache_forecast_images_bf16``).  ``r`` and ``p`` are dense [B, rows_per_batch, cols], indexed by image, and stay as they
    are.  An empty list launches nothing."""
    lib = _lib.load()
    _need(x, torch.bfloat16, "stepcache_forecast_images.x")
    _need(r, torch.bfloat16, "stepcache_forecast_images.r")
    _need(p, torch.bfloat16, "stepcache_forecast_images.p")
    arr, n = _index_list(images)
    c = [float(v) for v in coefs]
    if len(c) != n:
        raise ValueError(f"stepcache_forecast_images: {n} images but {len(c)} coefficients")
    _stepcache_room(x, dict(r=r, p=p), B, rows_per_batch, cols, x_batch_stride, "stepcache_forecast_images")
    check(lib.drag_stepcache_forecast_images_bf16(_p(x), _p(r), _p(p), B, rows_per_batch, cols, x_batch_stride, arr,
                                                  (ctypes.c_float * max(1, n))(*c), n, _stream()), "drag_stepcache_forecast_images_bf16")


def _dense_operand(t: torch.Tensor, n: int, name: str, exact: bool = False) -> None:
    """a further operand of an elementwise kernel that walks ``n`` dense bf16 elements: a GPU bf16 tensor whose own ``n`` elements (at
    least ``n``, or with ``exact`` just ``n``) lie dense in its storage — anything else is an error here, not a memory fault in the kernel"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16):
        raise ValueError(f"{name}: expected a GPU bfloat16 tensor, got {getattr(t, 'dtype', type(t))}")
    if not t.is_contiguous() or t.numel() < n or (exact and t.numel() != n):
        raise ValueError(f"{name}: expected a contiguous tensor of {'' if exact else 'at least '}{n} elements, got shape {tuple(t.shape)}, "
                         f"strides {t.stride()}")


def _dense_first(x: torch.Tensor, name: str) -> None:
    """the first operand sets the element count: its numel() elements must exist from its start on (an expanded view has fewer)"""
    if x.numel() > _room(x):
        raise ValueError(f"{name}: {x.numel()} elements, but only {_room(x)} from its start in its storage (an expanded view?)")


def act(x: torch.Tensor, kind: int, out: torch.Tensor | None = None) -> torch.Tensor:
    lib = _lib.load()
    _need(x, torch.bfloat16, "x")
    _dense_first(x, "act.x")
    if out is None:
        out = torch.empty_like(x)
    _dense_operand(out, x.numel(), "act.out", exact=True)
    if x.numel() == 0:                                      # an empty tensor has no address to hand the library
        return out
    check(lib.drag_act_bf16(_p(x), _p(out), x.numel(), kind, _stream()), "drag_act_bf16")
    return out


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    lib = _lib.load()
    _need(t, torch.float32, "t")
    out = torch.empty((t.numel(), dim), dtype=torch.bfloat16, device=t.device)
    check(lib.drag_timestep_embedding_bf16(_p(t), _p(out), t.numel(), dim, _stream()), "drag_timestep_embedding_bf16")
    return out


def flow_euler_step(x: torch.Tensor, v: torch.Tensor, dt: float) -> None:
    lib = _lib.load()
    _need(x, torch.bfloat16, "x")
    _dense_first(x, "flow_euler_step.x")
    _dense_operand(v, x.numel(), "flow_euler_step.v")
    if x.numel() == 0:
        return
    check(lib.drag_flow_euler_step_bf16(_p(x), _p(v), dt, x.numel(), _stream()), "drag_flow_euler_step_bf16")


def add(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    lib = _lib.load()
    _need(a, torch.bfloat16, "a")
    _dense_first(a, "add.a")
    _dense_operand(b, a.numel(), "add.b")
    if out is None:
        out = torch.empty_like(a)
    _dense_operand(out, a.numel(), "add.out", exact=True)
    if a.numel() == 0:
        return out
    check(lib.drag_add_bf16(_p(a), _p(b), _p(out), a.numel(), _stream()), "drag_add_bf16")
    return out


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if x.numel() == 0:
        return out
    check(lib.drag_cast_f32_to_bf16(_p(x), _p(out), x.numel(), _stream()), "drag_cast_f32_to_bf16")
    return out


def to_f32(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(x, torch.bfloat16, "x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel() == 0:
        return out
    check(lib.drag_cast_bf16_to_f32(_p(x), _p(out), x.numel(), _stream()), "drag_cast_bf16_to_f32")
    return out


def _need_rows(t: torch.Tensor, name: str):
    """the kernels take a base pointer + (rows, d): a sliced / transposed view would be scanned with the wrong stride"""
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous [rows, d] matrix (got shape {tuple(t.shape)}, strides {t.stride()}); "
                         "call .contiguous() on views")


def cosine_topk(corpus: torch.Tensor, queries: torch.Tensor, k: int):
    """(D, I) = exact inner-product top-k; D f32 [Q, k] descending, I int64 [Q, k]."""
    lib = _lib.load()
    _need(corpus, torch.float32, "corpus")
    _need(queries, torch.float32, "queries")
    _need_rows(corpus, "corpus"); _need_rows(queries, "queries")
    N, d = corpus.shape
    Q = queries.shape[0]
    if queries.shape[1] != d:
        raise ValueError(f"queries have d = {queries.shape[1]}, corpus has d = {d}")
    ws_bytes = lib.drag_cosine_topk_workspace_bytes(N, Q)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=corpus.device)
    D = torch.empty((Q, k), dtype=torch.float32, device=corpus.device)
    I = torch.empty((Q, k), dtype=torch.int64, device=corpus.device)
    check(lib.drag_cosine_topk_f32(_p(corpus), _p(queries), N, d, Q, k, _p(D), _p(I), _p(ws), _stream()),
          "drag_cosine_topk_f32")
    return D, I


def cosine_scores(corpus: torch.Tensor, queries: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """scan pass alone (ONE pass over the corpus): f32 [Q <= 64, ceil64(N)] inner products in the pinned summation order (entries >= N unspecified)"""
    lib = _lib.load()
    _need(corpus, torch.float32, "corpus")
    _need(queries, torch.float32, "queries")
    _need_rows(corpus, "corpus"); _need_rows(queries, "queries")
    N, d = corpus.shape
    Q = queries.shape[0]
    npad = (N + 63) // 64 * 64
    if out is None:
        out = torch.empty((Q, npad), dtype=torch.float32, device=corpus.device)
    check(lib.drag_cosine_scores_f32(_p(corpus), _p(queries), N, d, Q, _p(out), _stream()), "drag_cosine_scores_f32")
    return out


def l2_normalize_(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _need(x, torch.float32, "x")
    _need_rows(x, "x")
    check(lib.drag_l2_normalize_f32(_p(x), x.shape[0], x.shape[1], _stream()), "drag_l2_normalize_f32")
    return x


# ------------------------------------------------------------------ VAE-side ops
def conv3x3(x_pad: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, B: int, Ho: int, Wo: int, Hp: int, Wp: int,
            Cin: int, Cout: int, bias=None, resid=None, ldy: int | None = None, stride: int = 1, oy: int = 0, ox: int = 0,
            act: int = ACT_NONE) -> torch.Tensor:
    """3x3 conv over a zero-haloed NHWC input as an implicit GEMM (w is [Cout, 3, 3, Cin])."""
    lib = _lib.load()
    _need(x_pad, torch.bfloat16, "conv.x")
    _need(w, torch.bfloat16, "conv.w")
    a = _lib.ConvArgs()
    a.x, a.w, a.y = x_pad.data_ptr(), w.data_ptr(), y.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.resid = resid.data_ptr() if resid is not None else None
    a.B, a.Ho, a.Wo, a.Hp, a.Wp, a.Cin, a.Cout = B, Ho, Wo, Hp, Wp, Cin, Cout
    a.ldy, a.stride, a.oy, a.ox, a.act = ldy if ldy is not None else Cout, stride, oy, ox, act
    _recorded(lambda: check(lib.drag_conv3x3_bf16(ctypes.byref(a), _stream()), "drag_conv3x3_bf16"), (B * Ho * Wo, Cout, 9 * Cin), True)
    return y


_gn_ws: dict = {}


def groupnorm_silu(x, y, gamma, beta, B, H, W, C, *, out_pad: int, silu: bool, eps: float = 1e-6):
    lib = _lib.load()
    _need(x, torch.bfloat16, "gn.x")
    nbytes = lib.drag_groupnorm_workspace_bytes(B, H, W, C)
    key = (x.device, nbytes)
    ws = _gn_ws.get(key)
    if ws is None:
        ws = _gn_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(lib.drag_groupnorm_silu_bf16(_p(x), _p(y), _p(gamma), _p(beta), B, H, W, C, 32, out_pad, int(silu), eps,
                                       _p(ws), _stream()), "drag_groupnorm_silu_bf16")
    return y


def pad_copy(x, y, B, H, W, C, upsample: int = 1):
    lib = _lib.load()
    check(lib.drag_pad_copy_bf16(_p(x), _p(y), B, H, W, C, upsample, _stream()), "drag_pad_copy_bf16")
    return y


def softmax_rows(x: torch.Tensor, y: torch.Tensor, rows: int, cols: int, scale: float, ldy: int | None = None):
    lib = _lib.load()
    _need(x, torch.float32, "softmax.x")
    check(lib.drag_softmax_rows_f32_bf16(_p(x), _p(y), rows, cols, ldy if ldy is not None else cols, scale, _stream()),
          "drag_softmax_rows_f32_bf16")
    return y


def unpack_latents(tokens, y, B, h, w, ld, C, scaling, shift):
    lib = _lib.load()
    check(lib.drag_unpack_latents_bf16(_p(tokens), _p(y), B, h, w, ld, C, scaling, shift, _stream()), "drag_unpack_latents_bf16")
    return y


def sample_pack_latents(moments, noise, tokens, B, H, W, ldm, ld, scaling, shift):
    lib = _lib.load()
    check(lib.drag_sample_pack_latents_bf16(_p(moments), _p(noise), _p(tokens), B, H, W, ldm, ld, scaling, shift, _stream()),
          "drag_sample_pack_latents_bf16")
    return tokens


def image_preprocess(img_u8, mask_u8, y, B, H, W, C):
    lib = _lib.load()
    _need(img_u8, torch.uint8, "img")
    check(lib.drag_image_preprocess_u8(_p(img_u8), _p(mask_u8), _p(y), B, H, W, C, _stream()), "drag_image_preprocess_u8")
    return y


def image_postprocess(x, out_u8, npix, ld):
    lib = _lib.load()
    check(lib.drag_image_postprocess_u8(_p(x), _p(out_u8), npix, ld, _stream()), "drag_image_postprocess_u8")
    return out_u8


def mask_pack(mask_u8, tokens, B, H, W, ld):
    lib = _lib.load()
    _need(mask_u8, torch.uint8, "mask")
    check(lib.drag_mask_pack_u8(_p(mask_u8), _p(tokens), B, H, W, ld, _stream()), "drag_mask_pack_u8")
    return tokens


def flow_euler_rows(x, v, rows, cols, ldx, ldv, dt):
    lib = _lib.load()
    check(lib.drag_flow_euler_rows_bf16(_p(x), _p(v), rows, cols, ldx, ldv, dt, _stream()), "drag_flow_euler_rows_bf16")


def scale_noise_rows(x, noise, rows, cols, ldx, ldn, sigma):
    lib = _lib.load()
    check(lib.drag_scale_noise_rows_bf16(_p(x), _p(noise), rows, cols, ldx, ldn, sigma, _stream()), "drag_scale_noise_rows_bf16")


# ------------------------------------------------------------------ ViT front ends / Redux combine
def patchify(img_u8: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int, P: int, ldo: int, mean, std):
    lib = _lib.load()
    _need(img_u8, torch.uint8, "img")
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    check(lib.drag_patchify_u8(_p(img_u8), _p(out), B, H, W, P, ldo, m, s, _stream()), "drag_patchify_u8")
    return out


def scale_sum(x: torch.Tensor, scales: torch.Tensor, out: torch.Tensor, G: int, N: int, elems: int):
    lib = _lib.load()
    _need(x, torch.bfloat16, "x")
    _need(scales, torch.float32, "scales")
    check(lib.drag_scale_sum_bf16(_p(x), _p(scales), _p(out), G, N, elems, _stream()), "drag_scale_sum_bf16")
    return out


def resnet_stem_style(img_f32: torch.Tensor, conv_w, bn_scale, bn_shift, eps: float = 1e-5) -> torch.Tensor:
    """img fp32 [B,3,H,W] in [0,1] -> fp32 [B,128] (channel mean | std) of the ResNet50 stem output"""
    lib = _lib.load()
    _need(img_f32, torch.float32, "img")
    B, _, H, W = img_f32.shape
    out = torch.empty((B, 128), dtype=torch.float32, device=img_f32.device)
    ws = torch.empty(lib.drag_resnet_stem_style_workspace_bytes(B, H, W), dtype=torch.uint8, device=img_f32.device)
    check(lib.drag_resnet_stem_style_f32(_p(img_f32), _p(conv_w), _p(bn_scale), _p(bn_shift), _p(out), B, H, W, eps,
                                         _p(ws), _stream()), "drag_resnet_stem_style_f32")
    return out


def patchify_f32(img: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int, P: int, ldo: int):
    lib = _lib.load()
    _need(img, torch.float32, "img")
    check(lib.drag_patchify_f32_nchw(_p(img), _p(out), B, H, W, P, ldo, _stream()), "drag_patchify_f32_nchw")
    return out


# ---- LaMa stage (float32, NHWC) ------------------------------------------------------------------------------
PAD_ZERO, PAD_REFLECT = 0, 1
CONV_ACT_NONE, CONV_ACT_RELU, CONV_ACT_SIGMOID, CONV_ACT_QUICK_GELU = 0, 1, 2, 3


def conv2d_f32(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, B: int, Hi: int, Wi: int, Ho: int, Wo: int, Cin: int, ldx: int,
               ldy: int, stride: int = 1, pad: int = 0, pad_mode: int = PAD_ZERO, transposed: bool = False, act: int = CONV_ACT_NONE,
               scale=None, shift=None, addend=None, ld_add: int = 0, resid=None, ld_res: int = 0) -> torch.Tensor:
    """y = act((conv(x, w) + addend) * scale + shift) + resid on NHWC f32 views: ``x`` / ``y`` / ``addend`` / ``resid`` may be
    channel slices of wider buffers (1-D or offset views; ld* = floats per pixel).  ``w`` is [Cout, KH, KW, Cin]."""
    lib = _lib.load()
    for t, n in ((x, "x"), (w, "w"), (y, "y")):
        _need(t, torch.float32, "conv2d_f32." + n)
    Cout, KH, KW, wc = w.shape
    if wc != Cin or not w.is_contiguous():
        raise ValueError("conv2d_f32.w must be contiguous [Cout, KH, KW, Cin]")
    a = _lib.Conv2dF32Args()
    a.x, a.w, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    a.scale = scale.data_ptr() if scale is not None else None
    a.shift = shift.data_ptr() if shift is not None else None
    a.addend = addend.data_ptr() if addend is not None else None
    a.resid = resid.data_ptr() if resid is not None else None
    a.B, a.Hi, a.Wi, a.Cin, a.ldx, a.Ho, a.Wo, a.Cout, a.ldy, a.ld_add, a.ld_res = B, Hi, Wi, Cin, ldx, Ho, Wo, Cout, ldy, ld_add, ld_res
    a.KH, a.KW, a.stride, a.pad, a.pad_mode, a.transposed, a.act = KH, KW, stride, pad, pad_mode, int(transposed), act
    _recorded(lambda: check(lib.drag_conv2d_f32(ctypes.byref(a), _stream()), "drag_conv2d_f32"), (B * Ho * Wo, Cout, KH * KW * Cin), "f32")
    return y


def rfft2_f32(x, tmp, y, B, H, W, C, ldx, tw_w, tw_h):
    check(_lib.load().drag_rfft2_f32(_p(x), _p(tmp), _p(y), B, H, W, C, ldx, _p(tw_w), _p(tw_h), _stream()), "drag_rfft2_f32")


def irfft2_f32(f, tmp, y, add, B, H, W, C, ldy, ld_add, tw_w, tw_h):
    check(_lib.load().drag_irfft2_f32(_p(f), _p(tmp), _p(y), _p(add), B, H, W, C, ldy, ld_add, _p(tw_w), _p(tw_h), _stream()),
          "drag_irfft2_f32")


def lama_prepare(img_u8, mask_u8, x, H, W, Hp, Wp):
    _need(img_u8, torch.uint8, "lama_prepare.img"); _need(mask_u8, torch.uint8, "lama_prepare.mask")
    check(_lib.load().drag_lama_prepare_u8(_p(img_u8), _p(mask_u8), _p(x), H, W, Hp, Wp, _stream()), "drag_lama_prepare_u8")


def lama_blend(pred, ld, img_u8, mask_u8, out_u8, H, W, Hp, Wp):
    check(_lib.load().drag_lama_blend_u8(_p(pred), ld, _p(img_u8), _p(mask_u8), _p(out_u8), H, W, Hp, Wp, _stream()),
          "drag_lama_blend_u8")


# ---- float32 CLIP tower ------------------------------------------------------------------------------------
def linear_f32(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, M: int, *, ldx: int, ldy: int, bias=None, act: int = CONV_ACT_NONE,
               resid=None, ld_res: int = 0) -> torch.Tensor:
    """y[m, :N] = act(x[m, :K] @ w.T + bias) + resid on the f32 matrix core (a 1x1 convolution over M "pixels"); w [N, K]"""
    N, K = w.shape
    return conv2d_f32(x, w.view(N, 1, 1, K), y, B=1, Hi=1, Wi=M, Ho=1, Wo=M, Cin=K, ldx=ldx, ldy=ldy, act=act, shift=bias,
                      resid=resid, ld_res=ld_res)


def vit_prepare(img: torch.Tensor, out: torch.Tensor, mean, std) -> None:
    """uint8 [B,S,S,3] or normalised float [B,3,S,S] -> NHWC f32 [B,S,S,4] (4th channel 0)"""
    lib = _lib.load()
    if img.dtype == torch.uint8:
        m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        check(lib.drag_vit_prepare_u8(_p(img), _p(out), img.numel() // 3, m, s, _stream()), "drag_vit_prepare_u8")
    else:
        _need(img, torch.float32, "vit_prepare.img")
        B = img.shape[0]
        check(lib.drag_vit_prepare_f32(_p(img), _p(out), B, img.numel() // (3 * B), _stream()), "drag_vit_prepare_f32")


def layernorm_f32(x, y, gamma, beta, rows: int, D: int, eps: float, ldx: int | None = None, ldy: int | None = None) -> None:
    check(_lib.load().drag_layernorm_f32(_p(x), _p(y), _p(gamma), _p(beta), rows, D, ldx or D, ldy or D, eps, _stream()), "drag_layernorm_f32")


def clip_embed_ln(emb, cls, pos, gamma, beta, x, B: int, T: int, D: int, eps: float) -> None:
    check(_lib.load().drag_clip_embed_ln_f32(_p(emb), _p(cls), _p(pos), _p(gamma), _p(beta), _p(x), B, T, D, eps, _stream()),
          "drag_clip_embed_ln_f32")


def attention_small_f32(qkv, out, B: int, T: int, H: int, hd: int, ld: int, ldo: int, scale: float) -> None:
    check(_lib.load().drag_attention_small_f32(_p(qkv), _p(out), B, T, H, hd, ld, ldo, scale, _stream()), "drag_attention_small_f32")


def textenc_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int, *, ld: int,
                      batch_stride: int, scale: float, rel_bias: torch.Tensor | None = None, causal: bool = False, eager: bool,
                      ld_o: int | None = None, o_batch_stride: int | None = None) -> torch.Tensor:
    """head_dim-64 attention of the prompt encoders (``drag_textenc_attention_bf16``): ``q`` / ``k`` / ``v`` are views whose first element is
    head 0 of token 0 of batch 0 (token s of batch b at + b * batch_stride + s * ld, head h at + 64 h), ``out`` [B, S, H*64] rows of ``ld_o``.
    ``rel_bias`` bf16 [H, 2S-1] (T5), ``causal`` (CLIP); ``eager`` = T5's eager numerics, else CLIP's SDPA numerics."""
    lib = _lib.load()
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (out, "out")):
        _need(t, torch.bfloat16, f"textenc_attention.{n}")
    ld_o = H * 64 if ld_o is None else ld_o
    o_batch_stride = S * ld_o if o_batch_stride is None else o_batch_stride
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _fit(t, _rows_reach(B * S, H * 64, ld, S, batch_stride), f"textenc_attention.{n}: the rows do not fit the buffer", B * S, H * 64, ld, S, batch_stride)
    _fit(out, _rows_reach(B * S, H * 64, ld_o, S, o_batch_stride), "textenc_attention.out: the output rows do not fit the destination",
         B * S, H * 64, ld_o, S, o_batch_stride)
    if rel_bias is not None:
        _need(rel_bias, torch.bfloat16, "textenc_attention.rel_bias")
        if tuple(rel_bias.shape) != (H, 2 * S - 1) or not rel_bias.is_contiguous():
            raise ValueError(f"textenc_attention.rel_bias: expected a contiguous [{H}, {2 * S - 1}] table, got {tuple(rel_bias.shape)}")
    check(lib.drag_textenc_attention_bf16(_p(q), _p(k), _p(v), _p(out), B, S, H, ld, batch_stride, ld_o, o_batch_stride, float(scale),
                                          _p(rel_bias), int(causal), int(eager), _stream()), "drag_textenc_attention_bf16")
    return out


def t5_rmsnorm(x: torch.Tensor, weight: torch.Tensor, out: torch.Tensor, eps: float) -> torch.Tensor:
    """T5LayerNorm of the dense rows of ``x`` [M, D] into ``out`` (``drag_t5_rmsnorm_bf16``)"""
    for t, n in ((x, "x"), (weight, "weight"), (out, "out")):
        _need(t, torch.bfloat16, f"t5_rmsnorm.{n}")
    D = weight.numel()
    if not (x.is_contiguous() and out.is_contiguous() and x.numel() % D == 0 and out.numel() == x.numel()):
        raise ValueError(f"t5_rmsnorm: x / out must be contiguous rows of {D} elements")
    check(_lib.load().drag_t5_rmsnorm_bf16(_p(x), _p(weight), _p(out), x.numel() // D, D, float(eps), _stream()), "drag_t5_rmsnorm_bf16")
    return out


def gated_new_gelu(h: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out`` [M, F] = NewGELU(h[:, :F]) * h[:, F:] of the fused wi_0 | wi_1 rows ``h`` [M, 2F] (``drag_gated_new_gelu_bf16``)"""
    _need(h, torch.bfloat16, "gated_new_gelu.h")
    _need(out, torch.bfloat16, "gated_new_gelu.out")
    M, F = out.shape
    if not (h.is_contiguous() and out.is_contiguous() and tuple(h.shape) == (M, 2 * F)):
        raise ValueError(f"gated_new_gelu: expected contiguous h [{M}, {2 * F}] and out [{M}, {F}], got {tuple(h.shape)}")
    check(_lib.load().drag_gated_new_gelu_bf16(_p(h), _p(out), M, F, _stream()), "drag_gated_new_gelu_bf16")
    return out


def quick_gelu(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """CLIP's QuickGELU in torch's bf16 op order (``drag_quick_gelu_bf16``); ``out`` may be ``x``"""
    _need(x, torch.bfloat16, "quick_gelu.x")
    out = torch.empty_like(x) if out is None else out
    _need(out, torch.bfloat16, "quick_gelu.out")
    if not (x.is_contiguous() and out.is_contiguous() and out.numel() == x.numel()):
        raise ValueError("quick_gelu: x / out must be contiguous tensors of the same size")
    check(_lib.load().drag_quick_gelu_bf16(_p(x), _p(out), x.numel(), _stream()), "drag_quick_gelu_bf16")
    return out


def embed_gather(ids: torch.Tensor, table: torch.Tensor, out: torch.Tensor, pos: torch.Tensor | None = None) -> torch.Tensor:
    """``out`` [B*S, D] = table[ids] (+ pos[s], one bf16 add) for int64 device ids [B, S] (``drag_embed_gather_bf16``).  The ids must lie
    in [0, vocab): the caller checks them on the host before they are uploaded (the kernel writes a zero row for any other id)."""
    _need(ids, torch.int64, "embed_gather.ids")
    _need(table, torch.bfloat16, "embed_gather.table")
    _need(out, torch.bfloat16, "embed_gather.out")
    B, S = ids.shape
    V, D = table.shape
    if not (ids.is_contiguous() and table.is_contiguous() and out.is_contiguous() and out.numel() == B * S * D):
        raise ValueError(f"embed_gather: expected contiguous ids [B, S], table [V, D] and out [{B * S}, {D}]")
    if pos is not None:
        _need(pos, torch.bfloat16, "embed_gather.pos")
        if not pos.is_contiguous() or pos.shape[-1] != D or pos.numel() < S * D:
            raise ValueError(f"embed_gather.pos: expected contiguous rows of {D} covering {S} positions")
    check(_lib.load().drag_embed_gather_bf16(_p(ids), _p(table), _p(pos), _p(out), B * S, S, D, V, _stream()), "drag_embed_gather_bf16")
    return out
