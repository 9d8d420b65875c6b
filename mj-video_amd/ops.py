"""Thin tensor-level wrappers over the C ABI: torch supplies device memory and the current HIP stream,
every computation happens in libmjv_hip.so.  Every function enqueues on the current HIP stream OF THE DEVICE ITS
TENSORS LIVE ON (``torch.cuda.current_stream(t.device)``) and makes that device the current one for the call (the
library reads the current device for its CU count and per-device kernel attributes), so a direct ``ops.*`` call on
cuda:1 tensors works whatever the caller's current device is.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RELU, EPI_ROPE_QKV, EPI_SCALE_RES, EPI_SILU_MUL, FMT_MXFP8, AttnCtxDesc, AttnCtxSegments,
                   AttnDesc, GemmDesc, HeadsDesc, check, load_library)

BF16 = torch.bfloat16


def _stream(t: torch.Tensor) -> int:
    """HIP stream handle for work on ``t``: the current stream of t's device (a model on cuda:1 must not be launched
    on cuda:0's stream just because cuda:0 is the current device)."""
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk_bf16(*ts):
    for t in ts:
        if t is not None and (t.dtype != BF16 or not t.is_cuda):
            raise TypeError(f"expected a bf16 device tensor, got {t.dtype} on {t.device}")


def _row_stride(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "rows must be contiguous"
    return t.stride(0)


class MX8:
    """An MXFP8 matrix on the GPU (include/mjv.h "MXFP8 operand format"): ``data`` uint8 [rows, cols] OCP e4m3 elements, ``scales``
    uint8 e8m0 block scales in the MFMA's lane layout (``mxfp8_scale_bytes(rows, cols)`` bytes).  Operand / output of the fp8
    FFN GEMMs; produced by ``quantize_mxfp8``, the ``*_mxfp8`` norms and ``gemm(..., out=MX8)``."""
    __slots__ = ("data", "scales")

    def __init__(self, data: torch.Tensor, scales: torch.Tensor):
        assert data.dtype == torch.uint8 and scales.dtype == torch.uint8 and data.is_cuda and scales.is_cuda
        assert data.dim() == 2 and data.stride(1) == 1 and data.shape[1] % 128 == 0, "MXFP8: [rows, cols % 128 == 0] row-contiguous"
        assert scales.is_contiguous() and scales.numel() >= mxfp8_scale_bytes(data.shape[0], data.shape[1])
        self.data, self.scales = data, scales

    @staticmethod
    def empty(rows: int, cols: int, device) -> "MX8":
        return MX8(torch.empty(rows, cols, dtype=torch.uint8, device=device),
                   torch.empty(mxfp8_scale_bytes(rows, cols), dtype=torch.uint8, device=device))

    @property
    def shape(self):
        return self.data.shape

    @property
    def device(self):
        return self.data.device

    def rows(self, n: int) -> "MX8":
        """the first ``n`` rows (same scale buffer: the records are indexed by absolute row; the GROUP count of the scale
        layout follows the row count, so only a view with the same ceil(rows / 64) addresses the same records)"""
        assert (n + 63) // 64 == (self.data.shape[0] + 63) // 64, "a row view must keep the number of 64-row scale groups"
        return MX8(self.data[:n], self.scales)


def mxfp8_scale_bytes(rows: int, cols: int) -> int:
    return (cols // 128) * ((rows + 63) // 64) * 256


def quantize_mxfp8(x: torch.Tensor, out: Optional[MX8] = None) -> MX8:
    """bf16 [rows, cols] -> MXFP8 (weights once at load; tests)."""
    _chk_bf16(x)
    rows, cols = x.shape
    out = MX8.empty(rows, cols, x.device) if out is None else out
    assert tuple(out.shape) == (rows, cols)
    with torch.cuda.device(x.device):
        check(load_library().mjv_quantize_mxfp8(x.data_ptr(), _row_stride(x), out.data.data_ptr(), _row_stride(out.data),
                                                out.scales.data_ptr(), rows, cols, _stream(x)), "mjv_quantize_mxfp8")
    return out


class _CallDefaults(threading.local):
    """Per-THREAD defaults of the per-call choices the C ABI takes in its descriptors (ABI 4 has no process-wide setter):
    the split-K scratch of this thread's GEMM calls, the forced tile kernel and the attention kernel (parity tests).  Two
    threads scoring on two streams each see their own."""
    gemm_ws: Optional[torch.Tensor] = None
    tile: int = 0
    attn_kernel: int = 0


_tls = _CallDefaults()


def gemm_workspace_bytes() -> int:
    return int(load_library().mjv_gemm_workspace_bytes())


def set_gemm_workspace(ws: Optional[torch.Tensor]) -> None:
    """Scratch buffer handed to every following ``gemm`` call of THIS THREAD that does not pass its own ``workspace``
    (uint8/any dtype, on the GPU, private to the stream the calls go to while they are in flight).  None: never split K."""
    if ws is not None:
        assert ws.is_cuda and ws.is_contiguous() and ws.data_ptr() % 16 == 0
    _tls.gemm_ws = ws


def gemm_desc_plan(d: GemmDesc, cus: int = 0) -> dict:
    """``mjv_gemm_plan`` (include/mjv.h) of a filled descriptor: what ``mjv_gemm_bf16`` would launch for it on ``cus`` compute
    units (0: the current device) - ``dict(gm, nt_store, launches=[dict(family, epilogue, row0, rows, split, grid, persistent,
    rope_split_after), ...])``.  Reads no device memory and launches nothing: works without a GPU when ``cus`` is given."""
    lib = load_library()
    n = int(lib.mjv_gemm_plan(C.byref(d), cus, None, 0))
    check(min(0, n), "mjv_gemm_plan")
    buf = (C.c_int32 * n)()
    check(min(0, int(lib.mjv_gemm_plan(C.byref(d), cus, buf, n))), "mjv_gemm_plan")
    keys = ("family", "epilogue", "row0", "rows", "split", "grid", "persistent", "rope_split_after")
    return dict(gm=buf[1], nt_store=buf[2], launches=[dict(zip(keys, buf[4 + 8 * i:12 + 8 * i])) for i in range(buf[0])])


def gemm_plan(*args, cus: int = 0, **kw) -> dict:
    """the plan (``gemm_desc_plan``) of the launches ``gemm(*args, **kw)`` would make; nothing runs"""
    return gemm(*args, _plan_cus=cus, **kw)


def _gemm_mxfp8(a: MX8, w: MX8, out, epilogue: int, bias, scale, res, M: Optional[int], workspace=None, tile=None, _plan_cus=None):
    """MXFP8 operands (include/mjv.h, ABI 5): ``out`` a bf16 tensor or an ``MX8`` (the epilogue's result block-quantised)."""
    assert isinstance(w, MX8), "MXFP8 activations need MXFP8 weights"
    _chk_bf16(bias, scale, res)
    d = GemmDesc()
    d.A, d.lda = a.data.data_ptr(), _row_stride(a.data)
    d.W, d.ldw = w.data.data_ptr(), _row_stride(w.data)
    d.M = a.shape[0] if M is None else M
    assert d.M == a.shape[0], "an MXFP8 operand's scale records are laid out for its own row count"
    d.N, d.K = w.shape[0], w.shape[1]
    assert a.shape[1] == d.K, (a.shape, w.shape)
    d.a_format = d.w_format = FMT_MXFP8
    d.a_scales, d.w_scales = a.scales.data_ptr(), w.scales.data_ptr()
    nout = d.N // 2 if epilogue == EPI_SILU_MUL else d.N
    if isinstance(out, MX8):
        assert tuple(out.shape) == (d.M, nout), (tuple(out.shape), d.M, nout)
        d.C, d.ldc, d.c_format, d.c_scales = out.data.data_ptr(), _row_stride(out.data), FMT_MXFP8, out.scales.data_ptr()
        dev = out.data.device
    else:
        _chk_bf16(out)
        d.C, d.ldc = out.data_ptr(), _row_stride(out)
        dev = out.device
    d.epilogue = epilogue
    d.bias, d.scale = _p(bias), _p(scale)
    d.res, d.ldr = _p(res), (_row_stride(res) if res is not None else 0)
    # (the split-K scratch: peeled tail rows / under-filled launches run K-sliced; a forced tile = the one unsliced launch)
    ws = workspace if workspace is not None else _tls.gemm_ws
    if ws is not None and ws.device == dev:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    d.tile = _tls.tile if tile is None else tile
    if d.tile not in (0, 256):
        d.tile = 256    # (one tile kernel exists for MXFP8 operands: the parity tests' tile sweep maps onto it)
    with torch.cuda.device(dev):
        if _plan_cus is not None:
            return gemm_desc_plan(d, _plan_cus)
        check(load_library().mjv_gemm_bf16(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mjv_gemm_bf16(mxfp8)")
    return out


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, epilogue: int = EPI_BIAS,
         bias: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, res_mod: int = 0, res_off: int = 0, out_group: int = 0,
         out_pad: int = 0, out_rows: Optional[torch.Tensor] = None, M: Optional[int] = None,
         rope: Optional[tuple] = None, workspace: Optional[torch.Tensor] = None, tile: Optional[int] = None,
         folded_norm: Optional[tuple] = None, _plan_cus: Optional[int] = None) -> torch.Tensor:
    """out = epilogue(a[M,K] @ w[N,K]^T); 2-D row-contiguous bf16 views (row strides are honoured).
    ``rope`` (EPI_ROPE_QKV only) = (cos, sin, positions, q_out, k_out, group): see include/mjv.h.
    ``workspace``: split-K scratch of THIS call (default: the calling thread's ``set_gemm_workspace`` buffer);
    ``tile``: 0 automatic, 64 / 128 / 256 force one tile kernel (default: the calling thread's ``gemm_set_tile`` value).
    ``a`` and ``w`` may be ``MX8`` (MXFP8 operands, ABI 5), ``out`` then a bf16 tensor or an ``MX8``.
    ``folded_norm`` = (row_scale,) or (row_scale, row_shift, col_shift, bias_f32): fp32 vectors of a norm folded into this GEMM
    (include/mjv.h "row_scale"; row vectors of ``padded_rows(M)`` entries from ``row_stats``, column vectors of
    ``padded_rows(N)``)."""
    if isinstance(a, MX8):
        assert res_mod == 0 and out_group == 0 and out_rows is None and rope is None, "MXFP8 GEMMs write plain rows"
        return _gemm_mxfp8(a, w, out, epilogue, bias, scale, res, M, workspace, tile, _plan_cus)
    _chk_bf16(a, w, out, bias, scale, res)
    lib = load_library()
    d = GemmDesc()
    d.A, d.lda = a.data_ptr(), _row_stride(a)
    d.W, d.ldw = w.data_ptr(), _row_stride(w)
    d.C, d.ldc = out.data_ptr(), _row_stride(out)
    d.M = a.shape[0] if M is None else M
    d.N, d.K = w.shape[0], w.shape[1]
    assert a.shape[1] == d.K, (a.shape, w.shape)
    d.epilogue = epilogue
    d.bias, d.scale = _p(bias), _p(scale)
    d.res, d.ldr = _p(res), (_row_stride(res) if res is not None else 0)
    d.res_mod, d.res_off, d.out_group, d.out_pad = res_mod, res_off, out_group, out_pad
    if out_rows is not None:
        assert out_rows.dtype == torch.int32 and out_rows.is_cuda
    d.out_rows = _p(out_rows)
    if epilogue == EPI_ROPE_QKV:
        cos, sin, positions, q_out, k_out, group = rope
        _chk_bf16(cos, sin, q_out, k_out)
        assert positions.dtype == torch.int32 and positions.is_cuda and positions.numel() >= d.M
        assert cos.shape[1] == 128 and cos.is_contiguous() and sin.is_contiguous()
        d.rope_cos, d.rope_sin, d.rope_pos = cos.data_ptr(), sin.data_ptr(), positions.data_ptr()
        d.rope_q, d.rope_k = _p(q_out), k_out.data_ptr()   # (q_out None with group 0: a k | v projection, no q heads)
        d.rope_ldq, d.rope_ldk, d.rope_group = (_row_stride(q_out) if q_out is not None else 0), _row_stride(k_out), group
    if folded_norm is not None:
        for t, n in zip(folded_norm, (d.M, d.M, d.N, d.N)):
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() >= padded_rows(n), (t.shape, n)
        d.row_scale = folded_norm[0].data_ptr()
        if len(folded_norm) == 4:
            d.row_shift, d.col_shift, d.bias_f32 = (t.data_ptr() for t in folded_norm[1:])
        else:
            assert len(folded_norm) == 1
    ws = workspace if workspace is not None else _tls.gemm_ws
    if ws is not None and ws.device == a.device:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    d.tile = _tls.tile if tile is None else tile
    with torch.cuda.device(out.device):   # the library plans against / sets attributes on the CURRENT device
        if _plan_cus is not None:
            return gemm_desc_plan(d, _plan_cus)
        check(lib.mjv_gemm_bf16(C.byref(d), _stream(out)), "mjv_gemm_bf16")
    return out


def gemm_set_tile(tile: int) -> None:
    """This THREAD's default tile kernel: 0 = automatic choice, 64 / 128 / 256 = force that kernel (parity tests).  Codes
    >= 1000 are the measurement switches of the bench build (include/mjv_bench.h; process-wide) and need that library
    (MJV_LIBRARY=.../libmjv_hip_bench.so)."""
    if tile in (0, 64, 128, 256):
        _tls.tile = tile
        if tile == 0 and hasattr(load_library(), "mjv_bench_gemm_set") and getattr(load_library().mjv_bench_gemm_set, "argtypes", None):
            check(load_library().mjv_bench_gemm_set(1000), "mjv_bench_gemm_set")   # "automatic" also leaves the kernel variants
        return
    lib = load_library()
    if getattr(getattr(lib, "mjv_bench_gemm_set", None), "argtypes", None) is None:
        raise _lib.MjvLibraryError(f"gemm_set_tile({tile}): measurement switches exist in the bench build only "
                                   "(make -C mj-video_amd/csrc bench; MJV_LIBRARY=<repo>/mj-video_amd/libmjv_hip_bench.so)")
    check(lib.mjv_bench_gemm_set(tile), "mjv_bench_gemm_set")


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, cu_seqlens: torch.Tensor,
              max_seqlen: int, n_heads: int, kv_group: int, head_dim: int, causal: bool, scale: float,
              score_round_mode: int, q_head_stride: Optional[int] = None, k_head_stride: Optional[int] = None,
              v_head_stride: Optional[int] = None, o_head_stride: Optional[int] = None,
              kernel: Optional[int] = None, cu_seqlens_q: Optional[torch.Tensor] = None, max_seqlen_q: int = 0,
              prefix_k: Optional[torch.Tensor] = None, prefix_v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q/k/v/out are 2-D views [rows, >= heads*head_dim] (row stride honoured, first head at column 0).
    ``kernel``: 0 automatic, 4 / 5 = the round-1 / round-2 kernels (default: the calling thread's ``attention_set_variant``).
    Causal only (include/mjv.h ABI 6): ``cu_seqlens_q`` / ``max_seqlen_q`` - the queries are the LAST rows of every sequence,
    packed at those offsets of q / out; ``prefix_k`` / ``prefix_v`` [P, ...] - P (a multiple of 64) shared keys / values in front of
    every sequence's own rows, same row stride and head stride as k / v."""
    _chk_bf16(q, k, v, out)
    assert cu_seqlens.dtype == torch.int32 and cu_seqlens.is_cuda
    lib = load_library()
    d = AttnDesc()
    d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldv, d.ldo = _row_stride(q), _row_stride(k), _row_stride(v), _row_stride(out)
    d.q_head_stride = head_dim if q_head_stride is None else q_head_stride
    d.k_head_stride = head_dim if k_head_stride is None else k_head_stride
    d.v_head_stride = head_dim if v_head_stride is None else v_head_stride
    d.o_head_stride = head_dim if o_head_stride is None else o_head_stride
    d.cu_seqlens = cu_seqlens.data_ptr()
    d.n_seqs, d.max_seqlen = cu_seqlens.numel() - 1, max_seqlen
    d.n_heads, d.kv_group, d.head_dim = n_heads, kv_group, head_dim
    d.causal, d.scale, d.score_round_mode = int(causal), scale, score_round_mode
    d.kernel = _tls.attn_kernel if kernel is None else kernel
    if cu_seqlens_q is not None:
        assert cu_seqlens_q.dtype == torch.int32 and cu_seqlens_q.is_cuda and cu_seqlens_q.numel() == cu_seqlens.numel()
        d.cu_seqlens_q, d.max_seqlen_q = cu_seqlens_q.data_ptr(), max_seqlen_q
    if prefix_k is not None or prefix_v is not None:
        _chk_bf16(prefix_k, prefix_v)
        assert _row_stride(prefix_k) == d.ldk and _row_stride(prefix_v) == d.ldv and prefix_k.shape[0] == prefix_v.shape[0]
        d.prefix_k, d.prefix_v, d.prefix_len = prefix_k.data_ptr(), prefix_v.data_ptr(), prefix_k.shape[0]
    with torch.cuda.device(out.device):
        check(lib.mjv_attention_bf16(C.byref(d), _stream(out)), "mjv_attention_bf16")
    return out


class AttnCtxPlan:
    """What one batch of the caption pass needs for ``attention_ctx`` (include/mjv.h, mjv_attn_ctx_desc): the HOST index arrays
    (kept alive here: the C entry reads them in every call), the device copy of the plan ``mjv_attention_ctx_plan`` derived from
    them, and the size of the fp32 partials.  Built once per batch, used by every layer's launch.
    ``segments`` (mjv_attn_ctx_segments; None = plain contexts): one sequence per context of its uses in key order, a use =
    (entry of the launch's tensor list, the number of that tensor's first rows it reads); ``n_tensors``: entries of the tensor
    list (default: the largest entry named + 1).  ``cu_context`` still gives every context's total."""

    def __init__(self, cu_seqlens, context_index, cu_context, n_heads: int, kv_group: int, head_dim: int, device,
                 cu_seqlens_q=None, any_length: bool = False, segments=None, n_tensors: Optional[int] = None):
        import numpy as np
        self.segmented = segments is not None
        if self.segmented:
            uses = [[(int(t), int(n)) for t, n in ctx] for ctx in segments]
            flat = [u for ctx in uses for u in ctx]
            self.cu_use = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(ctx) for ctx in uses])]), dtype=np.int32)
            self.use_tensor = np.ascontiguousarray([u[0] for u in flat], dtype=np.int32)
            self.use_len = np.ascontiguousarray([u[1] for u in flat], dtype=np.int32)
            self.n_tensors = int(n_tensors) if n_tensors is not None else (int(self.use_tensor.max()) + 1 if flat else 0)
            if len(uses) != len(cu_context) - 1:
                raise ValueError(f"attention_ctx plan: segments for {len(uses)} contexts, cu_context describes {len(cu_context) - 1}")
        self.any_length = bool(any_length)   # contexts of any positive length (mjv_attn_ctx_desc.ctx_any_length); False: multiples of 64
        as_i32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.int32))  # noqa: E731
        self.cu, self.cu_q, self.index, self.cu_ctx = as_i32(cu_seqlens), as_i32(cu_seqlens_q), as_i32(context_index), as_i32(cu_context)
        if self.cu.ndim != 1 or self.cu.size < 2 or self.index.shape != (self.cu.size - 1,) or self.cu_ctx.ndim != 1 or self.cu_ctx.size < 2 \
                or (self.cu_q is not None and self.cu_q.shape != self.cu.shape):
            raise ValueError("attention_ctx plan: cu_seqlens [n + 1], context_index [n], cu_context [contexts + 1], cu_seqlens_q [n + 1] or None")
        self.n_heads, self.kv_group, self.head_dim, self.device = n_heads, kv_group, head_dim, torch.device(device)
        lib = load_library()
        d, sg = self.desc(), self.seg_desc()
        n = lib.mjv_attention_ctx_seg_plan(C.byref(d), sg, None, 0)
        if n < 0:
            check(int(n), "mjv_attention_ctx_plan")
        host = np.empty(int(n), dtype=np.int32)
        check(min(0, int(lib.mjv_attention_ctx_seg_plan(C.byref(d), sg, host.ctypes.data, int(n)))), "mjv_attention_ctx_plan")
        self.plan_ints = int(n)
        self.workspace_bytes = int(lib.mjv_attention_ctx_seg_workspace_bytes(C.byref(d), sg))
        self.total_q = int((self.cu_q if self.cu_q is not None else self.cu)[-1])
        self.plan = torch.from_numpy(host).to(self.device, non_blocking=False)

    def desc(self) -> AttnCtxDesc:
        d = AttnCtxDesc()
        d.cu_seqlens, d.context_index, d.cu_context = self.cu.ctypes.data, self.index.ctypes.data, self.cu_ctx.ctypes.data
        d.cu_seqlens_q = None if self.cu_q is None else self.cu_q.ctypes.data
        d.n_seqs, d.n_contexts = self.cu.size - 1, self.cu_ctx.size - 1
        d.n_heads, d.kv_group, d.head_dim, d.causal = self.n_heads, self.kv_group, self.head_dim, 1
        d.ctx_any_length = int(self.any_length)
        return d

    def seg_desc(self):
        """the plan's mjv_attn_ctx_segments (its arrays are kept alive here), or None for plain contexts"""
        if not self.segmented:
            return None
        sg = AttnCtxSegments()
        sg.cu_use, sg.use_tensor, sg.use_len = self.cu_use.ctypes.data, self.use_tensor.ctypes.data, self.use_len.ctypes.data
        sg.n_uses, sg.n_tensors = self.use_tensor.size, self.n_tensors
        return sg


def _check_ctx_rows(ctx_k, ctx_v, plan: "AttnCtxPlan", device, k_head_stride: int, v_head_stride: int):
    """``attention_ctx`` with per-context tensors: every context's keys / values are read WHERE THEY LIE, so each tensor is held
    to what the launch assumes of all of them before anything is launched - the device, bf16, at least the context's length in
    rows, a 16-byte aligned first row, one leading dimension per operand, columns for every kv head at the shared head stride.
    Host code (tensor attributes only).  Returns (ld_ctx_k, ld_ctx_v)."""
    if plan.segmented:   # one tensor per list entry; a tensor holds at least the rows of the longest use that names it
        import numpy as np
        n_ctx, what_n = plan.n_tensors, "segment tensors"
        lens = np.zeros(n_ctx, dtype=np.int64)
        np.maximum.at(lens, plan.use_tensor, plan.use_len)
    else:
        n_ctx, what_n = plan.cu_ctx.size - 1, "contexts"
        lens = plan.cu_ctx[1:] - plan.cu_ctx[:-1]
    if len(ctx_k) != n_ctx or len(ctx_v) != n_ctx:
        raise ValueError(f"attention_ctx: {len(ctx_k)} key / {len(ctx_v)} value tensors for the plan's {n_ctx} {what_n}")
    n_kv = plan.n_heads // plan.kv_group
    lds = []
    for what, ts, hs in (("keys", ctx_k, k_head_stride), ("values", ctx_v, v_head_stride)):
        ld = None
        for c, t in enumerate(ts):
            who = f"attention_ctx: {'segment tensor' if plan.segmented else 'context'} {c} ({what})"
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who}: not a tensor")
            if t.device != device:
                raise ValueError(f"{who} lives on {t.device}, the launch on {device}")
            if t.dtype != BF16:
                raise TypeError(f"{who}: expected bfloat16, got {t.dtype}")
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{who}: expected 2-D rows of contiguous elements, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.shape[0] < int(lens[c]):
                raise ValueError(f"{who}: {t.shape[0]} rows, the {'longest use of it reads' if plan.segmented else 'context has'} {int(lens[c])}")
            if t.shape[1] < (n_kv - 1) * hs + plan.head_dim:
                raise ValueError(f"{who}: {t.shape[1]} columns do not hold {n_kv} heads of {plan.head_dim} at head stride {hs}")
            if t.data_ptr() % 16:
                raise ValueError(f"{who}: its first row is not 16-byte aligned")
            if ld is None:
                ld = t.stride(0)
            elif t.stride(0) != ld:
                raise ValueError(f"{who}: leading dimension {t.stride(0)}, context 0 has {ld} (one stride for every context)")
        lds.append(ld)
    return lds[0], lds[1]


def ctx_pointer_rows(ctx_k, ctx_v) -> "np.ndarray":
    """host int64 [2, contexts]: the first-row addresses of every context's keys (row 0) and values (row 1) - what
    ``attention_ctx`` takes, uploaded, as ``ctx_list``"""
    import numpy as np
    return np.asarray([[t.data_ptr() for t in ctx_k], [t.data_ptr() for t in ctx_v]], dtype=np.int64)


def attention_ctx(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, ctx_k, ctx_v,
                  plan: AttnCtxPlan, scale: float, score_round_mode: int, workspace: Optional[torch.Tensor],
                  q_head_stride: Optional[int] = None, k_head_stride: Optional[int] = None, v_head_stride: Optional[int] = None,
                  o_head_stride: Optional[int] = None, ctx_k_head_stride: Optional[int] = None,
                  ctx_v_head_stride: Optional[int] = None, causal: bool = True,
                  ctx_list: Optional[torch.Tensor] = None, segments=None) -> torch.Tensor:
    """Causal attention of every sequence's own rows (q / k / v / out: 2-D views as in ``attention``) over
    [its context's rows | its own rows] (include/mjv.h, mjv_attention_ctx_bf16).  ``ctx_k`` / ``ctx_v``: every context's rows in ONE
    packed tensor each (context c at rows ``plan.cu_ctx[c]`` ...), or both a SEQUENCE of one tensor per context, read where they
    lie (ctx_k_list / ctx_v_list of the descriptor; every tensor is checked here, before any launch: ``_check_ctx_rows``).
    ``ctx_list`` (with sequences): a device int64 tensor [2, contexts] holding ``ctx_pointer_rows(ctx_k, ctx_v)`` - a caller with
    many launches over the same contexts uploads all its rows once; None: uploaded here.  ``plan``: the batch's
    ``AttnCtxPlan``; ``workspace``: a uint8 device tensor of at least ``plan.workspace_bytes`` (the library allocates nothing).
    A plan built with ``segments`` makes the launch segmented (mjv_attention_ctx_seg_bf16): ``ctx_k`` / ``ctx_v`` are then the
    sequences of SEGMENT TENSORS the plan's uses name (one per list entry, checked per use: rows >= the use's length), never
    packed.  ``segments`` here: None = the plan's own; given, it must be what the plan was built from."""
    hd = plan.head_dim
    if segments is not None:
        uses = [(int(t), int(n)) for ctx in segments for t, n in ctx]
        if not plan.segmented or uses != list(zip(plan.use_tensor.tolist(), plan.use_len.tolist())) \
                or [len(ctx) for ctx in segments] != (plan.cu_use[1:] - plan.cu_use[:-1]).tolist():
            raise ValueError("attention_ctx: segments differ from those the plan was built from")
    kchs = hd if ctx_k_head_stride is None else ctx_k_head_stride
    vchs = hd if ctx_v_head_stride is None else ctx_v_head_stride
    listed = [not isinstance(t, torch.Tensor) for t in (ctx_k, ctx_v)]
    if listed[0] != listed[1]:
        raise ValueError("attention_ctx: ctx_k and ctx_v must both be one packed tensor, or both a sequence of per-context tensors")
    listed = listed[0]
    if plan.segmented and not listed:
        raise ValueError("attention_ctx: a segmented plan needs sequences of segment tensors, not packed ctx_k / ctx_v")
    if listed:
        ctx_k, ctx_v = list(ctx_k), list(ctx_v)
        ld_ck, ld_cv = _check_ctx_rows(ctx_k, ctx_v, plan, q.device, kchs, vchs)
        if ctx_list is not None and (ctx_list.dtype != torch.int64 or ctx_list.device != q.device or not ctx_list.is_contiguous()
                                     or tuple(ctx_list.shape) != (2, len(ctx_k))):
            raise ValueError(f"attention_ctx: ctx_list must be a contiguous int64 tensor [2, {len(ctx_k)}] on {q.device}")
    elif ctx_list is not None:
        raise ValueError("attention_ctx: ctx_list goes with per-context tensors, not with packed ctx_k / ctx_v")
    _chk_bf16(q, k, v, out)
    if not listed:
        _chk_bf16(ctx_k, ctx_v)
    if q.shape[0] < plan.total_q or out.shape[0] < plan.total_q or k.shape[0] < int(plan.cu[-1]) or v.shape[0] < int(plan.cu[-1]) \
            or (not listed and (ctx_k.shape[0] < int(plan.cu_ctx[-1]) or ctx_v.shape[0] < int(plan.cu_ctx[-1]))):
        raise ValueError("attention_ctx: a tensor holds fewer rows than the plan's index arrays address")
    if workspace is not None and (workspace.dtype != torch.uint8 or not workspace.is_cuda):
        raise TypeError("attention_ctx: workspace must be a uint8 device tensor")
    d = plan.desc()
    d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldv, d.ldo = _row_stride(q), _row_stride(k), _row_stride(v), _row_stride(out)
    d.q_head_stride = hd if q_head_stride is None else q_head_stride
    d.k_head_stride = hd if k_head_stride is None else k_head_stride
    d.v_head_stride = hd if v_head_stride is None else v_head_stride
    d.o_head_stride = hd if o_head_stride is None else o_head_stride
    if listed:
        if ctx_list is None:
            ctx_list = torch.from_numpy(ctx_pointer_rows(ctx_k, ctx_v)).to(q.device)
        d.ctx_k_list, d.ctx_v_list = ctx_list[0].data_ptr(), ctx_list[1].data_ptr()
        d.ld_ctx_k, d.ld_ctx_v = ld_ck, ld_cv
    else:
        d.ctx_k, d.ctx_v, d.ld_ctx_k, d.ld_ctx_v = ctx_k.data_ptr(), ctx_v.data_ptr(), _row_stride(ctx_k), _row_stride(ctx_v)
    d.ctx_k_head_stride, d.ctx_v_head_stride = kchs, vchs
    d.causal, d.scale, d.score_round_mode = int(causal), scale, score_round_mode
    d.plan, d.plan_ints = plan.plan.data_ptr(), plan.plan_ints
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel()
    with torch.cuda.device(out.device):
        if plan.segmented:
            check(load_library().mjv_attention_ctx_seg_bf16(C.byref(d), plan.seg_desc(), _stream(out)), "mjv_attention_ctx_seg_bf16")
        else:
            check(load_library().mjv_attention_ctx_bf16(C.byref(d), _stream(out)), "mjv_attention_ctx_bf16")
    return out


class AttnReadoutPlan:
    """What one batch needs for ``attention_readout`` (include/mjv.h, mjv_attn_readout_desc): the HOST range / bin arrays (kept
    alive here: the C entry reads them in every call) and the device copy of the plan ``mjv_attention_readout_plan`` makes of them.
    Built once per batch, used by every layer's launch.  ``ranges``: per query its key ranges in key order, a range =
    (entry of the launch's tensor list, first row, rows); ``edges``: per query its ascending bin edges (bins + 1 of them, from 0 to
    the query's key count).  ``device`` None: the host plan only (``host``; no GPU is touched)."""

    def __init__(self, ranges, edges, n_heads: int, kv_group: int, head_dim: int, score_round_mode: int, device=None,
                 n_tensors: Optional[int] = None):
        import numpy as np
        ranges = [[(int(t), int(r0), int(n)) for t, r0, n in qr] for qr in ranges]
        edges = [[int(e) for e in qe] for qe in edges]
        if len(ranges) != len(edges):
            raise ValueError(f"attention_readout plan: ranges for {len(ranges)} queries, bin edges for {len(edges)}")
        flat = [r for qr in ranges for r in qr]
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))  # noqa: E731
        self.cu_range = i32(np.concatenate([[0], np.cumsum([len(qr) for qr in ranges])]))
        self.range_tensor, self.range_row0, self.range_rows = (i32([r[i] for r in flat]) for i in range(3))
        self.cu_bin = i32(np.concatenate([[0], np.cumsum([len(qe) for qe in edges])]))
        self.bin_edge = i32([e for qe in edges for e in qe])
        self.n_queries = len(ranges)
        self.n_tensors = int(n_tensors) if n_tensors is not None else (int(self.range_tensor.max()) + 1 if flat else 0)
        self.n_heads, self.kv_group, self.head_dim, self.score_round_mode = n_heads, kv_group, head_dim, score_round_mode
        self.max_bins = max((len(qe) - 1 for qe in edges), default=0)
        lib = load_library()
        d = self.desc()
        n = int(lib.mjv_attention_readout_plan(C.byref(d), None, 0))
        if n < 0:
            check(n, "mjv_attention_readout_plan")
        self.host = np.empty(n, dtype=np.int32)
        check(min(0, int(lib.mjv_attention_readout_plan(C.byref(d), self.host.ctypes.data, n))), "mjv_attention_readout_plan")
        self.plan_ints = n
        self.device = None if device is None else torch.device(device)
        self.plan = None if device is None else torch.from_numpy(self.host).to(self.device, non_blocking=False)

    def desc(self) -> "_lib.AttnReadoutDesc":
        d = _lib.AttnReadoutDesc()
        d.cu_range, d.range_tensor, d.range_row0, d.range_rows = (a.ctypes.data for a in (self.cu_range, self.range_tensor, self.range_row0,
                                                                                          self.range_rows))
        d.cu_bin, d.bin_edge = self.cu_bin.ctypes.data, self.bin_edge.ctypes.data
        d.n_queries, d.n_tensors = self.n_queries, self.n_tensors
        d.n_heads, d.kv_group, d.head_dim, d.score_round_mode = self.n_heads, self.kv_group, self.head_dim, self.score_round_mode
        return d


def attention_readout(q: torch.Tensor, k_tensors, plan: AttnReadoutPlan, scale: float, mass: torch.Tensor,
                      q_head_stride: Optional[int] = None, k_head_stride: Optional[int] = None,
                      k_list: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Softmax mass per bin of the plan's queries (include/mjv.h, mjv_attention_readout_bf16).  ``q``: 2-D view of at least
    ``plan.n_queries`` rows of already rotated queries; ``k_tensors``: the sequence of key tensors the plan's ranges name (2-D
    bf16 views, one leading dimension, first kv head at column 0; every range is checked against its tensor's rows here, before
    any launch); ``mass``: fp32 [>= n_queries, n_heads, >= plan.max_bins], contiguous - rows [0, n_queries) are written, bins
    beyond a query's count as 0.  ``k_list``: a device int64 tensor [len(k_tensors)] of the tensors' first-row addresses (a
    caller with many launches uploads them once); None: uploaded here."""
    import numpy as np
    hd = plan.head_dim
    k_tensors = list(k_tensors)
    if plan.plan is None or plan.plan.device != q.device:
        raise ValueError("attention_readout: the plan holds no device copy on the queries' device")
    if len(k_tensors) != plan.n_tensors:
        raise ValueError(f"attention_readout: {len(k_tensors)} key tensors for the plan's {plan.n_tensors}")
    _chk_bf16(q, *k_tensors)
    khs = hd if k_head_stride is None else k_head_stride
    n_kv = plan.n_heads // plan.kv_group
    need = np.zeros(plan.n_tensors, dtype=np.int64)
    np.maximum.at(need, plan.range_tensor, plan.range_row0.astype(np.int64) + plan.range_rows)
    ldk = None
    for t, kt in enumerate(k_tensors):
        who = f"attention_readout: key tensor {t}"
        if kt.device != q.device:
            raise ValueError(f"{who} lives on {kt.device}, the queries on {q.device}")
        if kt.dim() != 2 or kt.stride(1) != 1:
            raise ValueError(f"{who}: expected 2-D rows of contiguous elements, got shape {tuple(kt.shape)} strides {kt.stride()}")
        if kt.shape[0] < int(need[t]):
            raise ValueError(f"{who}: {kt.shape[0]} rows, a range of the plan reads up to row {int(need[t])}")
        if kt.shape[1] < (n_kv - 1) * khs + hd:
            raise ValueError(f"{who}: {kt.shape[1]} columns do not hold {n_kv} heads of {hd} at head stride {khs}")
        if kt.data_ptr() % 16:
            raise ValueError(f"{who}: its first row is not 16-byte aligned")
        if ldk is None:
            ldk = kt.stride(0)
        elif kt.stride(0) != ldk and kt.shape[0] > 1:
            raise ValueError(f"{who}: leading dimension {kt.stride(0)}, tensor 0 has {ldk} (one stride for every tensor)")
    if q.shape[0] < plan.n_queries:
        raise ValueError(f"attention_readout: {q.shape[0]} query rows, the plan has {plan.n_queries}")
    if mass.dtype != torch.float32 or mass.device != q.device or mass.dim() != 3 or not mass.is_contiguous() \
            or mass.shape[0] < plan.n_queries or mass.shape[1] != plan.n_heads or mass.shape[2] < plan.max_bins:
        raise ValueError(f"attention_readout: mass must be a contiguous fp32 tensor [>= {plan.n_queries}, {plan.n_heads}, >= {plan.max_bins}] "
                         f"on {q.device}")
    if k_list is None:
        k_list = torch.tensor([kt.data_ptr() for kt in k_tensors], dtype=torch.int64).to(q.device)
    elif k_list.dtype != torch.int64 or k_list.device != q.device or not k_list.is_contiguous() or k_list.numel() != len(k_tensors):
        raise ValueError(f"attention_readout: k_list must be a contiguous int64 tensor [{len(k_tensors)}] on {q.device}")
    d = plan.desc()
    d.Q, d.ldq, d.q_head_stride = q.data_ptr(), _row_stride(q), hd if q_head_stride is None else q_head_stride
    d.k_list, d.ldk, d.k_head_stride = k_list.data_ptr(), ldk, khs
    d.scale = scale
    d.mass, d.ld_mass = mass.data_ptr(), mass.shape[2]
    d.plan, d.plan_ints = plan.plan.data_ptr(), plan.plan_ints
    with torch.cuda.device(q.device):
        check(load_library().mjv_attention_readout_bf16(C.byref(d), _stream(q)), "mjv_attention_readout_bf16")
    return mass


def attention_set_variant(v: int) -> None:
    """This THREAD's default attention kernel: 0 automatic, 4 = register-staged round-1 kernel, 5 = round-2 choice, 6 / 7 =
    round-3 kernel with two / four waves per workgroup (all correct; tests A/B them).  1-3 are measurement variants of the
    bench build (process-wide, bench library only)."""
    lib = load_library()
    bench = getattr(getattr(lib, "mjv_bench_attention_set", None), "argtypes", None) is not None
    if v in (0, 4, 5, 6, 7):
        _tls.attn_kernel = v
        if bench:
            check(lib.mjv_bench_attention_set(0), "mjv_bench_attention_set")
        return
    if not bench:
        raise _lib.MjvLibraryError(f"attention_set_variant({v}): measurement variants exist in the bench build only")
    _tls.attn_kernel = 5 if v in (1, 2, 3) else 0
    check(lib.mjv_bench_attention_set(v), "mjv_bench_attention_set")


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, eps: float,
              rows: Optional[int] = None, gather_grid: int = 0) -> torch.Tensor:
    _chk_bf16(x, gamma, beta, out)
    lib = load_library()
    rows = out.shape[0] if rows is None else rows
    with torch.cuda.device(out.device):
        check(lib.mjv_layernorm_bf16(x.data_ptr(), _row_stride(x), out.data_ptr(), _row_stride(out), gamma.data_ptr(),
                                     beta.data_ptr(), rows, out.shape[1], eps, gather_grid, _stream(out)),
              "mjv_layernorm_bf16")
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, eps: float,
            row_index: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_bf16(x, w, out)
    lib = load_library()
    if row_index is not None:
        assert row_index.dtype == torch.int32 and row_index.is_cuda
    with torch.cuda.device(out.device):
        check(lib.mjv_rmsnorm_bf16(x.data_ptr(), _row_stride(x), out.data_ptr(), _row_stride(out), w.data_ptr(),
                                   _p(row_index), out.shape[0], out.shape[1], eps, _stream(out)), "mjv_rmsnorm_bf16")
    return out


def layernorm_mxfp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: MX8, eps: float) -> MX8:
    """``layernorm`` with the bf16 result block-quantised on the way out (the input of the fp8 fc1 GEMM)."""
    _chk_bf16(x, gamma, beta)
    assert tuple(out.shape) == tuple(x.shape)
    with torch.cuda.device(x.device):
        check(load_library().mjv_layernorm_mxfp8(x.data_ptr(), _row_stride(x), out.data.data_ptr(), _row_stride(out.data),
                                                 out.scales.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.shape[0], x.shape[1],
                                                 eps, _stream(x)), "mjv_layernorm_mxfp8")
    return out


def rmsnorm_mxfp8(x: torch.Tensor, w: torch.Tensor, out: MX8, eps: float) -> MX8:
    _chk_bf16(x, w)
    assert tuple(out.shape) == tuple(x.shape)
    with torch.cuda.device(x.device):
        check(load_library().mjv_rmsnorm_mxfp8(x.data_ptr(), _row_stride(x), out.data.data_ptr(), _row_stride(out.data),
                                               out.scales.data_ptr(), w.data_ptr(), x.shape[0], x.shape[1], eps, _stream(x)),
              "mjv_rmsnorm_mxfp8")
    return out


def padded_rows(n: int) -> int:
    """entries a row / column vector of a folded norm must hold for n rows / columns (whole 256-tiles are fetched)"""
    return (n + 255) // 256 * 256


def row_stats(x: torch.Tensor, rstd: torch.Tensor, mean_rstd: Optional[torch.Tensor], eps: float) -> None:
    """rstd[m] (and mean[m] * rstd[m]: LayerNorm; None: RMSNorm statistics) of the rows of ``x`` - the producer half of a norm
    folded into its consuming GEMM (``gemm(..., folded_norm=...)``)."""
    _chk_bf16(x)
    assert rstd.dtype == torch.float32 and rstd.is_cuda and rstd.numel() >= x.shape[0]
    assert mean_rstd is None or (mean_rstd.dtype == torch.float32 and mean_rstd.numel() >= x.shape[0])
    with torch.cuda.device(x.device):
        check(load_library().mjv_row_stats_bf16(x.data_ptr(), _row_stride(x), rstd.data_ptr(), _p(mean_rstd), x.shape[0], x.shape[1],
                                                eps, _stream(x)), "mjv_row_stats_bf16")


def rope_split(qkv: torch.Tensor, q: Optional[torch.Tensor], k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
               positions: torch.Tensor, kv_heads: int, group: int) -> None:
    """``group`` 0 (include/mjv.h): the rows are [k | v] pairs without q heads, ``q`` is None."""
    _chk_bf16(qkv, q, k, cos, sin)
    assert (q is None) == (group == 0), "rope_split: q is None exactly when there are no q heads (group 0)"
    assert positions.dtype == torch.int32 and positions.is_cuda
    assert cos.shape[1] == 128 and cos.is_contiguous() and sin.is_contiguous()
    lib = load_library()
    with torch.cuda.device(qkv.device):
        check(lib.mjv_rope_split_bf16(qkv.data_ptr(), _row_stride(qkv), _p(q), (_row_stride(q) if q is not None else 0), k.data_ptr(),
                                      _row_stride(k), cos.data_ptr(), sin.data_ptr(), positions.data_ptr(),
                                      qkv.shape[0], kv_heads, group, _stream(qkv)), "mjv_rope_split_bf16")


def rope_heads(x: torch.Tensor, n_heads: int, head_stride: int, cos: torch.Tensor, sin: torch.Tensor,
               positions: torch.Tensor) -> None:
    """Rotary embedding IN PLACE on the first ``n_heads`` heads (``head_stride`` elements apart, from column 0) of every row of
    ``x``; ``cos`` / ``sin`` [positions, rot_dim] bf16 tables (include/mjv.h, ABI 7: the Phi-3 tower's [q | k | v] projection)."""
    _chk_bf16(x, cos, sin)
    assert positions.dtype == torch.int32 and positions.is_cuda and positions.numel() >= x.shape[0]
    assert cos.is_contiguous() and sin.is_contiguous() and cos.shape == sin.shape
    assert n_heads * head_stride <= x.shape[1]
    with torch.cuda.device(x.device):
        check(load_library().mjv_rope_heads_bf16(x.data_ptr(), _row_stride(x), head_stride, n_heads, cos.shape[1], cos.data_ptr(),
                                                 sin.data_ptr(), positions.data_ptr(), x.shape[0], _stream(x)), "mjv_rope_heads_bf16")


def patchify(pixels: torch.Tensor, patches: torch.Tensor, patch: int) -> torch.Tensor:
    _chk_bf16(pixels, patches)
    assert pixels.is_contiguous() and pixels.dim() == 4 and pixels.shape[1] == 3 and pixels.shape[2] == pixels.shape[3]
    lib = load_library()
    with torch.cuda.device(patches.device):
        check(lib.mjv_patchify_bf16(pixels.data_ptr(), patches.data_ptr(), _row_stride(patches), pixels.shape[0],
                                    pixels.shape[2], patch, _stream(patches)), "mjv_patchify_bf16")
    return patches


def cls_rows(x: torch.Tensor, cls: torch.Tensor, pos0: torch.Tensor, tiles: int, tokens_per_tile: int) -> None:
    _chk_bf16(x, cls, pos0)
    lib = load_library()
    with torch.cuda.device(x.device):
        check(lib.mjv_cls_rows_bf16(x.data_ptr(), _row_stride(x), cls.data_ptr(), pos0.data_ptr(), tiles,
                                    tokens_per_tile, x.shape[1], _stream(x)), "mjv_cls_rows_bf16")


def embed_gather(ids: torch.Tensor, table: torch.Tensor, x: torch.Tensor, skip_id: int) -> None:
    _chk_bf16(table, x)
    assert ids.dtype == torch.int32 and ids.is_cuda
    lib = load_library()
    with torch.cuda.device(x.device):
        check(lib.mjv_embed_gather_bf16(ids.data_ptr(), table.data_ptr(), _row_stride(table), x.data_ptr(),
                                        _row_stride(x), ids.numel(), x.shape[1], skip_id, table.shape[0], _stream(x)),
              "mjv_embed_gather_bf16")


def reward_heads(desc: HeadsDesc, device: torch.device) -> None:
    """``device``: where the descriptor's pointers live (a descriptor carries no tensor to take the stream from)."""
    stream = torch.cuda.current_stream(device).cuda_stream
    with torch.cuda.device(device):
        check(load_library().mjv_reward_heads_bf16(C.byref(desc), stream), "mjv_reward_heads_bf16")


# ------------------------------------------------------------------------------------ profiler access
def prof_enable(on: bool) -> None:
    check(load_library().mjv_prof_enable(int(on)), "mjv_prof_enable")


def prof_filter(tag: Optional[str]) -> None:
    """Record only launches tagged ``tag`` (None: every kernel)."""
    check(load_library().mjv_prof_filter(tag.encode() if tag else None), "mjv_prof_filter")


def prof_reset() -> None:
    check(load_library().mjv_prof_reset(), "mjv_prof_reset")


def prof_results() -> dict:
    """{tag: dict(launches, ms, flops, bytes)} after synchronising the recorded events."""
    lib = load_library()
    check(lib.mjv_prof_collect(), "mjv_prof_collect")
    out = {}
    for i in range(lib.mjv_prof_count()):
        name, n = C.c_char_p(), C.c_int64()
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        check(lib.mjv_prof_get(i, C.byref(name), C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "mjv_prof_get")
        out[name.value.decode()] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)
    return out
