"""Attention on the hand-written gfx950 flash kernels (``kernels/attention_bf16.hip``).

``attention_qkv(qkv, h, hd)`` is the model's path: the fused QKV projection output
``[B, T, 3 * h * hd]`` is read in place by the forward kernel, which writes the attention output
straight into ``[B, T, h * hd]`` (the output projection's input: no head transpose) plus the
per-row log-sum-exp; the backward kernels recompute P from the LSE and write dq / dk / dv straight
into the QKV gradient layout ``[B, T, 3 * h * hd]`` (no stack / permute / copy).

``flash_attention(q, k, v)`` takes ``[B, H, T, D]`` views with any strides (contiguous head dim) —
the form the numerics tests compare against fp32 ``F.scaled_dot_product_attention``.

Grouped-query attention: ``k`` / ``v`` may carry ``Hkv`` heads, ``Hkv`` dividing ``H``; query head ``h`` reads
K / V head ``h // (H // Hkv)`` in place (no expanded copy) and the backward writes dk / dv with ``Hkv`` heads, the
sum over a group's query heads taken in fp32 inside the kernel. ``attention_qkv`` and ``attn_block`` take
``kv_heads``: the activation is then ``[B, T, (h + 2 hkv) hd]`` (``q | k | v``) and its gradient has that layout.

``split_heads(qkv, h, hd)`` remains for torch's SDPA path (CPU, other head dims): its backward
packs SDPA's dq / dk / dv into the QKV gradient layout in one HIP pass (``qkv_pack_bf16.hip``).

Packed documents (the rule; everything else refers to it). ``doc_start`` is an ``int32 [B, T]`` tensor on the inputs'
device: ``doc_start[b, t]`` is the position of the first token of the document that holds position ``t`` of row ``b``.
Valid input: ``doc_start[b, 0] == 0`` and, for every ``t``, ``doc_start[b, t]`` is ``doc_start[b, t - 1]`` or ``t``
(so it is non-decreasing and ``<= t``). The mask: query ``i`` sees key ``j`` iff ``doc_start[b, i] <= j <= i``, the
same for every head, and the same K / V head for a grouped query head. Every row sees at least itself, so no row is
empty. ``doc_start=None`` is the op as it was: same launches, same bits. ``doc_start`` requires ``causal=True``.
``doc_bounds(doc_ids)`` makes ``doc_start`` (and ``doc_end``, each key's exclusive document end, which the backward
kernels take and the ops derive themselves) from the document ids of a data loader, on the device, with no host sync.
``flash_attention``, ``attention_qkv`` and ``attn_block`` take ``doc_start=``: on the GPU the ``DOC`` instantiations of
the flash kernels, which skip the tiles outside a row's document (n equal documents per row: about 1 / n of the causal
work); on the torch path (CPU tensors, ``ops.torch_reference()``, other head dims) SDPA under the boolean mask of the
rule. A ``doc_start`` on the CPU is checked against the rule; on the GPU it is the caller's contract, as ``lens`` is
for the KV-cache kernels.

There is no silent fallback on a GPU: a kernel that rejects its arguments raises.
"""
from __future__ import annotations

import math

import torch

from . import _lib

HEAD_DIMS = (64, 128)


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def supported(qkv_or_q: torch.Tensor, head_dim: int) -> bool:
    """True when the flash kernels take this tensor (CUDA bf16, head dim 64 / 128)."""
    return qkv_or_q.is_cuda and qkv_or_q.dtype == torch.bfloat16 and head_dim in HEAD_DIMS


def _strides(*ts) -> "ctypes.Array":
    import ctypes
    vals = []
    for t in ts:
        vals += [int(t.stride(0)), int(t.stride(1)), int(t.stride(2))]
    return (ctypes.c_longlong * len(vals))(*vals)


def _check_views(*ts) -> None:
    for t in ts:
        if t.dtype != torch.bfloat16 or not t.is_cuda or t.dim() != 4 or t.stride(-1) != 1:
            raise ValueError("flash attention: bf16 CUDA [B, H, T, D] views with a contiguous head dim expected")


def check_kv_heads(h: int, hkv: int, what: str) -> None:
    """``hkv`` K / V heads for ``h`` query heads: at least one, dividing ``h``."""
    if hkv < 1 or h < 1 or h % hkv:
        raise ValueError(f"{what}: {hkv} K / V heads must be at least 1 and divide the {h} query heads")


def _kv_heads_of(q, k, v, what: str) -> int:
    H, Hkv = q.shape[1], k.shape[1]
    if k.shape != v.shape or (k.shape[0], k.shape[2], k.shape[3]) != (q.shape[0], q.shape[2], q.shape[3]):
        raise ValueError(f"{what}: k and v [B, Hkv, T, D] matching q {tuple(q.shape)} expected, got "
                         f"{tuple(k.shape)}, {tuple(v.shape)}")
    check_kv_heads(H, Hkv, what)
    return Hkv


def _doc_end(doc_start: torch.Tensor) -> torch.Tensor:
    """``doc_end[b, j]``: the exclusive end of ``j``'s document = the next document's start after ``j``, or T."""
    B, T = doc_start.shape
    ar = torch.arange(T, device=doc_start.device, dtype=torch.int32)
    nxt = torch.where(doc_start == ar, ar, T)  # a start's own position, T elsewhere
    nxt = torch.cat([nxt[:, 1:], nxt.new_full((B, 1), T)], 1)  # ... seen from the position before
    return nxt.flip(1).cummin(1).values.flip(1).contiguous()


def doc_bounds(doc_ids: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(doc_start, doc_end)``, ``int32 [B, T]`` on ``doc_ids``' device, of an int ``[B, T]`` tensor of document ids
    that change where a new document begins (the module docstring's rule). Torch ops only, no host sync."""
    if doc_ids.dim() != 2 or doc_ids.dtype.is_floating_point or doc_ids.dtype == torch.bool:
        raise ValueError(f"doc_bounds: an int [B, T] tensor of document ids expected, got {doc_ids.dtype} "
                         f"{tuple(doc_ids.shape)}")
    T = doc_ids.shape[1]
    ar = torch.arange(T, device=doc_ids.device, dtype=torch.int32)
    new = torch.ones(doc_ids.shape, dtype=torch.bool, device=doc_ids.device)
    new[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    doc_start = torch.where(new, ar, 0).cummax(1).values.to(torch.int32).contiguous()
    return doc_start, _doc_end(doc_start)


def doc_mask(doc_start: torch.Tensor) -> torch.Tensor:
    """The rule as a boolean mask ``[B, 1, T, T]`` (True: seen) for SDPA: the torch path and the tests' reference."""
    T = doc_start.shape[1]
    ar = torch.arange(T, device=doc_start.device)
    return ((ar >= doc_start[:, :, None]) & (ar <= ar[:, None])).unsqueeze(1)


def _check_doc(doc_start, B: int, T: int, device, causal: bool, what: str) -> None:
    if not causal:
        raise ValueError(f"{what}: doc_start requires causal=True (a document mask is block-diagonal causal)")
    if (not isinstance(doc_start, torch.Tensor) or doc_start.dtype != torch.int32 or doc_start.shape != (B, T)
            or doc_start.device != device or not doc_start.is_contiguous()):
        raise ValueError(f"{what}: doc_start: a contiguous int32 [{B}, {T}] tensor on {device} expected "
                         "(ops.doc_bounds makes one)")
    if not doc_start.is_cuda:  # the validity rule; on the GPU it is the caller's contract (no host sync)
        ar = torch.arange(T, dtype=torch.int32)
        if not ((doc_start[:, 0] == 0).all() and ((doc_start[:, 1:] == doc_start[:, :-1]) | (doc_start[:, 1:] == ar[1:])).all()):
            raise ValueError(f"{what}: doc_start breaks the rule: doc_start[b, 0] == 0 and doc_start[b, t] in "
                             "{doc_start[b, t - 1], t}")


def _sdpa_doc(q, k, v, doc_start, scale):
    """The torch path: SDPA under the rule's mask; grouped K / V heads expanded."""
    import torch.nn.functional as F
    G = q.shape[1] // k.shape[1]
    if G > 1:
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=doc_mask(doc_start), scale=scale)


def _torch_path(x: torch.Tensor, head_dim: int) -> bool:
    from . import native_enabled
    return not (native_enabled() and supported(x, head_dim))


def _fwd(q, k, v, o, causal: bool, scale: float, doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """q, o: [B, H, T, D] views, k, v: [B, Hkv, T, D] views (Hkv divides H). Returns lse [B, H, T] (f32).
    ``doc_start``: the packed-document forward (the module docstring's rule)."""
    B, H, T, D = q.shape
    Hkv = _kv_heads_of(q, k, v, "attn_fwd")
    lse = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
    if doc_start is not None:
        _check_doc(doc_start, B, T, q.device, causal, "attn_fwd")
        rc = _lib.lib().kfamd_attn_fwd_doc_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                doc_start.data_ptr(), B, H, Hkv, T, D, float(scale),
                                                _strides(q, k, v, o), _stream_ptr(q))
    elif Hkv == H:
        rc = _lib.lib().kfamd_attn_fwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                            B, H, T, D, float(scale), int(causal), _strides(q, k, v, o), _stream_ptr(q))
    else:
        rc = _lib.lib().kfamd_attn_fwd_gqa_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                B, H, Hkv, T, D, float(scale), int(causal), _strides(q, k, v, o),
                                                _stream_ptr(q))
    _lib.check(rc, f"attn_fwd[B={B} H={H} Hkv={Hkv} T={T} D={D}]")
    return lse


def _bwd(q, k, v, o, do, lse, dq, dk, dv, causal: bool, scale: float, group_split: int = 0,
         doc: tuple[torch.Tensor, torch.Tensor] | None = None) -> None:
    """dq [B, H, T, D], dk / dv [B, Hkv, T, D] views. ``group_split`` (grouped K / V only): how many query heads
    of a group one dK / dV workgroup sweeps, a divisor of H / Hkv; 0: the launcher's rule. ``doc``: the forward's
    ``(doc_start, _doc_end(doc_start))``."""
    B, H, T, D = q.shape
    Hkv = _kv_heads_of(q, k, v, "attn_bwd")
    if dk.shape != k.shape or dv.shape != v.shape:
        raise ValueError(f"attn_bwd: dk / dv {tuple(k.shape)} expected, got {tuple(dk.shape)}, {tuple(dv.shape)}")
    L = _lib.lib()
    if doc is not None:
        _check_doc(doc[0], B, T, q.device, causal, "attn_bwd")
        if Hkv == H:
            group_split = 0
        elif group_split < 0 or (group_split and (H // Hkv) % group_split):
            raise ValueError(f"attn_bwd: group_split={group_split} must divide the group size {H // Hkv}")
        ws = torch.empty(L.kfamd_attn_bwd_gqa_workspace(B, H, Hkv, T, D, int(group_split)), device=q.device,
                         dtype=torch.uint8)
        rc = L.kfamd_attn_bwd_doc_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(),
                                       lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(),
                                       doc[0].data_ptr(), doc[1].data_ptr(), B, H, Hkv, T, D, float(scale),
                                       int(group_split), _strides(q, k, v, o, do, dq, dk, dv), _stream_ptr(q))
    elif Hkv == H and group_split in (0, 1):
        ws = torch.empty(L.kfamd_attn_bwd_workspace(B, H, T, D), device=q.device, dtype=torch.uint8)
        rc = L.kfamd_attn_bwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(),
                                   lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), B, H, T,
                                   D, float(scale), int(causal), _strides(q, k, v, o, do, dq, dk, dv), _stream_ptr(q))
    else:
        G = H // Hkv
        if group_split < 0 or (group_split and G % group_split):
            raise ValueError(f"attn_bwd: group_split={group_split} must divide the group size {G}")
        nbytes = L.kfamd_attn_bwd_gqa_workspace(B, H, Hkv, T, D, int(group_split))
        if nbytes < 0:
            raise ValueError(f"attn_bwd: no workspace for B={B} H={H} Hkv={Hkv} T={T} D={D} group_split={group_split}")
        ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
        rc = L.kfamd_attn_bwd_gqa_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(),
                                       lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), B,
                                       H, Hkv, T, D, float(scale), int(causal), int(group_split),
                                       _strides(q, k, v, o, do, dq, dk, dv), _stream_ptr(q))
    _lib.check(rc, f"attn_bwd[B={B} H={H} Hkv={Hkv} T={T} D={D}]")


def _qkv_views(x: torch.Tensor, h: int, hkv: int, hd: int):
    """q [B, h, T, hd] and k, v [B, hkv, T, hd] views of ``x [B, T, (h + 2 hkv) hd]`` (q | k | v)."""
    B, T, _ = x.shape
    q = x[..., :h * hd].view(B, T, h, hd)
    k = x[..., h * hd:(h + hkv) * hd].view(B, T, hkv, hd)
    v = x[..., (h + hkv) * hd:].view(B, T, hkv, hd)
    return _bhtd(q), _bhtd(k), _bhtd(v)


def _bhtd(x: torch.Tensor) -> torch.Tensor:
    """[B, T, H, D] storage as a [B, H, T, D] view."""
    return x.permute(0, 2, 1, 3)


def _saved_doc(doc_start) -> tuple:
    """What a forward with ``doc_start`` saves for its backward besides: ``(doc_start, doc_end)``, else nothing."""
    return () if doc_start is None else (doc_start, _doc_end(doc_start))


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, doc_start=None):
        _check_views(q, k, v)
        B, H, T, D = q.shape
        _kv_heads_of(q, k, v, "flash_attention")
        o = _bhtd(torch.empty(B, T, H, D, device=q.device, dtype=q.dtype))
        lse = _fwd(q, k, v, o, causal, scale, doc_start)
        ctx.save_for_backward(q, k, v, o, lse, *_saved_doc(doc_start))
        ctx.causal, ctx.scale = causal, scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, *doc = ctx.saved_tensors
        B, H, T, D = q.shape
        if do.stride(-1) != 1 or any(s % 8 for s in do.stride()[:3]):
            do = do.contiguous()
        grads = [_bhtd(torch.empty(B, T, n, D, device=q.device, dtype=q.dtype)) for n in (H, k.shape[1], v.shape[1])]
        _bwd(q, k, v, o, do, lse, *grads, ctx.causal, ctx.scale, doc=tuple(doc) or None)
        return grads[0], grads[1], grads[2], None, None, None


class _FlashAttnQKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, h, hd, causal, scale, hkv, doc_start=None):
        B, T, _ = qkv.shape
        o = torch.empty(B, T, h, hd, device=qkv.device, dtype=qkv.dtype)
        lse = _fwd(*_qkv_views(qkv, h, hkv, hd), _bhtd(o), causal, scale, doc_start)
        ctx.save_for_backward(qkv, o, lse, *_saved_doc(doc_start))
        ctx.dims, ctx.causal, ctx.scale = (h, hkv, hd), causal, scale
        return o.view(B, T, h * hd)

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, *doc = ctx.saved_tensors
        h, hkv, hd = ctx.dims
        B, T, _ = qkv.shape
        do = do.contiguous().view(B, T, h, hd)
        dqkv = torch.empty_like(qkv)
        _bwd(*_qkv_views(qkv, h, hkv, hd), _bhtd(o), _bhtd(do), lse, *_qkv_views(dqkv, h, hkv, hd),
             ctx.causal, ctx.scale, doc=tuple(doc) or None)
        return dqkv, None, None, None, None, None, None


class _AttnBlock(torch.autograd.Function):
    """x -> qkv = x Wqkv^T + bqkv -> flash attention -> o Wproj^T + bproj (+ residual), one autograd
    node. Its backward orders the work across the three: the projection's dgrad, the attention
    backward, the QKV dgrad, and then both weight gradients in ONE launch (gemm.wgrad_pair: 192 + 64
    tiles at gpt-1b, where apart the QKV wgrad filled 75 % of the CUs and the projection's ran
    split-K). The forward is the separate layers' (gemm_nt with bias, _fwd, gemm_nt with bias and
    residual). ``rope`` (a rotary table, ops/rope.py): qkv is rotated in place right after its GEMM, and dqkv
    inverse-rotated in place right after the attention backward, before the bias gradient, the dgrad and the
    weight-gradient pair read it. ``hkv`` K / V heads: qkv and dqkv are ``[B, T, (h + 2 hkv) hd]`` (q | k | v)."""

    @staticmethod
    def forward(ctx, x, wqkv, bqkv, wproj, bproj, h, hd, causal, scale, residual, rope=None, hkv=None, doc_start=None):
        from .gemm import gemm_nt
        from .rope import rotate_native_
        B, T, D = x.shape
        x2 = x.reshape(B * T, D)
        if x2.stride(-1) != 1 or x2.stride(0) != D:
            x2 = x2.contiguous()
        hkv = h if hkv is None else hkv
        qkv = gemm_nt(x2, wqkv, bias=bqkv).view(B, T, (h + 2 * hkv) * hd)
        if rope is not None:
            rotate_native_(qkv, rope, h, hkv)
        o = torch.empty(B, T, h, hd, device=x.device, dtype=x.dtype)
        lse = _fwd(*_qkv_views(qkv, h, hkv, hd), _bhtd(o), causal, scale, doc_start)
        o2 = o.view(B * T, h * hd)
        res = residual.reshape(B * T, wproj.shape[0]).contiguous() if residual is not None else None
        out = gemm_nt(o2, wproj, bias=bproj, residual=res)
        ctx.save_for_backward(x2, wqkv, bqkv, wproj, bproj, qkv, o, lse, *_saved_doc(doc_start))
        ctx.dims, ctx.causal, ctx.scale, ctx.rope = (B, T, D, h, hkv, hd), causal, scale, rope
        return out.view(B, T, wproj.shape[0])

    @staticmethod
    def backward(ctx, gy):
        from .gemm import act_grad, mm, wgrad_pair
        from .rope import rotate_native_
        x2, wqkv, bqkv, wproj, bproj, qkv, o, lse, *doc = ctx.saved_tensors
        B, T, D, h, hkv, hd = ctx.dims
        ni = ctx.needs_input_grad
        gy2 = gy.reshape(B * T, wproj.shape[0])
        if not gy2.is_contiguous():
            gy2 = gy2.contiguous()

        def bias_grad(g, bias, need):
            if not need:
                return None
            _, db = act_grad(g, None, "none", True,
                             db_dtype=torch.bfloat16 if bias.dtype == torch.bfloat16 else torch.float32)
            return db.to(bias.dtype)
        gbp = bias_grad(gy2, bproj, bproj is not None and ni[4])
        o2 = o.view(B * T, h * hd)
        do = mm(gy2, wproj).view(B, T, h, hd)  # the projection's dgrad
        dqkv = torch.empty_like(qkv)
        _bwd(*_qkv_views(qkv, h, hkv, hd), _bhtd(o), _bhtd(do), lse, *_qkv_views(dqkv, h, hkv, hd),
             ctx.causal, ctx.scale, doc=tuple(doc) or None)
        if ctx.rope is not None:  # the gradient of the rotated q, k -> of the projection's output
            rotate_native_(dqkv, ctx.rope, h, hkv, inverse=True)
        dqkv2 = dqkv.view(B * T, (h + 2 * hkv) * hd)
        gbq = bias_grad(dqkv2, bqkv, bqkv is not None and ni[2])
        dx = mm(dqkv2, wqkv).view(B, T, D) if ni[0] else None
        gwq = gwp = None
        pair = wgrad_pair(dqkv2, x2, gy2, o2) if ni[1] and ni[3] else None
        if pair is not None:
            gwq, gwp = pair
        else:
            gwq = mm(dqkv2, x2, trans_a=True) if ni[1] else None
            gwp = mm(gy2, o2, trans_a=True) if ni[3] else None
        return dx, gwq, gbq, gwp, gbp, None, None, None, None, (gy if ni[9] else None), None, None, None


def attn_block(x: torch.Tensor, wqkv: torch.Tensor, bqkv: torch.Tensor | None, wproj: torch.Tensor,
               bproj: torch.Tensor | None, h: int, hd: int, residual: torch.Tensor | None = None,
               causal: bool = True, scale: float | None = None, rope: torch.Tensor | None = None,
               kv_heads: int | None = None, doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """A transformer block's attention half on the HIP kernels: ``proj(attn(qkv(x))) (+ residual)``,
    x ``[B, T, D]``, wqkv ``[3 h hd, D]`` (q | k | v rows, heads inside each), wproj ``[D_out, h hd]``.
    ``rope``: an ``ops.rope_table`` ``[max_pos >= T, hd]``; q and k are rotated (positions 0 .. T - 1) between the
    QKV projection and the attention, in place in both directions (``ops.rope_qkv``'s kernel).
    ``kv_heads``: grouped-query attention with that many K / V heads (a divisor of ``h``); wqkv is then
    ``[(h + 2 kv_heads) hd, D]`` and the flash kernels read each K / V head in place for its whole group.
    ``doc_start``: packed documents (the module docstring's rule); ``rope`` positions do not restart, which computes
    the same function (a rotated score depends on ``i - j`` alone)."""
    hkv = h if kv_heads is None else int(kv_heads)
    check_kv_heads(h, hkv, "attn_block")
    if x.dim() != 3 or wqkv.shape[0] != (h + 2 * hkv) * hd or wproj.shape[1] != h * hd:
        raise ValueError("attn_block: x [B, T, D], wqkv [(h + 2 kv_heads) hd, D] (3 h hd without kv_heads), "
                         "wproj [D_out, h hd] expected")
    if not supported(x, hd):
        raise ValueError(f"attn_block: bf16 CUDA input with head dim in {HEAD_DIMS} expected")
    if rope is not None and (rope.dim() != 2 or rope.shape[1] != hd or rope.shape[0] < x.shape[1]):
        raise ValueError(f"attn_block: rope [max_pos >= {x.shape[1]}, {hd}] expected, got {tuple(rope.shape)}")
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    if doc_start is None:
        return _AttnBlock.apply(x, wqkv, bqkv, wproj, bproj, h, hd, causal, scale, residual, rope, hkv)
    _check_doc(doc_start, x.shape[0], x.shape[1], x.device, causal, "attn_block")
    return _AttnBlock.apply(x, wqkv, bqkv, wproj, bproj, h, hd, causal, scale, residual, rope, hkv, doc_start)


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = True,
                    scale: float | None = None, doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """softmax(scale * q k^T (+ causal mask)) v for [B, H, T, D] bf16 views (D = 64 / 128). ``k`` / ``v`` may have
    ``Hkv`` heads, ``Hkv`` dividing ``H`` (grouped-query attention: query head h reads K / V head h // (H // Hkv));
    the output is ``[B, H, T, D]`` and the gradients of k / v have ``Hkv`` heads. ``doc_start``: packed documents
    (the module docstring's rule); with it, tensors off the flash kernels (CPU, ``ops.torch_reference()``, other
    head dims or dtypes) run SDPA under the rule's mask."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("flash attention: [B, H, T, D] views expected")
    _kv_heads_of(q, k, v, "flash_attention")
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if doc_start is None:
        return _FlashAttn.apply(q, k, v, causal, scale)
    _check_doc(doc_start, q.shape[0], q.shape[2], q.device, causal, "flash_attention")
    if _torch_path(q, D):
        return _sdpa_doc(q, k, v, doc_start, scale)
    return _FlashAttn.apply(q, k, v, causal, scale, doc_start)


def attention_qkv(qkv: torch.Tensor, h: int, hd: int, causal: bool = True, scale: float | None = None,
                  kv_heads: int | None = None, doc_start: torch.Tensor | None = None) -> torch.Tensor:
    """Attention of the fused QKV output ``[B, T, 3 * h * hd]`` (q | k | v, heads inside each) ->
    ``[B, T, h * hd]``, the output projection's input layout. ``kv_heads``: grouped-query attention, the activation
    is ``[B, T, (h + 2 kv_heads) * hd]`` (read in place) and so is its gradient. ``doc_start``: packed documents (the
    module docstring's rule); with it, an activation off the flash kernels runs SDPA under the rule's mask."""
    hkv = h if kv_heads is None else int(kv_heads)
    check_kv_heads(h, hkv, "attention_qkv")
    if qkv.dim() != 3 or not qkv.is_contiguous() or qkv.shape[-1] != (h + 2 * hkv) * hd:
        raise ValueError("attention_qkv: contiguous [B, T, (h + 2 * kv_heads) * hd] expected "
                         "([B, T, 3 * h * hd] without kv_heads)")
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    if doc_start is not None:
        B, T, _ = qkv.shape
        _check_doc(doc_start, B, T, qkv.device, causal, "attention_qkv")
        if _torch_path(qkv, hd):
            return _sdpa_doc(*_qkv_views(qkv, h, hkv, hd), doc_start, scale).transpose(1, 2).reshape(B, T, h * hd)
        return _FlashAttnQKV.apply(qkv, h, hd, causal, scale, hkv, doc_start)
    if not supported(qkv, hd):
        raise ValueError(f"attention_qkv: bf16 CUDA input with head dim in {HEAD_DIMS} expected")
    return _FlashAttnQKV.apply(qkv, h, hd, causal, scale, hkv)


class _SplitHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, h, hd):
        B, T, _ = qkv.shape
        ctx.dims = (B, T, h, hd)
        q, k, v = qkv.view(B, T, 3, h, hd).permute(2, 0, 3, 1, 4)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        B, T, h, hd = ctx.dims
        ref = next(g for g in (dq, dk, dv) if g is not None)
        out = torch.empty(B, T, 3 * h * hd, dtype=ref.dtype, device=ref.device)
        grads = [g if g is None or g.stride(-1) == 1 else g.contiguous() for g in (dq, dk, dv)]
        strides = []
        for g in grads:
            strides += list(g.stride()[:3]) if g is not None else [0, 0, 0]
        rc = _lib.lib().kfamd_qkv_pack_bf16(*(g.data_ptr() if g is not None else None for g in grads), out.data_ptr(),
                                           B, T, h, hd, *strides, _stream_ptr(ref))
        if rc != 0:  # off the kernel's alignment contract: autograd's own layout change
            z = [g if g is not None else torch.zeros(B, h, T, hd, dtype=ref.dtype, device=ref.device) for g in grads]
            out.view(B, T, 3, h, hd).copy_(torch.stack(z, 0).permute(1, 3, 0, 2, 4))
        return out, None, None


def split_heads(qkv: torch.Tensor, h: int, hd: int):
    """q, k, v ``[B, h, T, hd]`` views of the fused QKV output ``[B, T, 3 * h * hd]``."""
    from . import native_enabled
    if (native_enabled() and qkv.is_cuda and qkv.dtype == torch.bfloat16 and hd % 8 == 0
            and qkv.is_contiguous() and torch.is_grad_enabled() and qkv.requires_grad):
        return _SplitHeads.apply(qkv, h, hd)
    B, T, _ = qkv.shape
    q, k, v = qkv.view(B, T, 3, h, hd).permute(2, 0, 3, 1, 4)
    return q, k, v
