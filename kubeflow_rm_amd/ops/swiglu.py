"""SwiGLU: the gated MLP activation of the Llama family, and the one place its layout rule is stated.

The rule
--------
* The up-projection weight is ``fc1.weight [2F, d_model]`` with ``F = cfg.d_ff``.
* Its rows are INTERLEAVED: row ``2j`` is gate ``j``, row ``2j + 1`` is up ``j``. The bias is ``[2F]`` in the same
  order (and so are an 8-bit weight's row scales).
* With ``z = x @ W1.T + b1`` (``[..., 2F]``), the output is ``h[..., j] = silu(z[..., 2j]) * z[..., 2j + 1]`` with
  ``silu(v) = v / (1 + exp(-v))``, computed in fp32 and rounded once.

Why interleaved and not stacked ``[gate; up]``: a (gate, up) pair then sits in the same wave / 8-row tile of the
weight-streaming GEMMs (``kernels/gemm_skinny_bf16.hip``, ``gemm_skinny_w8.hip``), so the gate is their epilogue;
it sits in adjacent C columns for any later large-GEMM epilogue; and a contiguous column-parallel shard of ``fc1``
keeps whole pairs, so tensor parallelism needs no special sharding (``fc2``'s row shard matches).
Checkpoints that store two matrices go through ``swiglu_interleave`` / ``swiglu_deinterleave``.

Where it runs: ``gemm_nt(..., act="swiglu", variant="skinny*")`` is the one-launch gated GEMM for up to 16 rows;
``swiglu(z)`` is the elementwise pass (``kernels/swiglu_bf16.hip``) for more rows and for training, with its own
backward kernel. CPU tensors, and GPU tensors inside ``ops.torch_reference()``, compute the rule in torch.
"""
from __future__ import annotations

import torch

from . import _lib


def swiglu_interleave(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """Two ``[F, ...]`` tensors (weights ``[F, K]`` or biases ``[F]``) -> the interleaved ``[2F, ...]`` one."""
    if gate.shape != up.shape or gate.dim() < 1:
        raise ValueError(f"swiglu_interleave: two tensors of one shape [F, ...] expected, got {tuple(gate.shape)} and "
                         f"{tuple(up.shape)}")
    return torch.stack((gate, up), dim=1).reshape(2 * gate.shape[0], *gate.shape[1:])


def swiglu_deinterleave(w: torch.Tensor):
    """The inverse of ``swiglu_interleave``: ``(gate, up)``, each ``[F, ...]`` (views of ``w``)."""
    if w.dim() < 1 or w.shape[0] % 2:
        raise ValueError(f"swiglu_deinterleave: an even leading dimension expected, got {tuple(w.shape)}")
    return w[0::2], w[1::2]


def swiglu_reference(z: torch.Tensor) -> torch.Tensor:
    """The rule in torch: fp32 arithmetic, the result in ``z``'s dtype. Differentiable."""
    if z.shape[-1] % 2:
        raise ValueError(f"swiglu: an even last dimension [.., 2F] expected, got {tuple(z.shape)}")
    zf = z.float()
    g, u = zf[..., 0::2], zf[..., 1::2]
    return (g / (1.0 + torch.exp(-g)) * u).to(z.dtype)


def _native(z: torch.Tensor) -> bool:
    from . import native_enabled
    return z.is_cuda and native_enabled()


def _rows(t: torch.Tensor, what: str) -> torch.Tensor:
    """``t`` as ``[rows, cols]`` with a unit inner stride, without a copy where its layout allows (a strided
    2-D view keeps its row stride)."""
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{what} must be bfloat16, got {t.dtype}")
    if t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):  # no overlapping rows
        return t
    return t.reshape(-1, t.shape[-1]).contiguous() if not t.is_contiguous() else t.view(-1, t.shape[-1])


def swiglu_fwd(z: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``kfamd_swiglu_fwd_bf16``: ``z [..., 2F]`` bf16 on the GPU -> ``h [..., F]``. A 2-D ``z`` / ``out`` may be
    row-strided views."""
    if z.shape[-1] % 2 or z.shape[-1] < 2:
        raise ValueError(f"swiglu: an even last dimension [.., 2F] expected, got {tuple(z.shape)}")
    if not z.is_cuda:
        raise ValueError("swiglu_fwd: a GPU tensor expected")
    F = z.shape[-1] // 2
    z2 = _rows(z, "z")
    rows = z2.shape[0]
    if out is None:
        out = torch.empty(*z.shape[:-1], F, dtype=torch.bfloat16, device=z.device)
    elif tuple(out.shape) != (*z.shape[:-1], F) or out.device != z.device:
        raise ValueError(f"swiglu: out {(*z.shape[:-1], F)} on {z.device} expected, got {tuple(out.shape)}")
    o2 = _rows(out, "out")
    if o2.data_ptr() != out.data_ptr():
        raise ValueError("swiglu: out must have a contiguous last dimension and uniform rows")
    if rows:
        rc = _lib.lib().kfamd_swiglu_fwd_bf16(z2.data_ptr(), o2.data_ptr(), rows, F, z2.stride(0), o2.stride(0),
                                              torch.cuda.current_stream(z.device).cuda_stream)
        _lib.check(rc, f"swiglu_fwd[{rows}x{F}]")
    return out


def swiglu_bwd(dh: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """``kfamd_swiglu_bwd_bf16``: ``dz [..., 2F]`` (contiguous) from ``dh [..., F]`` and the forward's ``z``."""
    F = z.shape[-1] // 2
    z2, d2 = _rows(z, "z"), _rows(dh.to(torch.bfloat16), "dh")
    rows = z2.shape[0]
    dz = torch.empty(*z.shape, dtype=torch.bfloat16, device=z.device)
    if rows:
        rc = _lib.lib().kfamd_swiglu_bwd_bf16(d2.data_ptr(), z2.data_ptr(), dz.data_ptr(), rows, F, d2.stride(0),
                                              z2.stride(0), 2 * F, torch.cuda.current_stream(z.device).cuda_stream)
        _lib.check(rc, f"swiglu_bwd[{rows}x{F}]")
    return dz


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return swiglu_fwd(z)

    @staticmethod
    def backward(ctx, dh):
        (z,) = ctx.saved_tensors
        return swiglu_bwd(dh, z)


def swiglu(z: torch.Tensor) -> torch.Tensor:
    """Autograd-aware ``h[..., j] = silu(z[..., 2j]) * z[..., 2j + 1]`` over an interleaved ``z [..., 2F]``: the two
    HIP kernels on a bf16 GPU tensor, the torch rule on CPU tensors and inside ``ops.torch_reference()``."""
    if not _native(z):
        return swiglu_reference(z)
    return _SwiGLU.apply(z)
