"""Rotary position embeddings (RoPE) on a fused QKV activation (``kernels/rope_bf16.hip``).

The rule, which the kernels and the torch path both implement:

**Table.** ``rope_table(max_pos, D, theta)`` is fp32 ``[max_pos, D]``; row ``p`` is
``cos(p f_0 .. p f_{D/2-1}) | sin(p f_0 .. p f_{D/2-1})`` with ``f_i = theta ** (-2 i / D)``, computed in float64 on
the host and rounded once to fp32. The GPU kernels and the CPU reference read the same table; no kernel calls
``sin`` or ``cos``.

**Pairing.** Rotate-half (the Hugging Face Llama / NeoX convention). For ``i < D/2`` at position ``p``, with
``c = table[p, i]`` and ``s = table[p, D/2 + i]``::

    y[i]       = x[i] * c - x[i + D/2] * s
    y[i + D/2] = x[i + D/2] * c + x[i] * s

**Arithmetic.** The inputs are widened to fp32; the two products and the add or subtract are each rounded on
their own (no FMA contraction: the kernels switch it off, and torch's fp32 ops never contract); the result is
rounded once to the activation's dtype (bf16 on the GPU: round-to-nearest-even). The kernels therefore equal the
torch form on the same table bit for bit.

**Inverse.** The backward of the map is the same map with ``s -> -s``, passed as a sign; negation is exact.

**What is rotated.** The whole head dimension of every q and k head; v is untouched. No partial rotary, no
frequency scaling.

**Positions.** Row ``(b, t)`` of the activation is at position ``(positions[b] if given else 0) + t``. A row whose
position is at or beyond the table's row count is left as it is (and the table is not read for it).

``rope_qkv`` is the standalone rotation (an autograd function; in place on the GPU). ``ops.kv_append(...,
rope=table)`` is the fused rotate-and-append of the KV-cache steps, ``ops.attn_block(..., rope=table)`` the training
block's form.
"""
from __future__ import annotations

import torch

from . import _lib

HEAD_DIMS = (64, 128)  # what the kernels take


def rope_table(max_pos: int, D: int, theta: float = 10000.0, device=None) -> torch.Tensor:
    """The fp32 ``[max_pos, D]`` table of the rule above: float64 on the host, rounded once."""
    if max_pos < 1 or D < 2 or D % 2:
        raise ValueError(f"rope_table: max_pos >= 1 and an even head dim expected, got {max_pos}, {D}")
    f = float(theta) ** (-2.0 * torch.arange(D // 2, dtype=torch.float64) / D)
    ang = torch.arange(max_pos, dtype=torch.float64).unsqueeze(1) * f.unsqueeze(0)
    return torch.cat([ang.cos(), ang.sin()], 1).to(torch.float32).to(device=device)


def _check(qkv, table, q_heads: int, kv_heads: int) -> int:
    if table.dim() != 2 or table.dtype != torch.float32 or table.shape[1] % 2:
        raise ValueError("rope: an fp32 [max_pos, D] table expected (ops.rope_table)")
    D = table.shape[1]
    if qkv.dim() != 3 or q_heads < 1 or kv_heads < 1 or qkv.shape[2] != (q_heads + 2 * kv_heads) * D:
        raise ValueError(f"rope: qkv [B, T, {(q_heads + 2 * kv_heads) * D}] expected, got {tuple(qkv.shape)}")
    if table.device != qkv.device:
        raise ValueError("rope: the table must live on the activation's device")
    return D


def rotate_torch(qkv: torch.Tensor, table: torch.Tensor, q_heads: int, kv_heads: int,
                 positions: torch.Tensor | None = None, inverse: bool = False) -> torch.Tensor:
    """The rule in torch fp32 ops, out of place: a new tensor of qkv's dtype with the q and k head slices rotated
    (``inverse``: by the inverse rotation) and the v slice copied."""
    D = _check(qkv, table, q_heads, kv_heads)
    B, T, _ = qkv.shape
    nr = (q_heads + kv_heads) * D
    pos = torch.arange(T, device=qkv.device).unsqueeze(0).expand(B, T)
    if positions is not None:
        pos = pos + positions.to(device=qkv.device, dtype=torch.long).view(B, 1)
    live = (pos >= 0) & (pos < table.shape[0])
    rows = table[pos.clamp(0, table.shape[0] - 1)]  # [B, T, D]
    c, s = rows[..., :D // 2].unsqueeze(2), rows[..., D // 2:].unsqueeze(2)  # [B, T, 1, D/2]
    if inverse:
        s = -s
    x = qkv[..., :nr].reshape(B, T, q_heads + kv_heads, D).float()
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(qkv.dtype).view(B, T, nr)
    y = torch.where(live.unsqueeze(-1), y, qkv[..., :nr])
    return torch.cat([y, qkv[..., nr:]], -1)


def rotate_native_(qkv: torch.Tensor, table: torch.Tensor, q_heads: int, kv_heads: int,
                   positions: torch.Tensor | None = None, inverse: bool = False) -> torch.Tensor:
    """``kfamd_rope_qkv_bf16`` on ``qkv`` IN PLACE (bf16 GPU ``[B, T, (Hq + 2 Hkv) D]``, contiguous last dim, any
    16-B aligned b / t strides). No fallback: a shape the kernel rejects raises."""
    D = _check(qkv, table, q_heads, kv_heads)
    if D not in HEAD_DIMS:
        raise ValueError(f"rope: head dim in {HEAD_DIMS} expected on a GPU, got {D}")
    if qkv.dtype != torch.bfloat16 or qkv.stride(2) != 1 or not table.is_contiguous():
        raise ValueError("rope: bf16 qkv with a contiguous last dim and a contiguous table expected")
    B, T, _ = qkv.shape
    if positions is not None and (positions.dtype != torch.int32 or positions.device != qkv.device
                                  or positions.numel() != B or not positions.is_contiguous()):
        raise ValueError("rope: positions must be a device int32 [B] tensor")
    rc = _lib.lib().kfamd_rope_qkv_bf16(qkv.data_ptr(), table.data_ptr(),
                                        positions.data_ptr() if positions is not None else None, table.shape[0], B, T,
                                        q_heads, kv_heads, D, qkv.stride(0), qkv.stride(1), int(inverse),
                                        torch.cuda.current_stream(qkv.device).cuda_stream)
    _lib.check(rc, f"rope_qkv[B={B} T={T} Hq={q_heads} Hkv={kv_heads} D={D}]")
    return qkv


def _native(t: torch.Tensor) -> bool:
    from . import native_enabled
    return t.is_cuda and native_enabled()


class _RopeQKV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, q_heads, kv_heads, positions, inplace):
        ctx.args = (table, q_heads, kv_heads, positions)
        if _native(qkv):
            if inplace:
                ctx.mark_dirty(qkv)
                return rotate_native_(qkv, table, q_heads, kv_heads, positions)
            return rotate_native_(qkv.clone(), table, q_heads, kv_heads, positions)
        return rotate_torch(qkv, table, q_heads, kv_heads, positions)

    @staticmethod
    def backward(ctx, g):
        table, q_heads, kv_heads, positions = ctx.args
        if _native(g):  # the incoming gradient is this node's alone only as a copy
            g = rotate_native_(g.clone(memory_format=torch.contiguous_format), table, q_heads, kv_heads, positions,
                               inverse=True)
        else:
            g = rotate_torch(g, table, q_heads, kv_heads, positions, inverse=True)
        return g, None, None, None, None, None


def rope_qkv(qkv: torch.Tensor, table: torch.Tensor, q_heads: int, kv_heads: int,
             positions: torch.Tensor | None = None) -> torch.Tensor:
    """Rotate the q and k head slices of the fused activation ``qkv [B, T, (q_heads + 2 kv_heads) * D]`` (``q | k |
    v``) by ``table`` (``rope_table``; D is its width); v is untouched. ``positions``: int32 ``[B]`` on the
    activation's device, the position of each row's first token (default 0).

    On the GPU kernels (bf16, D = 64 / 128) the rotation is IN PLACE: ``qkv`` itself is rotated and returned
    (``mark_dirty``). That is sound for the output of ``ops.linear`` / ``ops.gemm_nt`` without an activation, whose
    backward saves its input and weight and not its output; a producer that did save its output makes autograd
    raise at backward. A leaf that requires grad is rotated out of place. On CPU tensors and under
    ``ops.torch_reference()`` the same rule runs in torch fp32 ops, out of place. Backward: the inverse rotation
    of the gradient's q and k slices; the v gradient passes through."""
    inplace = not (qkv.requires_grad and qkv.is_leaf)
    return _RopeQKV.apply(qkv, table, int(q_heads), int(kv_heads), positions, inplace)
