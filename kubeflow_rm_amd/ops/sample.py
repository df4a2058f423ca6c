"""Token sampling from a row of logits (``kernels/sample_bf16.hip``): greedy, temperature, top-k, top-p
and a stop token, with a fully specified result driven by uniforms the caller passes in as data.

The rule, per batch row with logits ``x[0..V)`` (``-inf`` allowed: never sampled; NaN or an all ``-inf`` row
is out of contract):

* Tokens are ordered by ``x`` descending, equal logits (``-0 == +0``) by token index ascending.
* ``temperature == 0`` or ``top_k == 1``: the first token of that order (lowest-index argmax); ``u`` is unused.
* Otherwise ``w_i = exp((x_i - x_max) / temperature)``. ``top_k`` keeps the first ``min(top_k, V)`` tokens of
  the order. ``top_p`` then keeps the shortest prefix of the order whose mass reaches ``top_p * Z`` (``Z``:
  the mass of the top-k set), at least one token; ``top_p == 1`` keeps the whole set. The token is the first
  kept token in token-INDEX order whose inclusive running sum of kept weights exceeds ``u * W`` (``W``: the
  kept mass); if rounding leaves none, the last kept token of non-zero weight.
* ``stop_token`` with ``done`` (int32 ``[B]``): a row whose flag is set emits ``stop_token``; any other row
  emits its token and sets its flag when that token is ``stop_token``.

On bf16 keys equal logits weigh exactly the same, so the order, the top-k set and the tie admission are
exact; only the masses carry rounding. The kernel evaluates the weights in fp32 and sums them as 64-bit
fixed-point integers (no order of additions to depend on), so it is deterministic and replays bit for bit
from a captured graph: ``u`` may be a ``[S, B]`` schedule with a device ``step`` counter that selects the
row, the kernel writes ``out`` (and column ``step`` of ``seq``), and the caller advances ``step``.

On CPU tensors and under ``ops.torch_reference()`` the same rule runs in plain torch in fp64: that form is
the reference. On a GPU there is no fallback: a tensor the kernel rejects raises.
"""
from __future__ import annotations

import torch

from . import _lib

MAX_V = 1 << 20


def _native(t: torch.Tensor) -> bool:
    from . import native_enabled
    return t.is_cuda and native_enabled()


def _first_true(mask: torch.Tensor) -> torch.Tensor:
    """Lowest index of a True per row (V where there is none)."""
    V = mask.shape[-1]
    idx = torch.arange(V, device=mask.device).expand_as(mask)
    return torch.where(mask, idx, torch.full_like(idx, V)).min(-1).values


def kept_weights(logits: torch.Tensor, temperature: float, top_k: int | None, top_p: float | None) -> torch.Tensor:
    """fp64 ``[B, V]``: ``w_i`` of the rule for every kept token, 0 for the others (the reference kept set;
    a kept ``-inf`` token also has weight 0 and is never drawn)."""
    x = logits.double()
    V = x.shape[-1]
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices  # ties: index ascending
    xs = x.gather(-1, order)
    w = torch.exp((xs - xs[:, :1]) / float(temperature))
    keep = torch.ones_like(w, dtype=torch.bool)
    if top_k is not None and top_k < V:
        keep[:, top_k:] = False
    w = w * keep
    if top_p is not None and top_p < 1.0:
        before = w.cumsum(-1) - w  # the mass of the strictly earlier tokens
        prefix = before < float(top_p) * w.sum(-1, keepdim=True)
        prefix[:, 0] = True
        w = w * prefix
    return torch.zeros_like(w).scatter_(-1, order, w)


def _sample_torch(logits, u, temperature, top_k, top_p):
    x = logits.double()
    if temperature == 0 or top_k == 1:
        return _first_true(x == x.max(-1, keepdim=True).values)
    wk = kept_weights(logits, temperature, top_k, top_p)
    run = wk.cumsum(-1)
    live = wk > 0
    tok = _first_true(live & (run > u.double().unsqueeze(-1) * wk.sum(-1, keepdim=True)))
    V = x.shape[-1]
    last = V - 1 - _first_true(live.flip(-1))
    return torch.where(tok < V, tok, last)


def sample(logits: torch.Tensor, u: torch.Tensor, temperature: float = 1.0, top_k: int | None = None,
           top_p: float | None = None, *, step: torch.Tensor | None = None, out: torch.Tensor | None = None,
           seq: torch.Tensor | None = None, done: torch.Tensor | None = None,
           stop_token: int | None = None) -> torch.Tensor:
    """One token per row of ``logits [B, V]`` -> int64 ``[B]`` by the module's rule.

    ``u``: fp32 uniforms in [0, 1), ``[B]``, or a schedule ``[S, B]`` with ``step`` (an int32 tensor of one
    element on the logits' device) selecting row ``u[step]``. ``out``: optional int64 ``[B]`` to write.
    ``seq``: optional int64 ``[B, >= S]`` whose column ``step`` also receives the tokens. ``stop_token``
    needs ``done`` (int32 ``[B]``, read and updated in place) and the other way round. Nothing here advances
    ``step``: the caller does (``step.add_(1)``), as with ``KVCache.lens``.

    On a GPU: bf16 logits with a contiguous last dimension (any row stride, no alignment), V <= 2^20."""
    if logits.dim() != 2:
        raise ValueError(f"sample: logits [B, V] expected, got {tuple(logits.shape)}")
    B, V = logits.shape
    if B < 1 or V < 1:
        raise ValueError("sample: at least one row and one token expected")
    temperature = float(temperature)
    if not temperature >= 0.0 or temperature == float("inf"):
        raise ValueError(f"sample: a finite temperature >= 0 expected, got {temperature}")
    if top_k is not None and int(top_k) < 1:
        raise ValueError(f"sample: top_k >= 1 expected, got {top_k}")
    top_k = None if top_k is None else int(top_k)
    if top_p is not None and not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"sample: 0 < top_p <= 1 expected, got {top_p}")
    top_p = None if top_p is None else float(top_p)
    if (stop_token is None) != (done is None):
        raise ValueError("sample: stop_token and done go together")
    if stop_token is not None and not 0 <= int(stop_token) < V:
        raise ValueError(f"sample: stop_token in [0, {V}) expected, got {stop_token}")
    if u.dtype != torch.float32 or u.device != logits.device or u.dim() not in (1, 2) or u.shape[-1] != B \
            or not u.is_contiguous():
        raise ValueError(f"sample: u must be a contiguous fp32 [{B}] or [S, {B}] tensor on the logits' device")
    S = 1 if u.dim() == 1 else u.shape[0]
    if step is None:
        if S != 1:
            raise ValueError("sample: a [S, B] schedule of uniforms needs step")
    elif step.dtype != torch.int32 or step.numel() != 1 or step.device != logits.device:
        raise ValueError("sample: step must be an int32 tensor of one element on the logits' device")
    for name, t, shape in (("out", out, (B,)), ("done", done, (B,))):
        want = torch.int64 if name == "out" else torch.int32
        if t is not None and (tuple(t.shape) != shape or t.dtype != want or t.device != logits.device
                              or not t.is_contiguous()):
            raise ValueError(f"sample: {name} must be a contiguous {want} [{B}] tensor on the logits' device")
    if seq is not None and (seq.dim() != 2 or seq.shape[0] != B or seq.shape[1] < S or seq.dtype != torch.int64
                            or seq.device != logits.device or (seq.shape[1] > 1 and seq.stride(1) != 1)):
        raise ValueError(f"sample: seq must be an int64 [{B}, >= {S}] tensor (contiguous rows) on the logits' device")

    if not _native(logits):
        s = 0 if step is None else int(step.item())
        if not 0 <= s < S:
            raise ValueError(f"sample: step {s} outside the schedule of {S} rows")
        tok = _sample_torch(logits, u.view(S, B)[s], temperature, top_k, top_p)
        if done is not None:
            tok = torch.where(done != 0, torch.full_like(tok, int(stop_token)), tok)
            done.copy_((tok == int(stop_token)).to(done.dtype))
        if out is not None:
            tok = out.copy_(tok)
        if seq is not None:
            seq[:, s] = tok
        return tok

    if logits.dtype != torch.bfloat16 or (V > 1 and logits.stride(1) != 1):
        raise ValueError("sample: bf16 logits with a contiguous last dimension expected on a GPU")
    if V > MAX_V:
        raise ValueError(f"sample: V <= {MAX_V} expected on a GPU, got {V}")
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=logits.device)
    rc = _lib.lib().kfamd_sample_bf16(
        logits.data_ptr(), logits.stride(0), u.data_ptr(), step.data_ptr() if step is not None else None,
        out.data_ptr(), seq.data_ptr() if seq is not None else None, seq.stride(0) if seq is not None else 0,
        done.data_ptr() if done is not None else None, B, V, S, 0.0 if temperature == 0 else 1.0 / temperature,
        top_k or 0, 1.0 if top_p is None else top_p, -1 if stop_token is None else int(stop_token),
        torch.cuda.current_stream(logits.device).cuda_stream)
    _lib.check(rc, f"sample[B={B} V={V} S={S} top_k={top_k} top_p={top_p}]")
    return out
