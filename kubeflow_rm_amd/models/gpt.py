"""GPT-style decoder LM built on the framework's gfx950 ops — the in-notebook workload.

Used by the multi-GPU notebook smoke (BASELINE config 4: DP/TP over RCCL inside a pod), the
examples and ``smoke()``. Every projection runs on the hand-written MFMA GEMM with its fused
epilogue (bias + GELU for the MLP up-projection; residual for the down-projection), LayerNorm
on the wave-per-row kernel, the LM-head loss on the bf16 cross-entropy kernel, causal attention on
the hand-written flash kernels (``ops.attention_qkv``: reads the fused QKV output in place, writes
the output projection's input layout; head dims 64 / 128). Other head dims and the torch reference
mode use ``scaled_dot_product_attention``.
With a tensor-parallel group the attention heads and the MLP are split Megatron-style
(QKV / fc1 column-parallel, out-proj / fc2 row-parallel: one all-reduce per sub-block).

On CPU tensors the same module runs torch's reference ops (used by the gloo tests).

Sampling: ``GPT.generate`` (``prefill`` + ``decode_step`` over an ``ops.KVCache``) runs each new token
on the decode kernels — the M <= 16 weight-streaming GEMM, the KV append and split-KV single-query
attention — and can replay the step as one hipGraph (no tensor-parallel group; head dims 64 / 128).
``GPT.decode_weights()`` / ``generate(weight_dtype=torch.float8_e4m3fn)`` run the steps of up to 16 rows on
8-bit copies of the projection weights (W8A16: bf16 activations, fp32 accumulation).
``generate(sampler="fused")`` samples on ``ops.sample`` (top-k, top-p, a stop token; seeded uniforms, so the
result does not depend on the device) and with ``graph=True`` replays step + sampler + token feedback as
one hipGraph per token.

Grouped-query attention: ``GPTConfig(n_kv_heads=Hkv)`` with ``Hkv`` dividing ``n_heads`` gives every group of
``G = n_heads // Hkv`` query heads one K / V head (query head h reads K / V head ``h // G``); the fused QKV
projection then has ``(n_heads + 2 * Hkv) * head_dim`` features, ``q | k | v``. The KV cache holds the ``Hkv``
heads (1 / G of the bytes) and the decode / extend / chunk kernels stream K / V once per group. Training and
``prefill`` run the flash kernels on the ``Hkv`` K / V heads in place (``ops.attn_block(kv_heads=...)`` on the fused
single-rank path, ``ops.attention_qkv(kv_heads=...)`` on the others and in ``prefill``): no expanded copy, dq / dk /
dv written straight into the ``(n_heads + 2 * Hkv) * head_dim`` QKV gradient, dK / dV summed over a group in fp32
inside the kernel, for any ``G`` dividing ``n_heads``. Tensor-parallel K / V head sharding and, on the KV-cache
kernels, group sizes outside {1, 2, 4, 8, 16} are not built.

Rotary position embeddings: ``GPTConfig(pos="rope", rope_theta=...)`` drops the learned position table (no ``pos``
parameter, nothing of it in ``state_dict()``) and rotates q and k instead (rotate-half over the whole head dim; the
rule is the docstring of ``ops/rope.py``), from one non-persistent fp32 buffer ``rope_table [max_seq, head_dim]``.
Training rotates inside ``ops.attn_block(rope=...)`` on the fused path and with ``ops.rope_qkv`` on the others;
``prefill`` / ``decode_step`` / ``extend`` rotate inside their one ``ops.kv_append(..., rope=...)`` per layer, at
positions read from the device-side ``cache.lens``: K is stored rotated, the step stays capturable and launches
no more kernels than with learned positions. ``pos="learned"`` (the default) is the model as it was. Not built:
partial rotary, scaled rotary (NTK / YaRN), and a rotation fused into the flash kernel's Q / K loads.

Llama-style blocks: ``GPTConfig(norm="rms", mlp="swiglu")``. ``norm="rms"`` makes ``ln1`` / ``ln2`` / ``ln_f`` RMSNorms
(a ``weight`` only: no norm bias in ``state_dict()``; ``norm_eps`` defaults to the op's 1e-6) on
``ops.rms_norm_residual`` / ``kfamd_rmsnorm_fwd_bf16``. ``mlp="swiglu"`` makes ``fc1`` a ``[2 * d_ff, d_model]``
projection whose rows are interleaved gate / up (the rule is the docstring of ``ops/swiglu.py``;
``ops.swiglu_interleave`` packs a checkpoint's two matrices) and the MLP ``fc2(silu(gate) * up)``: training and steps of
more than 16 rows run ``linear -> ops.swiglu -> fc2``, the KV-cache steps of up to 16 rows run the gated
weight-streaming GEMM (``ops.gemm_nt(act="swiglu")``), one launch as the GELU up-projection has, on the bf16 or the
``decode_weights()`` copy of ``fc1`` (quantised row by row, so a pair keeps its two scales). Everything above (GQA,
rotary, FP8 cache / weights, graphs, the fused sampler, drafting, chunked prefill, tensor parallelism: a contiguous
column shard of ``fc1`` keeps whole pairs) takes the configured norm and MLP. The defaults ``norm="layer"``,
``mlp="gelu"`` are the model as it was: same parameters, same state dict, same launches. Not built: bias-free linears
(the biases stay, zero-initialised: a bias-free checkpoint loads with ``strict=False`` and leaves them at zero), GEGLU
or any other gate, and a GLU epilogue in the large (more than 16 rows) GEMM.

Sliding-window attention: ``GPTConfig(window=W)`` gives every layer a local causal mask: a position sees itself and the
``W - 1`` positions before it (the rule is the docstring of ``ops/decode.py``; Mistral's ``q_pos - k_pos < W``).
``decode_step`` / ``extend`` / ``extend(chunk=N)`` pass ``window`` to ``ops.attention_decode`` / ``attention_extend`` /
``attention_chunk`` and are otherwise unchanged (capturable as before; GQA, rotary, FP8 cache and weights, the fused
sampler, ``prefill_chunk`` and ``draft=``, which may have its own window or none, compose by shapes only). ``prefill``
on the GPU cannot use the flash kernel, which has no window: it runs the prompt over the cache on
``ops.attention_chunk`` in one step (its docstring). The training ``forward`` applies the mask on the torch path (CPU,
``ops.torch_reference()``) and raises ``NotImplementedError`` on the native GPU path. A flat ``KVCache`` still holds
every position (the ring below does not). ``window=None`` (the default) is the model as it was: same launches, same
bits. Not built: a window in the flash forward / backward kernels (native GPU training of a windowed model), per-layer
windows, attention sinks.

Ring-buffer cache: ``new_cache(..., ring=True)`` / ``generate(..., ring=True)`` of a windowed model keep the last
``capacity`` positions only (``ops/decode.py``'s ring rule): the cache's memory is O(window), the positions run to
``max_seq``, and ``decode_step``, ``extend``, ``extend(chunk=N)`` and the graphed steps run on it with a launch grid that
depends on the window and the step's token count alone (no ``pin_bound``). A step of T tokens needs ``window + T - 1 <=
capacity``. Not built: a ring without a window, a capacity that is no multiple of 256, tensor-parallel sharding of a
ring.

Paged cache: ``new_cache(..., paged=True)`` / ``generate(..., paged=True)`` keep the K / V rows in pages of an
``ops.PagePool`` (``ops/decode.py``'s page rule): memory follows the tokens held, caches on one pool share it, and
``generate(num_samples=S)`` prefills a prompt once and forks it S ways, the samples sharing the prompt's full pages.
The steps call ``cache.reserve`` themselves; the logits equal a flat cache's bit for bit. Not built: paged with a
window or a ring, with ``draft=``, or with a tensor-parallel group that issues collectives.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from kubeflow_rm_amd import ops
from kubeflow_rm_amd.parallel import tp as tpl


@dataclass
class GPTConfig:
    vocab_size: int = 32000
    d_model: int = 1024
    n_layers: int = 12
    n_heads: int = 16
    d_ff: int = 4096
    max_seq: int = 2048
    dropout: float = 0.0
    dtype: torch.dtype = torch.bfloat16
    n_kv_heads: int | None = None  # K / V heads (grouped-query attention); None: n_heads
    pos: str = "learned"  # "learned": a [max_seq, d_model] table added to the embedding; "rope": rotary q / k
    rope_theta: float = 10000.0  # the rotary base (pos="rope")
    norm: str = "layer"  # "layer": LayerNorm (weight + bias); "rms": RMSNorm (weight only)
    mlp: str = "gelu"  # "gelu": fc2(gelu_tanh(fc1 x)); "swiglu": fc1 [2 d_ff, d_model] interleaved gate / up (ops/swiglu.py)
    norm_eps: float | None = None  # None: the ops' defaults, 1e-5 (LayerNorm) / 1e-6 (RMSNorm)
    window: int | None = None  # sliding-window attention: a position sees itself and the window - 1 before it; None: all

    def __post_init__(self):
        if self.window is not None and (isinstance(self.window, bool) or not isinstance(self.window, int)
                                        or self.window < 1):
            raise ValueError(f"window={self.window!r}: None or an int >= 1 expected")
        if self.norm not in ("layer", "rms"):
            raise ValueError(f'norm={self.norm!r}: "layer" or "rms" expected')
        if self.mlp not in ("gelu", "swiglu"):
            raise ValueError(f'mlp={self.mlp!r}: "gelu" or "swiglu" expected')
        if self.norm_eps is not None and not self.norm_eps > 0:
            raise ValueError(f"norm_eps={self.norm_eps!r}: None or a positive number expected")
        if self.pos not in ("learned", "rope"):
            raise ValueError(f'pos={self.pos!r}: "learned" or "rope" expected')
        if self.pos == "rope" and (self.d_model // self.n_heads) % 2:
            raise ValueError(f"pos=\"rope\" needs an even head dim, got {self.d_model // self.n_heads}")
        if self.n_kv_heads is not None and (self.n_kv_heads < 1 or self.n_heads % self.n_kv_heads):
            raise ValueError(f"n_kv_heads={self.n_kv_heads} must divide n_heads={self.n_heads}")

    @property
    def head_dim(self) -> int:
        return self.d_model // self.n_heads

    @property
    def kv_heads(self) -> int:
        return self.n_heads if self.n_kv_heads is None else self.n_kv_heads

    @property
    def eps(self) -> float:
        return self.norm_eps if self.norm_eps is not None else (1e-6 if self.norm == "rms" else 1e-5)


CONFIGS = {
    "gpt-tiny": GPTConfig(vocab_size=512, d_model=256, n_layers=2, n_heads=4, d_ff=1024, max_seq=256),
    "gpt-small": GPTConfig(vocab_size=32000, d_model=768, n_layers=12, n_heads=12, d_ff=3072, max_seq=2048),
    "gpt-1b": GPTConfig(vocab_size=32000, d_model=2048, n_layers=24, n_heads=16, d_ff=8192, max_seq=4096),
}


def _layer_norm(x, w, b, eps=1e-5):
    if x.is_cuda:
        from kubeflow_rm_amd import ops
        if ops.native_enabled():
            return ops.layer_norm(x, w, b, eps)
        return F.layer_norm(x, (x.shape[-1],), w, b, eps)
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def _cross_entropy(logits, targets):
    if logits.is_cuda:
        from kubeflow_rm_amd import ops
        if ops.native_enabled():
            return ops.cross_entropy(logits, targets)  # bf16 logits, no fp32 copy
    return F.cross_entropy(logits.float().view(-1, logits.shape[-1]), targets.reshape(-1))


class LayerNorm(torch.nn.Module):
    def __init__(self, d, dtype, device=None, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(d, dtype=dtype, device=device))
        self.bias = torch.nn.Parameter(torch.zeros(d, dtype=dtype, device=device))

    def forward(self, x):
        return _layer_norm(x, self.weight, self.bias, self.eps)

    def with_residual(self, x):
        """(LayerNorm(x), r) with r = x for the block's residual add: on the HIP path the two gradient
        contributions to x are summed inside the LayerNorm backward kernel (no separate add)."""
        if x.is_cuda:
            from kubeflow_rm_amd import ops
            if ops.native_enabled():
                return ops.layer_norm_residual(x, self.weight, self.bias, self.eps)
        return self(x), x

    def fwd(self, x):
        """The no-grad forward of the KV-cache steps on the HIP kernel (GPU, bf16)."""
        return ops.layer_norm_fwd(x, self.weight, self.bias, self.eps)[0]


def _rms_norm_torch(x, w, eps):
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()).to(x.dtype)


class RMSNorm(torch.nn.Module):
    """``GPTConfig(norm="rms")``: y = x * rsqrt(mean(x^2) + eps) * weight. A ``weight`` only (no ``bias`` key in the
    state dict); the same GPU / CPU pattern as ``LayerNorm``."""

    def __init__(self, d, dtype, device=None, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(d, dtype=dtype, device=device))

    def forward(self, x):
        if x.is_cuda and ops.native_enabled():
            return ops.rms_norm(x, self.weight, self.eps)
        return _rms_norm_torch(x, self.weight, self.eps)

    def with_residual(self, x):
        """(RMSNorm(x), r) with r = x for the block's residual add, as ``LayerNorm.with_residual``."""
        if x.is_cuda and ops.native_enabled():
            return ops.rms_norm_residual(x, self.weight, self.eps)
        return self(x), x

    def fwd(self, x):
        return ops.rms_norm_fwd(x, self.weight, self.eps)[0]


def Norm(cfg: "GPTConfig", device=None) -> torch.nn.Module:
    """The configured norm over d_model (``ln1`` / ``ln2`` / ``ln_f``): ``LayerNorm`` or ``RMSNorm``."""
    return (RMSNorm if cfg.norm == "rms" else LayerNorm)(cfg.d_model, cfg.dtype, device, cfg.eps)


def _window_mask(T: int, window: int, device) -> torch.Tensor:
    """The sliding-window causal mask ``[T, T]`` of a full sequence (True: seen): key j for query i iff
    ``0 <= i - j < window`` (``ops/decode.py``'s rule with one token per position)."""
    d = torch.arange(T, device=device).view(T, 1) - torch.arange(T, device=device).view(1, T)
    return (d >= 0) & (d < window)


def _qkv_shard(cfg: GPTConfig, tp: int, rank: int, seed: int, device) -> torch.Tensor:
    full = tpl.full_weight((3 * cfg.d_model, cfg.d_model), seed)
    hl, hd = cfg.n_heads // tp, cfg.head_dim
    rows = []
    for part in range(3):  # q, k, v
        base = part * cfg.d_model + rank * hl * hd
        rows.append(full[base:base + hl * hd])
    return torch.cat(rows, 0).to(dtype=cfg.dtype, device=device)


class Block(torch.nn.Module):
    def __init__(self, cfg: GPTConfig, layer: int, tp_group=None, device=None):
        super().__init__()
        tp = tpl._world(tp_group)
        if cfg.n_heads % tp:
            raise ValueError(f"n_heads={cfg.n_heads} not divisible by tp={tp}")
        if tp > 1 and cfg.kv_heads != cfg.n_heads:
            raise NotImplementedError("grouped-query attention (n_kv_heads < n_heads) with a tensor-parallel group of "
                                      "more than one rank: sharding the K / V heads is not built")
        self.cfg, self.tp_group = cfg, tp_group
        self.local_heads = cfg.n_heads // tp
        # K / V heads of this rank; fewer than local_heads: grouped-query attention (single rank only)
        self.local_kv_heads = self.local_heads if cfg.kv_heads == cfg.n_heads else cfg.kv_heads
        seed = 1000 * (layer + 1)
        self.ln1 = Norm(cfg, device)
        # fused QKV, column-parallel: each rank owns local_heads of q, k and v. Grouped-query attention: q | k | v
        # with kv_heads heads of k and of v ((n_heads + 2 kv_heads) * head_dim features; 3 * d_model without it)
        qkv_out = (3 * cfg.d_model if cfg.kv_heads == cfg.n_heads  # seeded as a (3 d_model, d_model) matrix, as ever
                   else (cfg.n_heads + 2 * cfg.kv_heads) * cfg.head_dim)
        self.qkv = tpl.ColumnParallelLinear(cfg.d_model, qkv_out, group=tp_group, dtype=cfg.dtype, device=device,
                                            seed=seed + 1)
        if tp > 1:
            # the canonical full QKV weight is [q_all; k_all; v_all]; this rank's column shard must
            # hold q, k and v rows of *its* heads so the sharded model equals the unsharded one
            with torch.no_grad():
                self.qkv.weight.copy_(_qkv_shard(cfg, tp, tpl._rank(tp_group), seed + 1, device))
        self.proj = tpl.RowParallelLinear(cfg.d_model, cfg.d_model, group=tp_group, dtype=cfg.dtype, device=device, seed=seed + 2)
        self.ln2 = Norm(cfg, device)
        # mlp="swiglu": 2 * d_ff features, interleaved gate / up rows (ops/swiglu.py), gated after the projection; a
        # contiguous column shard keeps whole pairs, so the tensor-parallel layers need nothing beyond the width
        self.swiglu = cfg.mlp == "swiglu"
        self.fc1 = tpl.ColumnParallelLinear(cfg.d_model, (2 if self.swiglu else 1) * cfg.d_ff,
                                            act="none" if self.swiglu else "gelu_tanh", group=tp_group,
                                            dtype=cfg.dtype, device=device, seed=seed + 3)
        self.fc2 = tpl.RowParallelLinear(cfg.d_ff, cfg.d_model, group=tp_group, dtype=cfg.dtype, device=device, seed=seed + 4)

    def _attention_gqa(self, x, residual, rope=None):
        """Grouped-query attention of the training forward off the fused ``ops.attn_block`` path (CPU, other head
        dims, forced-distributed runs). On the GPU the flash kernels read the ``[B, T, (h + 2 hkv) hd]`` activation
        in place (``ops.attention_qkv(kv_heads=...)``: every K / V head serves its group, dk / dv summed over the
        group in the kernel); elsewhere SDPA runs on K / V repeated over the group."""
        B, T, _ = x.shape
        h, hkv, hd = self.local_heads, self.local_kv_heads, self.cfg.head_dim
        G = h // hkv
        qkv = self.qkv(x)
        if rope is not None:
            qkv = ops.rope_qkv(qkv, rope, h, hkv)
        if ops.native_enabled() and ops.attention_supported(qkv, hd):
            y = ops.attention_qkv(qkv.contiguous(), h, hd, causal=True, kv_heads=hkv)  # [B, T, h * hd]
            return self.proj(y, residual=residual)
        q = qkv[..., :h * hd].view(B, T, h, hd)
        k, v = qkv[..., h * hd:].view(B, T, 2, hkv, hd).unbind(2)
        k = k.unsqueeze(3).expand(B, T, hkv, G, hd).reshape(B, T, h, hd)
        v = v.unsqueeze(3).expand(B, T, hkv, G, hd).reshape(B, T, h, hd)
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))  # [B, h, T, hd] views
        y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return self.proj(y.transpose(1, 2).reshape(B, T, h * hd), residual=residual)

    def _attention_window(self, x, residual, rope=None):
        """Sliding-window attention of the training forward (``GPTConfig(window=W)``): SDPA under the windowed causal
        mask, on torch ops only (CPU tensors, ``ops.torch_reference()``, head dims the flash kernels do not take). The
        flash kernels have no window, so the native GPU path raises."""
        B, T, _ = x.shape
        h, hkv, hd = self.local_heads, self.local_kv_heads, self.cfg.head_dim
        if x.is_cuda and ops.native_enabled() and ops.attention_supported(x, hd):
            raise NotImplementedError("GPTConfig(window=...): the flash attention kernels (ops.flash_attention / "
                                      "attention_qkv / attn_block) have no sliding window; the training forward of a "
                                      "windowed model runs on the torch path (CPU, ops.torch_reference()) only")
        qkv = self.qkv(x)
        if rope is not None:
            qkv = ops.rope_qkv(qkv, rope, h, hkv)
        q, k, v = GPT._split_gqa(qkv, h, hkv, hd)
        y = F.scaled_dot_product_attention(q, k, v, attn_mask=_window_mask(T, self.cfg.window, x.device))
        return self.proj(y.transpose(1, 2).reshape(B, T, h * hd), residual=residual)

    def attention(self, x, residual=None, rope=None):
        """``rope``: the model's rotary table (``GPTConfig(pos="rope")``): q and k are rotated right after the QKV
        projection, inside ``ops.attn_block`` on the fused path, by ``ops.rope_qkv`` on the others."""
        B, T, _ = x.shape
        h, hkv, hd = self.local_heads, self.local_kv_heads, self.cfg.head_dim
        if self.cfg.window is not None:
            return self._attention_window(x, residual, rope)
        # the fused single-rank path whenever the TP layers would issue no collective; a forced-distributed
        # run at world size 1 (KFAMD_FORCE_DIST) takes the TP layers and their RCCL all-reduces
        if x.is_cuda and ops.native_enabled() and ops.attention_supported(x, hd) and not tpl._collective(self.tp_group):
            # one autograd node on the HIP path (ops.attn_block): its backward runs the QKV and
            # output-projection weight gradients as one GEMM launch
            if hkv != h:  # grouped-query attention: the same node on the (h + 2 hkv) hd activation
                return ops.attn_block(x, self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias, h, hd,
                                      residual=residual, rope=rope, kv_heads=hkv)
            return ops.attn_block(x, self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias, h, hd,
                                  residual=residual, rope=rope)
        if hkv != h:
            return self._attention_gqa(x, residual, rope)
        qkv = self.qkv(x)  # [B, T, 3 * h * hd] — the column shard is [q_h | k_h | v_h] per rank
        if rope is not None:  # per head: a tensor-parallel shard rotates its own heads
            qkv = ops.rope_qkv(qkv, rope, h, h)
        if ops.native_enabled() and ops.attention_supported(qkv, hd):
            y = ops.attention_qkv(qkv.contiguous(), h, hd, causal=True)  # [B, T, h * hd]
            return self.proj(y, residual=residual)
        q, k, v = ops.split_heads(qkv, h, hd)  # backward: one pass into the QKV gradient layout
        y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return self.proj(y.transpose(1, 2).reshape(B, T, h * hd), residual=residual)

    def mlp(self, h, residual):
        if self.swiglu:  # linear -> gate (ops.swiglu: the elementwise kernels and their backward) -> fc2 (+ residual)
            return self.fc2(ops.swiglu(self.fc1(h)), residual=residual)
        # without TP, fc1 + fc2 are one autograd node on the HIP path (ops.mlp): fc2's dgrad applies
        # fc1's gelu backward in its GEMM epilogue
        if h.is_cuda and ops.native_enabled() and not tpl._collective(self.tp_group):
            return ops.mlp(h, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, act=self.fc1.act,
                           residual=residual)
        return self.fc2(self.fc1(h), residual=residual)

    def forward(self, x, rope=None):
        # both residual adds ride in the output projections' GEMM epilogues (without TP); the
        # residual gradient joins the LayerNorm backward's dx store (LayerNorm.with_residual)
        h, r = self.ln1.with_residual(x)
        x = self.attention(h, residual=r, rope=rope)
        h, r = self.ln2.with_residual(x)
        return self.mlp(h, r)


def _sample_top_k(logits, temperature, top_k, generator):
    """Multinomial over softmax(logits / temperature) restricted to exactly ``top_k`` candidates (the
    largest logits; among equal logits at the cut, the ones ``torch.topk`` returns)."""
    vals, ix = torch.topk(logits.float() / temperature, min(int(top_k), logits.shape[-1]), dim=-1)
    pick = torch.multinomial(torch.softmax(vals, -1), 1, generator=generator)
    return ix.gather(1, pick).squeeze(1)


def _sample(logits, temperature, top_k, generator):
    """Next token ``[B]`` from logits ``[B, vocab]``: argmax at temperature 0, else multinomial over
    softmax(logits / temperature), optionally restricted to the top_k largest logits."""
    # top_k == 1 leaves one candidate, the argmax. bf16 logits hold exact ties, which argmax and topk
    # need not break the same way, so that case takes argmax itself and equals greedy on any dtype.
    if temperature == 0 or top_k == 1:
        return logits.argmax(-1)
    if top_k is not None:
        return _sample_top_k(logits, temperature, top_k, generator)
    return torch.multinomial(torch.softmax(logits.float() / temperature, -1), 1, generator=generator).squeeze(1)


_LINEARS = ("qkv", "proj", "fc1", "fc2")

class DecodeWeights:
    """8-bit copies of a ``GPT``'s projection weights for the KV-cache steps (``GPT.decode_weights``):
    ``blocks[i]`` maps "qkv" / "proj" / "fc1" / "fc2" to an ``ops.QuantizedWeight`` (to the model's own bf16 weight
    for a matrix whose inner dimension is no multiple of 16, which the 8-bit kernel does not take), ``head`` is the
    quantised LM head (the tied embedding; the embedding gather itself keeps the model's ``tok``). The
    biases are the model's own. ``unquantized`` names the matrices left in bf16 ("blocks.0.fc2", ...; empty when all
    were quantised). Plain tensors: neither parameters nor buffers."""

    def __init__(self, blocks: list, head, key: tuple):
        self.blocks, self.head, self._key = blocks, head, key
        self.unquantized = [f"blocks.{i}.{n}" for i, b in enumerate(blocks) for n in _LINEARS
                            if not isinstance(b[n], ops.QuantizedWeight)]
        if not isinstance(head, ops.QuantizedWeight):
            self.unquantized.append("head")

    def matrices(self) -> list:
        return [b[n] for b in self.blocks for n in _LINEARS] + [self.head]

    @property
    def nbytes(self) -> int:
        """The sum of the quantised matrices' ``nbytes`` (codes + fp32 row scales)."""
        return sum(q.nbytes for q in self.matrices())


def _flinear(x, w, bias=None):
    """``F.linear`` of the torch path; a ``QuantizedWeight`` enters as its dequantised value in x's dtype."""
    if isinstance(w, ops.QuantizedWeight):
        w = w.dequantize().to(x.dtype)
    return F.linear(x, w, bias)


class _GraphedDecodeStep:
    """A captured ``decode_step``: the replay runs no Python of the step, so the capacity check and the
    host-side bound of ``decode_step`` are kept here (``cache.lens`` may never pass the capacity: the
    position embedding is gathered by it)."""

    def __init__(self, graphed, cache, limit: int | None = None):
        self.graphed, self.cache = graphed, cache
        self.limit = cache.capacity if limit is None else limit  # a ring cache: the model's max_seq

    def __call__(self, tok: torch.Tensor) -> torch.Tensor:
        c = self.cache
        if c._bound + 1 > self.limit:
            raise ValueError(f"max_seq {self.limit} exceeded" if c.ring else f"cache capacity {c.capacity} exceeded")
        if c.pool is not None:  # the replay reads the device table: a page taken here is seen by it
            c.reserve(1)
        out = self.graphed(tok)
        c._bound += 1
        if c.pool is not None:
            c._hlen = [n + 1 for n in c._hlen]  # the replay advanced lens on the device
        return out


class _GraphedGenerateStep:
    """A captured ``decode_step`` -> ``ops.sample`` -> ``step += 1`` (``GPT.graphed_generate_step``): one
    ``replay()`` per generated token and no other host work. As in ``_GraphedDecodeStep`` the capacity check
    and the host-side bound of ``decode_step`` are kept here."""

    def __init__(self, graphed, cache, keep, limit: int | None = None):
        self.graphed, self.cache, self._keep = graphed, cache, keep  # the captured kernels read `keep`
        self.limit = cache.capacity if limit is None else limit  # a ring cache: the model's max_seq

    def replay(self) -> None:
        c = self.cache
        if c._bound + 1 > self.limit:
            raise ValueError(f"max_seq {self.limit} exceeded" if c.ring else f"cache capacity {c.capacity} exceeded")
        if c.pool is not None:  # the replay reads the device table: a page taken here is seen by it
            c.reserve(1)
        self.graphed.graph.replay()
        c._bound += 1
        if c.pool is not None:
            c._hlen = [n + 1 for n in c._hlen]  # the replay advanced lens on the device


class GPT(torch.nn.Module):
    def __init__(self, cfg: GPTConfig, tp_group=None, device=None):
        super().__init__()
        self.cfg = cfg
        g = torch.Generator(device="cpu").manual_seed(7)
        emb = torch.randn(cfg.vocab_size, cfg.d_model, generator=g) * 0.02
        pos = torch.randn(cfg.max_seq, cfg.d_model, generator=g) * 0.01
        self.tok = torch.nn.Parameter(emb.to(dtype=cfg.dtype, device=device))
        if cfg.pos == "rope":  # no position parameter; one fp32 table [max_seq, head_dim], not in the state dict
            self.register_parameter("pos", None)
            self.register_buffer("rope_table", ops.rope_table(cfg.max_seq, cfg.head_dim, cfg.rope_theta, device),
                                 persistent=False)
        else:
            self.pos = torch.nn.Parameter(pos.to(dtype=cfg.dtype, device=device))
            self.register_buffer("rope_table", None, persistent=False)
        self.blocks = torch.nn.ModuleList([Block(cfg, i, tp_group, device) for i in range(cfg.n_layers)])
        self.ln_f = Norm(cfg, device)

    def forward(self, idx, targets=None):
        B, T = idx.shape
        x = F.embedding(idx, self.tok)
        if self.pos is not None:
            x = x + self.pos[:T]
        for blk in self.blocks:
            x = blk(x, self.rope_table)
        x = self.ln_f(x)
        logits = tpl._linear(x, self.tok)  # tied output head [B, T, vocab]
        if targets is None:
            return logits
        return logits, _cross_entropy(logits, targets)

    # ---- KV-cache generation --------------------------------------------------------------------
    # prefill() runs the prompt once and fills the cache; decode_step() runs ONE new token per batch
    # row against it. On the GPU both run on the HIP kernels (prefill: the training forward's GEMMs +
    # flash attention; decode: the M <= 16 weight-streaming GEMM with fused epilogues, ops.kv_append,
    # ops.attention_decode); CPU tensors and ops.torch_reference() run the same methods on torch ops.
    # Nothing in decode_step depends on a host-side position (the position embedding is gathered by
    # the device-side cache.lens), so it can be captured once into a hipGraph and replayed.
    # prefill(), decode_step() and extend()'s _extend_chunk() keep the embedding, the positions and cache.advance;
    # the layer itself is _cache_layer() and the LM head _lm_head(), each written once per path.

    def new_cache(self, B: int, capacity: int, device=None, kv_dtype: torch.dtype | None = None,
                  ring: bool = False, paged: bool = False, pool: "ops.PagePool | None" = None,
                  n_pages: int | None = None) -> "ops.KVCache":
        """A cache for B sequences of up to ``capacity`` tokens. ``kv_dtype``: what the cache stores;
        ``None`` is the model's dtype, ``torch.float8_e4m3fn`` the 8-bit cache (codes plus one fp32 scale
        per row: about half the bytes, see ``KVCache.nbytes``). ``ring=True`` (a windowed model only): a ring buffer of
        the last ``capacity`` positions (``ops/decode.py``'s ring rule): ``capacity`` is a multiple of 256 and need
        neither exceed the window nor reach ``max_seq``; a step of T tokens needs ``window + T - 1 <= capacity``, and
        the positions stay bounded by ``max_seq`` (the position or rotary table). ``paged=True`` (or a ``pool``): a paged
        cache (``ops/decode.py``'s page rule) on ``pool``, or on a new ``ops.PagePool`` of ``n_pages`` pages (default
        ``B * capacity / 256``, which can never run short); ``capacity`` (at most ``max_seq``) is rounded up to a
        multiple of 256 and bounds a row's length, the memory is the pool's. A windowed model raises."""
        c = self.cfg
        if paged or pool is not None:
            if c.window is not None or ring:
                raise ValueError("new_cache(paged=True): a paged cache with a window or a ring is not built")
            if capacity > c.max_seq:
                raise ValueError(f"cache capacity {capacity} exceeds max_seq {c.max_seq}")
            cap = -(-capacity // ops.decode.PAGE) * ops.decode.PAGE
            hkv = self.blocks[0].local_kv_heads
            if pool is None:
                pool = ops.PagePool(c.n_layers, hkv, c.head_dim, B * cap // ops.decode.PAGE if n_pages is None
                                    else n_pages, device=device if device is not None else self.tok.device,
                                    dtype=kv_dtype if kv_dtype is not None else c.dtype)
            elif n_pages is not None:
                raise ValueError("new_cache: n_pages sizes a new pool; it cannot be given with pool=")
            return ops.KVCache(c.n_layers, B, hkv, c.head_dim, cap, dtype=kv_dtype, pool=pool)
        if ring and c.window is None:
            raise ValueError("new_cache(ring=True): a ring cache needs a windowed model (GPTConfig(window=W))")
        if not ring and capacity > c.max_seq:
            raise ValueError(f"cache capacity {capacity} exceeds max_seq {c.max_seq}")
        return ops.KVCache(c.n_layers, B, self.blocks[0].local_kv_heads, c.head_dim, capacity,
                           device=device if device is not None else self.tok.device,
                           dtype=kv_dtype if kv_dtype is not None else c.dtype,
                           **({"ring": True, "window": c.window} if ring else {}))

    def _native_decode(self, x: torch.Tensor) -> bool:
        # both paths read the sharded weights without the TP layers' all-reduces: refuse, on any device
        if tpl._collective(self.blocks[0].tp_group):
            raise NotImplementedError("KV-cache generation with a tensor-parallel group that issues collectives")
        if not (x.is_cuda and ops.native_enabled()):
            return False
        if self.cfg.dtype != torch.bfloat16 or self.cfg.head_dim not in ops.decode.HEAD_DIMS:
            raise ValueError(f"KV-cache generation on a GPU: bf16 and head dim in {ops.decode.HEAD_DIMS} expected, "
                             f"got {self.cfg.dtype}, head dim {self.cfg.head_dim}")
        return True

    def _check_cache(self, cache, B: int, T: int, step: int | None = None) -> None:
        """``T`` new tokens fit; ``step``: the tokens per attention call when the T run in several steps."""
        if cache.B != B or cache.n_layers != len(self.blocks):
            raise ValueError("cache does not match the batch / model")
        if cache.ring:  # positions are bounded by the tables, a step by the ring rule
            W, n = self.cfg.window, min(T, step or T)
            if W is None:
                raise ValueError("a ring cache needs a windowed model (GPTConfig(window=W))")
            if cache._bound + T > self.cfg.max_seq:
                raise ValueError(f"max_seq {self.cfg.max_seq} exceeded")
            if W + n - 1 > cache.capacity:
                raise ValueError(f"a step of {n} tokens with window {W} needs a ring of capacity >= {W + n - 1}, got "
                                 f"{cache.capacity}")
        elif cache._bound + T > cache.capacity:
            raise ValueError(f"cache capacity {cache.capacity} exceeded")
        elif cache.pool is not None:
            if self.cfg.window is not None:
                raise ValueError("a paged cache with a windowed model is not built")
            if cache._bound + T > self.cfg.max_seq:  # the capacity is rounded up to whole pages
                raise ValueError(f"max_seq {self.cfg.max_seq} exceeded")
            cache.reserve(T)  # the step's pages: present and private before the first append

    @staticmethod
    def _att(cache, T: int, window) -> dict:
        """What a step of T appended tokens hands to its attention: the lengths including them, the host bound that
        goes with them (none on a ring: its grid does not come from it) and the window."""
        return {"lens": cache.lens_after(T), "t_bound": None if cache.ring else cache.bound_after(T), "window": window}

    def _cache_layer(self, blk, li: int, x, cache, *, native: bool, lin, w, attend):
        """One layer against ``cache``, the body ``prefill``, ``decode_step`` and ``_extend_chunk`` share. They vary
        ``lin`` (``self._skinny`` or ``self._auto``), ``w(li, name)`` (the weight of "qkv" / "proj" / "fc1" / "fc2":
        ``_weight_selector``) and ``attend(li, qkv, native)``, the attention over the QKV linear's output as the linear
        returned it. ``native``: the HIP kernels on ``x [rows, d_model]``, ``attend`` returning ``[rows, h * hd]``; else
        torch ops (CPU tensors / ops.torch_reference()) on ``x [B, ..., d_model]``, ``attend`` returning that shape.
        The append also rotates a rotary layer's q and k in place, at positions read from the device-side lens."""
        h, rope = blk.local_heads, self.rope_table
        if native:
            qkv = lin(blk.ln1.fwd(x), w(li, "qkv"), blk.qkv.bias)  # [rows, (h + 2 * hkv) * hd]
            ops.kv_append(qkv.view(cache.B, -1, qkv.shape[-1]), cache, li, q_heads=h, rope=rope)
            x = lin(attend(li, qkv, True), w(li, "proj"), blk.proj.bias, residual=x)
            y = self._fc1(lin, blk.ln2.fwd(x), w(li, "fc1"), blk)
            return lin(y, w(li, "fc2"), blk.fc2.bias, residual=x)
        qkv = _flinear(blk.ln1(x), w(li, "qkv"), blk.qkv.bias)
        ops.kv_append(qkv.view(cache.B, -1, qkv.shape[-1]), cache, li, q_heads=h, rope=rope)
        x = x + _flinear(attend(li, qkv, False), w(li, "proj"), blk.proj.bias)
        y = self._fc1_torch(blk.ln2(x), w(li, "fc1"), blk)
        return x + _flinear(y, w(li, "fc2"), blk.fc2.bias)

    def _lm_head(self, x, w, lin, native: bool):
        """``ln_f`` -> the tied LM head on the weight ``w`` (``_head_weight``): ``lin`` (``_skinny`` / ``_auto``) over
        ``x [rows, d_model]`` on the HIP kernels, else torch ops over ``x [..., d_model]``."""
        if native:
            return lin(self.ln_f.fwd(x), w)
        return _flinear(self.ln_f(x), w)

    @torch.no_grad()
    def prefill(self, idx: torch.Tensor, cache) -> torch.Tensor:
        """Run the prompt ``idx [B, T0]`` into an empty ``cache``; logits ``[B, vocab]`` of the last position.
        The prompt's own attention runs on the unquantised QKV activation (the flash kernel on the GPU) and
        never reads the cache: with an FP8 cache only what is STORED is quantised, and the logits are those
        of a bf16 cache bit for bit.

        A windowed model (``GPTConfig(window=W)``) on the GPU kernels cannot use the flash kernel, which has no
        window: the prompt then runs over the cache as ONE ``extend`` step of T0 rows on ``ops.attention_chunk``
        (``generate(prefill_chunk=N)`` runs it in steps of N instead). With an FP8 cache the prompt then attends the
        QUANTISED rows, as ``prefill_chunk`` does, and the logits are no longer those of a bf16 cache. On the torch
        path (CPU, ``ops.torch_reference()``) the prompt's attention stays on the activation, under the windowed mask."""
        B, T = idx.shape
        if cache.ring and self.cfg.window is not None and self.cfg.window + T - 1 > cache.capacity:
            raise ValueError(f"prefill: a prompt of {T} tokens with window {self.cfg.window} needs a ring of capacity >= "
                             f"{self.cfg.window + T - 1}, got {cache.capacity}: run it in steps with extend(chunk=N)")
        self._check_cache(cache, B, T)
        if cache._bound != 0:
            raise ValueError("prefill expects an empty cache (continuing a cache takes decode_step)")
        native = self._native_decode(self.tok)
        c = self.cfg
        if native and c.window is not None:  # the windowed MFMA kernel over the cache: one step of T rows
            return self._extend_chunk(idx, cache, True, head="last", mfma=True)
        h, hkv, hd = self.blocks[0].local_heads, self.blocks[0].local_kv_heads, c.head_dim
        kv = {} if hkv == h else {"kv_heads": hkv}  # grouped K / V heads, read in place by the flash kernel
        mask = {"is_causal": True} if c.window is None else {"attn_mask": _window_mask(T, c.window, idx.device)}

        def attend(li, qkv, native):  # over the QKV activation itself, which kv_append has rotated (rotary)
            if native:
                return ops.attention_qkv(qkv.view(B, T, -1), h, hd, causal=True, **kv).view(B * T, h * hd)
            q, k, v = self._split_gqa(qkv, h, hkv, hd)
            return F.scaled_dot_product_attention(q, k, v, **mask).transpose(1, 2).reshape(B, T, h * hd)
        x = F.embedding(idx, self.tok)
        if self.pos is not None:
            x = x + self.pos[:T]
        if native:
            x = x.reshape(B * T, c.d_model)
        w = self._weight_selector(None, B * T)  # the model's own weights, on the "auto" route, whatever B * T is
        for li, blk in enumerate(self.blocks):
            x = self._cache_layer(blk, li, x, cache, native=native, lin=self._auto, w=w, attend=attend)
        cache.advance(T)
        last = x.view(B, T, c.d_model)[:, -1]  # the LM head of the last position only
        # M = B rows: auto routes it as the parent commit did
        return self._lm_head(last.contiguous() if native else last, self.tok, self._auto, native)

    @staticmethod
    def _split_gqa(qkv, h: int, hkv: int, hd: int):
        """q, k, v ``[B, h, T, hd]`` of a fused activation ``[B, T, (h + 2 hkv) hd]``: views when hkv == h, else
        K / V with every head repeated over its group (materialised)."""
        B, T = qkv.shape[:2]
        q = qkv[..., :h * hd].view(B, T, h, hd).transpose(1, 2)
        k, v = qkv[..., h * hd:].view(B, T, 2, hkv, hd).unbind(2)
        if hkv != h:
            k, v = (t.repeat_interleave(h // hkv, dim=2) for t in (k, v))
        return q, k.transpose(1, 2), v.transpose(1, 2)

    def _skinny(self, x, w, bias=None, act="none", residual=None):
        # decode linears: the weight-streaming kernel wherever it beat the "auto" route in
        # profiles/decode (every gpt-1b projection shape at M = 1, 2, 4, 8, 16: 2.8x to 28x)
        return ops.gemm_nt(x, w, bias=bias, act=act, residual=residual, variant="skinny")

    def _auto(self, x, w, bias=None, act="none", residual=None):
        # more than 16 rows (extend with B * T > 16): the "auto" route, as prefill
        return ops.gemm_nt(x, w, bias=bias, act=act, residual=residual)

    def _fc1(self, lin, y, w, blk):
        """The up-projection and its activation on the HIP kernels, ``lin`` being ``_skinny`` or ``_auto``. GELU: the
        GEMM's epilogue on either route. SwiGLU: on the weight-streaming route the gated GEMM, one launch as GELU has
        (it won or tied the two-launch form at every measured M, weight format and d_ff: profiles/glu/README.md);
        on the "auto" route (more than 16 rows, and every prefill) the GEMM to [rows, 2 d_ff], then the elementwise
        gate kernel."""
        if not blk.swiglu:
            return lin(y, w, blk.fc1.bias, act=blk.fc1.act)
        if lin == self._skinny:
            return lin(y, w, blk.fc1.bias, act="swiglu")
        return ops.swiglu(lin(y, w, blk.fc1.bias))

    @staticmethod
    def _fc1_torch(y, w, blk):
        """The same on torch ops (CPU tensors / ops.torch_reference())."""
        z = _flinear(y, w, blk.fc1.bias)
        return ops.swiglu(z) if blk.swiglu else F.gelu(z, approximate="tanh")

    # ---- 8-bit decode weights ---------------------------------------------------------------------
    def decode_weights(self, dtype: torch.dtype = torch.float8_e4m3fn) -> DecodeWeights:
        """8-bit copies (``ops.quantize_weight``: e4m3fn codes + one fp32 scale per output row) of every
        block's qkv / proj / fc1 / fc2 weight and of the LM head, for ``decode_step`` / ``extend`` /
        ``graphed_decode_step`` / ``generate``. With a tensor-parallel group that issues no collective the
        local shards are quantised. The biases and the embedding gather keep the model's tensors. A matrix whose
        inner dimension is no multiple of 16 (the 8-bit kernel's contract; e.g. fc2 with d_ff = 344) is not quantised:
        its entry is the model's bf16 weight and its steps run the bf16 weight-streaming kernel; the call warns, and
        the result's ``unquantized`` lists them.

        The copies are plain tensors, absent from ``state_dict()`` and from any optimiser. The result is
        memoised on the model, keyed by the source parameters' ``_version`` (and storage): a call after an
        in-place update (a training step) requantises what changed and returns a new object. An object kept
        across an update is stale and out of contract: ask the model again after training.

        Which steps read them: those of up to 16 rows, see ``extend``; ``prefill`` never does."""
        if dtype != torch.float8_e4m3fn:
            raise ValueError(f"decode_weights: torch.float8_e4m3fn expected, got {dtype}")
        srcs = [getattr(blk, n).weight for blk in self.blocks for n in _LINEARS] + [self.tok]
        key = tuple((p._version, p.data_ptr(), str(p.device), p.dtype) for p in srcs)
        memo = self.__dict__.get("_decode_weights")
        if memo is not None and memo._key == key:
            return memo
        old = memo.matrices() if memo is not None and len(memo._key) == len(key) else [None] * len(srcs)
        with torch.no_grad():
            # the W8A16 kernel takes K % 16 == 0: a matrix off that grid (fc2 of a Llama-style d_ff such as 344 or
            # 11008 / tp) stays the model's bf16 parameter, and its steps run the bf16 weight-streaming kernel
            qs = [q if q is not None and memo._key[i] == key[i]
                  else (ops.quantize_weight(p.detach()) if p.shape[1] % 16 == 0 else p.detach())
                  for i, (p, q) in enumerate(zip(srcs, old))]
        n = len(_LINEARS)
        blocks = [dict(zip(_LINEARS, qs[i * n:(i + 1) * n])) for i in range(len(self.blocks))]
        memo = DecodeWeights(blocks, qs[-1], key)
        if memo.unquantized:  # once per (memoised) object: the caller asked for 8-bit weights and gets a mixed set
            warnings.warn(f"decode_weights: {len(memo.unquantized)} matrices keep bf16 weights (inner dimension no "
                          f"multiple of 16): {', '.join(memo.unquantized[:4])}"
                          f"{', ...' if len(memo.unquantized) > 4 else ''}", stacklevel=2)
        self.__dict__["_decode_weights"] = memo  # not a parameter, buffer or submodule
        return memo

    def _weight_selector(self, weights, rows: int):
        """(layer, name) -> the weight a step of ``rows`` rows reads in that linear: the 8-bit one when
        ``weights`` is given and the step takes the weight-streaming route (rows <= 16), else the model's."""
        if weights is not None and not isinstance(weights, DecodeWeights):
            raise TypeError("weights: a DecodeWeights (GPT.decode_weights()) expected")
        if weights is None or rows > ops.gemm.SKINNY_MAX_M:
            return lambda li, name: getattr(self.blocks[li], name).weight
        if len(weights.blocks) != len(self.blocks):
            raise ValueError("weights do not match the model")
        return lambda li, name: weights.blocks[li][name]

    def _head_weight(self, weights, rows: int):
        return self.tok if weights is None or rows > ops.gemm.SKINNY_MAX_M else weights.head

    @torch.no_grad()
    def decode_step(self, tok: torch.Tensor, cache, weights: "DecodeWeights | None" = None) -> torch.Tensor:
        """One new token ``tok [B]`` per row against ``cache``; logits ``[B, vocab]``. Advances the cache.
        ``weights`` (``decode_weights()``): a step of B <= 16 rows reads the 8-bit weights in every linear and
        in the LM head; a wider batch reads the bf16 weights (the rule of ``extend``)."""
        B = tok.shape[0]
        self._check_cache(cache, B, 1)
        native = self._native_decode(self.tok)
        h, hd = self.blocks[0].local_heads, self.cfg.head_dim
        wsel = self._weight_selector(weights, B)
        head_w = self._head_weight(weights, B)
        x = F.embedding(tok, self.tok)  # [B, d_model]
        if self.pos is not None:
            x = x + F.embedding(cache.lens, self.pos)
        # the step's attention sees the row it appends: lens + 1, computed on the device
        att = self._att(cache, 1, self.cfg.window)

        def attend(li, qkv, native):
            q = qkv[:, :h * hd].view(B, h, hd)
            if not native:
                return ops.attention_decode(q, cache, li, **att).reshape(B, h * hd)
            a = torch.empty(B, h * hd, device=qkv.device, dtype=qkv.dtype)
            ops.attention_decode(q, cache, li, out=a.view(B, h, hd), **att)
            return a
        for li, blk in enumerate(self.blocks):
            x = self._cache_layer(blk, li, x, cache, native=native, lin=self._skinny, w=wsel, attend=attend)
        cache.advance(1)
        return self._lm_head(x, head_w, self._skinny, native)

    @torch.no_grad()
    def extend(self, idx: torch.Tensor, cache, last_only: bool = False,
               weights: "DecodeWeights | None" = None, chunk: int | None = None) -> torch.Tensor:
        """Append ``idx [B, T]`` (T >= 1 tokens per row) to ``cache`` in any state, empty included; logits
        ``[B, T, vocab]`` of every new position (``[B, vocab]`` of the last one with ``last_only``).
        Advances the cache by T. On the GPU a step of up to 16 tokens runs the decode kernels with
        ``ops.attention_extend`` (K / V read once per 8 new rows; the weight-streaming GEMM while
        B * T <= 16); longer inputs run in chunks of 16. Like ``decode_step`` it reads the position
        from the device-side ``cache.lens`` only, so a fixed T <= 16 can be captured into a hipGraph.
        A grouped-query model (``n_kv_heads < n_heads``, G query heads per K / V head) steps ``16 // G`` tokens
        at a time on this path: ``ops.attention_extend`` takes 16 rows per K / V head, and a token is G of them.

        ``weights`` (``decode_weights()``): a chunk whose linears take the weight-streaming route, B * T <= 16
        rows, reads the 8-bit weights; the LM head does by its own row count (B with ``last_only``). Chunks
        with more rows read the bf16 weights, as ``prefill`` always does (compute-bound, and the originals
        are there). The rule looks at row counts only, on every device: the CPU / ``ops.torch_reference()``
        path applies it with the dequantised weights.

        ``chunk=N`` (16 < N <= the cache's capacity): the input runs in steps of N tokens per row instead of 16,
        attention on ``ops.attention_chunk`` (MFMA query tiles over the cache, K / V read once per 128 new
        rows), the linears on the route the step's row count B * N picks (the bf16 weights above 16 rows,
        whatever ``weights`` holds). It always means that kernel, a last step of 16 tokens or fewer included.
        What a follow-up turn or a long prompt over a cache in any state takes: N rows of activations at a
        time, one pass over the weights per N tokens. Capturable for a fixed T like the default path (one
        eager call first: the attention workspace is allocated on first use). ``chunk=None`` is the path
        described above, unchanged."""
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise ValueError(f"extend: idx [B, T >= 1] expected, got {tuple(idx.shape)}")
        B, T = idx.shape
        if not cache.ring:
            self._check_cache(cache, B, T)
        native = self._native_decode(self.tok)
        R = ops.decode.MAX_EXTEND_ROWS
        if chunk is None and native:  # the kernel takes 16 ROWS per K / V head: 16 // G tokens of a grouped-query model
            R = max(R // (self.blocks[0].local_heads // self.blocks[0].local_kv_heads), 1)  # G > 16: the op raises
        if chunk is not None:
            if isinstance(chunk, bool) or not isinstance(chunk, int) or not R < chunk <= cache.capacity:
                raise ValueError(f"extend(chunk=...): an int in {R + 1} .. the cache's capacity ({cache.capacity}) "
                                 f"expected, got {chunk!r}")
            R = chunk
        if cache.ring:  # the ring rule bounds a step, not the whole input
            self._check_cache(cache, B, T, step=R)
        outs = []
        for t0 in range(0, T, R):
            final = t0 + R >= T
            if last_only and not final:
                self._extend_chunk(idx[:, t0:t0 + R], cache, native, head="none", weights=weights,
                                   mfma=chunk is not None)
            else:
                outs.append(self._extend_chunk(idx[:, t0:t0 + R], cache, native, head="last" if last_only else "all",
                                               weights=weights, mfma=chunk is not None))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 1)

    def _extend_chunk(self, idx, cache, native: bool, head: str, weights=None, mfma: bool = False):
        """One extend step of T tokens per row (T <= 16 on ``ops.attention_extend``; any T with ``mfma``, on
        ``ops.attention_chunk``); ``head``: LM head on "all" rows, the "last", or "none"."""
        B, T = idx.shape
        attention = ops.attention_chunk if mfma else ops.attention_extend
        c = self.cfg
        h, hd = self.blocks[0].local_heads, c.head_dim
        x = F.embedding(idx, self.tok)  # [B, T, d_model]
        if self.pos is not None:
            pos = cache.lens.unsqueeze(1) + torch.arange(T, device=idx.device, dtype=cache.lens.dtype)  # [B, T], device
            x = x + F.embedding(pos, self.pos)
        # the step's attention sees the rows it appends: lens + T, computed on the device
        att = self._att(cache, T, c.window)
        lin = self._skinny if B * T <= ops.gemm.SKINNY_MAX_M else self._auto
        wsel = self._weight_selector(weights, B * T)

        def attend(li, qkv, native):
            q = qkv[..., :h * hd].view(B, T, h, hd)
            if not native:
                return attention(q, cache, li, **att).reshape(B, T, h * hd)
            a = torch.empty(B, T, h * hd, device=qkv.device, dtype=qkv.dtype)
            attention(q, cache, li, out=a.view(B, T, h, hd), **att)
            return a.view(B * T, h * hd)
        if native:
            x = x.reshape(B * T, c.d_model)
        for li, blk in enumerate(self.blocks):
            x = self._cache_layer(blk, li, x, cache, native=native, lin=lin, w=wsel, attend=attend)
        cache.advance(T)
        if head == "none":
            return None
        x = x.view(B, T, c.d_model)
        if head == "last":
            x = x[:, -1].contiguous()  # [B, d_model]
        rows = x.numel() // c.d_model  # the head's own row count picks its weight and its route
        head_w = self._head_weight(weights, rows)
        head_lin = self._skinny if rows <= ops.gemm.SKINNY_MAX_M else self._auto
        if not native:
            return self._lm_head(x, head_w, head_lin, False)
        return self._lm_head(x.reshape(rows, c.d_model), head_w, head_lin, True).view(*x.shape[:-1], c.vocab_size)

    def _ring_capacity(self, step: int) -> int:
        """The capacity ``generate(ring=True)`` gives a ring whose largest step is ``step`` tokens: ``window + step - 1``
        rounded up to a multiple of 256."""
        return -(-(self.cfg.window + step - 1) // ops.decode.RING_ALIGN) * ops.decode.RING_ALIGN

    def _generate_draft(self, idx, max_new_tokens: int, draft: "GPT", lookahead: int, kv_dtype=None, tw=None,
                        dw=None, ring_chunk: int | None = None):
        """Greedy draft-and-verify for one sequence: per round the draft proposes up to ``lookahead``
        tokens (``decode_step`` on its own cache), the target scores ``[last accepted, proposals...]`` in
        ONE ``extend`` and keeps the longest prefix that equals its own argmax, plus its own next token
        (the correction at the first mismatch, or the extra token after a full acceptance)."""
        T0 = idx.shape[1]
        total = T0 + max_new_tokens
        def cache_and_prompt(m):  # ring_chunk=N: a ring where the model has a window, its prompt in steps of N
            if ring_chunk is None or m.cfg.window is None:
                c = m.new_cache(1, total, device=idx.device, kv_dtype=kv_dtype)
                if T0 > 1:
                    m.prefill(idx[:, :-1], c)
                return c
            c = m.new_cache(1, m._ring_capacity(max(ring_chunk, 16, lookahead + 1)), device=idx.device,
                            kv_dtype=kv_dtype, ring=True)
            if T0 > 1:
                m.extend(idx[:, :-1], c, last_only=True, chunk=ring_chunk)
            return c
        # both caches hold the prompt but its last token: every new token comes from a round
        tc, dc = cache_and_prompt(self), cache_and_prompt(draft)
        seq = idx[0].tolist()
        stats = {"target_steps": 0, "proposed": 0, "accepted": 0}
        while len(seq) < total:
            K = min(lookahead, total - len(seq) - 1)  # a round emits at most K + 1 tokens
            last = torch.tensor([seq[-1]], dtype=idx.dtype, device=idx.device)
            props, tok = [], last
            for _ in range(K):
                tok = draft.decode_step(tok, dc, weights=dw).argmax(-1)
                props.append(tok)
            row = torch.cat([last, *props]).view(1, K + 1)
            want = self.extend(row, tc, weights=tw).argmax(-1)[0].tolist()  # the target's token after each row
            prop = row[0, 1:].tolist()
            n = 0
            while n < K and prop[n] == want[n]:
                n += 1
            seq += prop[:n] + [want[n]]
            tc.rewind(K - n)  # the cache keeps [last, accepted proposals]
            if K > 0 and n == K:
                draft.decode_step(props[-1], dc, weights=dw)  # the draft has not seen its own last proposal yet
            elif K > 0:
                dc.rewind(K - 1 - n)  # the draft's cache holds [last, proposals but the final one]
            stats["target_steps"] += 1
            stats["proposed"] += K
            stats["accepted"] += n
        return torch.tensor([seq], dtype=idx.dtype, device=idx.device), stats

    @torch.no_grad()
    def generate(self, idx: torch.Tensor, max_new_tokens: int, temperature: float = 0.0, top_k: int | None = None,
                 generator: torch.Generator | None = None, graph: bool = False, draft: "GPT | None" = None,
                 lookahead: int = 4, return_stats: bool = False, kv_dtype: torch.dtype | None = None,
                 weight_dtype: torch.dtype | None = None, top_p: float | None = None, stop_token: int | None = None,
                 sampler: str = "torch", prefill_chunk: int | None = None, ring: bool = False, paged: bool = False,
                 num_samples: int | None = None, pool: "ops.PagePool | None" = None, return_cache: bool = False):
        """Sample ``max_new_tokens`` after the prompt ``idx [B, T0]`` -> ``[B, T0 + max_new_tokens]``.
        ``temperature == 0``: greedy; otherwise softmax sampling (optionally over the ``top_k`` largest
        logits) with ``torch.multinomial`` under ``generator``. ``graph=True`` (GPU): decode_step is
        captured once into a hipGraph and replayed per token.

        ``draft`` (a ``GPT`` with the same vocabulary): greedy draft-and-verify decoding, ``lookahead``
        proposals per target ``extend``; greedy only, B = 1, no ``graph``. ``return_stats`` then also
        returns ``{"target_steps", "proposed", "accepted"}``.

        ``kv_dtype``: what the KV cache stores (``new_cache``); ``torch.float8_e4m3fn`` halves its bytes.
        With a draft, both the target's and the draft's caches use it.

        ``weight_dtype``: ``torch.float8_e4m3fn`` decodes on ``self.decode_weights()`` (and the draft on its
        own): every step of up to 16 rows reads 8-bit projection weights and LM head, half the bytes of a
        small-batch step; the prompt's ``prefill`` and steps of more rows read the bf16 weights. It combines
        freely with ``kv_dtype`` and ``graph``. Any other dtype raises.

        ``sampler``: ``"torch"`` (the default) is the sampler described above; ``top_p`` / ``stop_token`` raise
        with it. ``"fused"`` samples every token with ``ops.sample`` (one HIP kernel on the GPU, the same rule
        in fp64 torch on the CPU): ``top_k``, then nucleus ``top_p`` on the top-k set's mass, ties broken by
        token index. Its uniforms are drawn once, ``torch.rand(max_new_tokens, B, generator=generator)`` on the
        generator's device (the CPU without one), so a seeded generation is the same on every device up to
        the logits. With ``stop_token`` a row that emits it is finished: the output keeps its shape ``[B, T0 +
        max_new_tokens]`` and the rest of such a row is padded with ``stop_token``; there is no per-token host
        sync and no early exit, every row runs ``max_new_tokens`` steps. It combines with ``kv_dtype``,
        ``weight_dtype`` and ``graph``; with ``graph=True`` the captured graph holds the step, the sampler and
        the token feedback (``graphed_generate_step``), so a token costs one replay. ``draft`` keeps its own
        greedy sampler: ``sampler="fused"`` with it raises.

        ``prefill_chunk=N`` (16 < N <= prompt + max_new_tokens, the cache's capacity): the prompt runs as
        ``extend(idx, cache, last_only=True, chunk=N)`` instead of ``prefill``: N tokens per row at a time through
        ``ops.attention_chunk``, so the prompt's activation memory is bounded by N rows whatever its length.
        Each step attends the cache, not the QKV activation: with ``kv_dtype=torch.float8_e4m3fn`` the prompt
        then attends the QUANTISED K / V it has stored, where ``prefill`` attends the unquantised rows, so the
        logits differ from a bf16 cache's from the first token on. It raises with ``draft`` (unless ``ring``).

        ``ring=True`` (a windowed model: it raises without ``GPTConfig(window=W)``): the cache is a ring buffer
        (``new_cache(ring=True)``), so the memory is O(window) whatever ``max_new_tokens`` is. The prompt runs through
        ``prefill_chunk=N`` (default 256) on every device, and the capacity is ``W + max(N, 16, lookahead + 1) - 1``
        rounded up to a multiple of 256. With ``draft=`` the target's cache is a ring, and the draft's is one iff the
        draft has a window. It composes with ``kv_dtype``, ``weight_dtype``, ``sampler="fused"``, ``graph=True``, grouped
        K / V heads and ``pos="rope"`` by shapes only.

        ``paged=True``: the same generation on a paged cache (``new_cache(paged=True)``; ``ops/decode.py``'s page rule),
        token for token and logit for logit. It composes with ``kv_dtype``, ``weight_dtype``, ``sampler="fused"``,
        ``graph=True`` (the whole length is reserved before the capture), ``prefill_chunk``, grouped K / V heads and
        ``pos="rope"``. ``num_samples=S`` (implies ``paged``): S samples per prompt. The prompt is prefilled once on B
        rows, the cache is forked S ways (the samples share the prompt's full pages; the parent's pages pass to its
        last child), the last position's logits are repeated S-fold and decoding continues on ``B * S`` rows. Returns
        ``[B * S, T0 + max_new_tokens]``, prompt-major: row ``b * S + s``; the samplers draw for ``B * S`` rows, so a
        seeded run equals a flat run on the prompts repeated S-fold. ``S = 1`` is ``paged=True``. The pool holds
        ``B * (T0 // 256) + B * S * (pages of the prompt's tail and the new tokens)`` pages. ``pool=``: generate on
        that ``ops.PagePool`` instead (it must have that many pages free); the pages return to it at the end.
        ``return_cache=True`` (paged only): returns ``(tokens, cache)`` and leaves the pages held, for a follow-up turn
        or a look at ``cache.pool``; call ``cache.release()`` when done. Not built (raises): ``paged`` / ``num_samples``
        with ``draft=``, with ``ring`` or a windowed model, or with a tensor-parallel group that issues collectives."""
        if num_samples is not None:
            if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
                raise ValueError(f"generate(num_samples=...): an int >= 1 expected, got {num_samples!r}")
            paged = True
        paged = bool(paged) or pool is not None
        if return_cache and not paged:
            raise ValueError("generate(return_cache=True) needs a paged cache (paged=True or num_samples=)")
        if paged:
            if draft is not None:
                raise NotImplementedError("generate: paged / num_samples with draft= is not built")
            if ring or self.cfg.window is not None:
                raise ValueError("generate: a paged cache with a window or a ring is not built")
            if tpl._collective(self.blocks[0].tp_group):
                raise NotImplementedError("generate: a paged cache with a tensor-parallel group that issues collectives "
                                          "is not built")
        if ring:
            if self.cfg.window is None:
                raise ValueError("generate(ring=True) needs a windowed model (GPTConfig(window=W))")
            if prefill_chunk is None:
                prefill_chunk = 256
        if prefill_chunk is not None and draft is not None and not ring:
            raise ValueError("generate(prefill_chunk=...) cannot be combined with draft=")
        if sampler not in ("torch", "fused"):
            raise ValueError(f'generate(sampler=...): "torch" or "fused" expected, got {sampler!r}')
        if sampler == "torch" and (top_p is not None or stop_token is not None):
            raise ValueError('generate(top_p=..., stop_token=...) need sampler="fused"')
        if sampler == "fused" and draft is not None:
            raise ValueError('generate(draft=...) keeps its greedy sampler: sampler="fused" cannot be combined with it')
        if weight_dtype is not None and weight_dtype != torch.float8_e4m3fn:
            raise ValueError(f"generate(weight_dtype=...): None or torch.float8_e4m3fn expected, got {weight_dtype}")
        B, T0 = idx.shape
        total = T0 + max_new_tokens
        if max_new_tokens < 0 or T0 < 1 or total > self.cfg.max_seq:
            raise ValueError(f"prompt {T0} + max_new_tokens {max_new_tokens} must fit max_seq {self.cfg.max_seq}")
        if draft is not None:
            if not (temperature == 0 or top_k == 1) or B != 1 or graph:
                raise ValueError("generate(draft=...): greedy (temperature == 0 or top_k == 1), B = 1 and graph=False "
                                 "expected")
            if not isinstance(draft, GPT) or draft.cfg.vocab_size != self.cfg.vocab_size or lookahead < 1:
                raise ValueError("generate(draft=...): a GPT with the same vocabulary and lookahead >= 1 expected")
            if total > draft.cfg.max_seq:
                raise ValueError(f"prompt + max_new_tokens must fit the draft's max_seq {draft.cfg.max_seq}")
            out, stats = ((idx.clone(), {"target_steps": 0, "proposed": 0, "accepted": 0}) if max_new_tokens == 0
                          else self._generate_draft(idx, max_new_tokens, draft, int(lookahead), kv_dtype,
                                                    self.decode_weights() if weight_dtype is not None else None,
                                                    draft.decode_weights() if weight_dtype is not None else None,
                                                    prefill_chunk if ring else None))
            return (out, stats) if return_stats else out
        if return_stats:
            raise ValueError("generate(return_stats=True) reports draft decoding: pass draft=")
        if max_new_tokens == 0:
            return idx.clone()
        if graph and not idx.is_cuda:
            raise ValueError("generate(graph=True) needs GPU tensors")
        S = num_samples or 1
        if ring:
            cache = self.new_cache(B, self._ring_capacity(max(prefill_chunk, 16, lookahead + 1)), device=idx.device,
                                   kv_dtype=kv_dtype, ring=True)
        elif paged:  # the prompt's full pages once per prompt, its tail and the new tokens once per sample
            P = ops.decode.PAGE
            n_pages = B * (T0 // P) + B * S * (-(-total // P) - T0 // P)
            if pool is not None and pool.pages_free < n_pages:
                raise RuntimeError(f"generate: {n_pages} pages needed, {pool.pages_free} free in the pool")
            cache = self.new_cache(B, total, device=idx.device, kv_dtype=kv_dtype, paged=True, pool=pool,
                                   n_pages=None if pool is not None else n_pages)
        else:
            cache = self.new_cache(B, total, device=idx.device, kv_dtype=kv_dtype)
        if prefill_chunk is None:
            logits = self.prefill(idx, cache)
        else:  # the bf16 weights, as prefill: a prompt is not a decode step
            logits = self.extend(idx, cache, last_only=True, chunk=prefill_chunk)
        if S > 1:  # one prefill, S continuations: row b * S + s
            cache = cache.fork(S, release=True)  # the parent's pages pass on: the pool is sized without them
            logits, idx, B = logits.repeat_interleave(S, 0), idx.repeat_interleave(S, 0), B * S
        if paged and graph:
            cache.reserve(max_new_tokens - 1)  # a capture cannot take pages: every position the replays append
        weights = self.decode_weights() if weight_dtype is not None else None
        if sampler == "fused":
            out = self._generate_fused(idx, logits, cache, weights, max_new_tokens, temperature, top_k, top_p,
                                       stop_token, generator, graph)
        else:
            step = lambda t: self.decode_step(t, cache, weights=weights)  # noqa: E731
            if graph and max_new_tokens > 1:
                step = self.graphed_decode_step(cache, weights=weights)
            out = [idx]
            for i in range(max_new_tokens):
                nxt = _sample(logits, temperature, top_k, generator)
                out.append(nxt.view(B, 1))
                if i + 1 < max_new_tokens:
                    logits = step(nxt)
            out = torch.cat(out, 1)
        if return_cache:
            return out, cache
        if paged and pool is not None:  # a caller's pool gets its pages back
            cache.release()
        return out


    def _generate_fused(self, idx, logits, cache, weights, S: int, temperature, top_k, top_p, stop_token, generator,
                        graph: bool):
        """The token loop of ``generate(sampler="fused")`` after the prefill (``logits``: its output)."""
        B, dev = idx.shape[0], idx.device
        u = torch.rand(S, B, generator=generator, device=generator.device if generator is not None else "cpu").to(dev)
        seq = torch.empty(B, S, dtype=torch.long, device=dev)  # the new tokens, one column per step
        tok = torch.empty(B, dtype=torch.long, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        done = torch.zeros(B, dtype=torch.int32, device=dev) if stop_token is not None else None
        kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, step=step, out=tok, seq=seq, done=done,
                  stop_token=stop_token)
        ops.sample(logits, u, **kw)  # the first token: from the prefill's logits, eagerly
        step.add_(1)
        if graph and S > 1:
            g = self.graphed_generate_step(cache, weights, tok=tok, u=u, **{k: v for k, v in kw.items() if k != "out"})
            for _ in range(S - 1):
                g.replay()
        else:
            for _ in range(S - 1):
                ops.sample(self.decode_step(tok, cache, weights=weights), u, **kw)
                step.add_(1)
        return torch.cat([idx, seq], 1)

    def graphed_generate_step(self, cache, weights: "DecodeWeights | None" = None, *, tok: torch.Tensor,
                              u: torch.Tensor, step: torch.Tensor, temperature: float = 1.0, top_k: int | None = None,
                              top_p: float | None = None, seq: torch.Tensor | None = None,
                              done: torch.Tensor | None = None,
                              stop_token: int | None = None) -> "_GraphedGenerateStep":
        """``decode_step(tok) -> ops.sample(..., out=tok) -> step += 1`` on ``cache`` captured once into a
        hipGraph, on a single stream: ``tok`` (int64 ``[B]``) is both the step's input and the sampler's
        output, so each ``replay()`` of the result turns the token of one position into the token of the next
        and writes it into column ``step`` of ``seq``, with no host work besides the replay. ``u [S, B]``,
        ``step``, ``seq``, ``done``, ``stop_token`` and the sampling arguments are ``ops.sample``'s. Nothing is
        returned per replay: read ``tok`` / ``seq`` once at the end.

        Everything the replay reads per token lives on the device (``cache.lens``, ``step``, ``tok``, ``done``);
        the host-side capacity check is kept (a ``replay()`` with no free cache row raises like
        ``decode_step``). The cache needs one free row, and ``step`` one free row of ``u``, for the warm-up
        step, whose effects (``lens``, ``step``, ``tok``, ``seq``, ``done``) are undone here. The graph holds the
        tensors' addresses: the returned object keeps them (and ``weights``) alive."""
        limit = self.cfg.max_seq if cache.ring else cache.capacity
        if cache._bound + 1 > limit:
            raise ValueError("graphed_generate_step needs a free cache row")
        if not cache.ring:  # a ring's grid does not come from the bound
            cache.pin_bound()
        bound = cache._bound
        hlen = list(cache._hlen) if cache.pool is not None else None  # a paged cache's host mirror of lens
        state = [t for t in (cache.lens, step, tok, seq, done) if t is not None]
        saved = [t.clone() for t in state]

        def body(t):  # warm-up and capture both start from the same host bound
            cache._bound = bound
            if hlen is not None:  # the warm-up took the step's page; the capture finds it and changes nothing
                cache._hlen = list(hlen)
            ops.sample(self.decode_step(t, cache, weights=weights), u, temperature=temperature, top_k=top_k,
                       top_p=top_p, step=step, out=t, seq=seq, done=done, stop_token=stop_token)
            step.add_(1)

        g = ops.GraphedCallable(body, tok, warmup=1)
        torch.cuda.current_stream().synchronize()
        for t, s0 in zip(state, saved):
            t.copy_(s0)
        cache._bound = bound
        if hlen is not None:
            cache._hlen = list(hlen)
        return _GraphedGenerateStep(g, cache, (weights, u, step, tok, seq, done), limit)

    def graphed_decode_step(self, cache, weights: "DecodeWeights | None" = None) -> "_GraphedDecodeStep":
        """``decode_step`` on ``cache`` captured once into a hipGraph (its attention grid sized for the
        whole capacity); each call replays it on a new token ``[B]`` and returns the logits, valid until
        the next call. The position lives in the device-side ``cache.lens``, which the replay advances;
        the host-side bound follows, and a call with no free cache row raises like ``decode_step``. The
        cache needs one free row for the warm-up step, whose effect on ``lens`` is undone here. ``weights``: as
        ``decode_step``; the graph holds the quantised tensors' addresses, so keep the object alive."""
        limit = self.cfg.max_seq if cache.ring else cache.capacity
        if cache._bound + 1 > limit:
            raise ValueError("graphed_decode_step needs a free cache row")
        if not cache.ring:  # a ring's grid does not come from the bound
            cache.pin_bound()
        saved, bound = cache.lens.clone(), cache._bound
        hlen = list(cache._hlen) if cache.pool is not None else None  # a paged cache's host mirror of lens

        def step(t):  # warm-up and capture both start from the same host bound
            cache._bound = bound
            if hlen is not None:  # the warm-up took the step's page; the capture finds it and changes nothing
                cache._hlen = list(hlen)
            return self.decode_step(t, cache, weights=weights)

        g = ops.GraphedCallable(step, torch.zeros(cache.B, dtype=torch.long, device=cache.lens.device), warmup=1)
        torch.cuda.current_stream().synchronize()
        cache.lens.copy_(saved)
        cache._bound = bound
        if hlen is not None:
            cache._hlen = list(hlen)
        gs = _GraphedDecodeStep(g, cache, limit)
        gs.weights = weights  # the captured kernels read these tensors: they live as long as the step
        return gs

    def flops_per_token(self, seq: int) -> float:
        """Training FLOPs/token (fwd+bwd = 3x fwd): dense matmuls + attention scores."""
        c = self.cfg
        kv = 2 * c.kv_heads * c.head_dim  # the K and V projections' features (2 * d_model without grouping)
        mlp = (3 if c.mlp == "swiglu" else 2) * c.d_model * c.d_ff  # gate, up and down / up and down
        dense = (2 * ((2 * c.d_model + kv) * c.d_model + mlp) * c.n_layers
                 + 2 * c.d_model * c.vocab_size)
        attn = 2 * 2 * seq * c.d_model * c.n_layers
        return 3.0 * (dense + attn)


def build(name_or_cfg, tp_group=None, device=None) -> GPT:
    cfg = CONFIGS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg
    return GPT(cfg, tp_group=tp_group, device=device)


def num_params(model: torch.nn.Module) -> int:
    return sum(p.numel() for p in model.parameters())


def init_scale(d: int) -> float:
    return 1.0 / math.sqrt(d)
