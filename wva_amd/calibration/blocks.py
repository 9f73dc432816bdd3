"""Pieces the three calibration engines share (model.py, moe_model.py,
tp_model.py): weight drawing and the layer weights, the KV slab and its
random fill, the residual/RMSNorm layer loop, the contiguous-layout decode
attention block and the one-shot prefill's q/k/v preparation, slab
write-back and attention.

The linears are not here: each call site keeps its own dispatch
(ops.linear, LlamaDecodeModel._linear, plain matmul in the prefill family,
all-reduced row-parallel linears under TP) and passes it in through the
`attn` / `mlp` callables of run_layers.
"""
from __future__ import annotations

import torch

from .. import ops


def w(rows, cols, device, dtype, gen) -> torch.Tensor:
    """A [rows, cols] weight drawn N(0, 0.02) from `gen`."""
    return torch.empty(rows, cols, device=device, dtype=dtype).normal_(
        0.0, 0.02, generator=gen
    )


class AttnLayer:
    """The norms and attention projections every layer has, drawn in the
    order wqkv, wo."""

    def __init__(self, hidden, q_size, kv_size, device, dtype, gen):
        self.input_norm = torch.ones(hidden, device=device, dtype=dtype)
        self.post_attn_norm = torch.ones(hidden, device=device, dtype=dtype)
        self.wqkv = w(q_size + 2 * kv_size, hidden, device, dtype, gen)
        self.wo = w(hidden, q_size, device, dtype, gen)


class DenseLayer(AttnLayer):
    """A Llama decoder layer. Under TP `q_size`, `kv_size` and `inter` are
    the rank's shard: wqkv and w_gate_up are column-parallel, wo and w_down
    row-parallel."""

    def __init__(self, hidden, q_size, kv_size, inter, device, dtype, gen):
        super().__init__(hidden, q_size, kv_size, device, dtype, gen)
        self.w_gate_up = w(2 * inter, hidden, device, dtype, gen)
        self.w_down = w(hidden, inter, device, dtype, gen)


def alloc_kv_slabs(num_layers, max_batch, num_kv_heads, max_seq, head_dim,
                   device, dtype):
    """(k_cache, v_cache): per layer one head-major contiguous slab
    [B, Hk, S, D] — each (sequence, kv-head) is one sequential HBM stream
    for the attention kernel's tile staging (docs/mi355x-kernels.md)."""
    k_cache = [
        torch.zeros(
            max_batch, num_kv_heads, max_seq, head_dim,
            device=device, dtype=dtype,
        )
        for _ in range(num_layers)
    ]
    v_cache = [torch.zeros_like(k_cache[0]) for _ in range(num_layers)]
    return k_cache, v_cache


def reset_kv_slabs(context_lens, k_cache, v_cache, batch, context_len):
    """Set context_lens[:batch] = context_len (0 elsewhere) and random-fill
    the slabs' first context_len rows of `batch` sequences, K then V per
    layer from the global generator."""
    context_lens.zero_()
    context_lens[:batch] = context_len
    for k, v in zip(k_cache, v_cache):
        for cache in (k, v):
            rows = cache[:batch, :, :context_len]
            if cache.dtype == torch.bfloat16:
                rows.normal_(0.0, 1.0)
            else:  # normal_ unsupported on float8: generate + cast
                cache[:batch, :, :context_len] = torch.randn(
                    rows.shape, device=cache.device, dtype=torch.bfloat16
                ).to(cache.dtype)


def run_layers(layers, x, final_norm, eps, attn, mlp) -> torch.Tensor:
    """The transformer-block skeleton over `layers` from the embedded rows
    `x`: fused add-RMSNorm, `attn(li, layer, h)`, fused add-RMSNorm,
    `mlp(layer, h2)`, and the final norm, whose output is returned. The
    callables own their linears; build them once per step, not per layer
    (at batch 1 the eager step is launch-bound and host work per layer
    lands in α)."""
    residual = None
    for li, layer in enumerate(layers):
        if residual is None:
            residual = x.clone()
            h = ops.rmsnorm(x, layer.input_norm, None, eps)
        else:
            h = ops.rmsnorm(x, layer.input_norm, residual, eps)
        x = attn(li, layer, h)
        x = mlp(layer, ops.rmsnorm(x, layer.post_attn_norm, residual, eps))
    return ops.rmsnorm(x, final_norm, residual, eps)


def decode_attn(qkv, k_cache, v_cache, positions, ctx, num_q_heads,
                num_kv_heads, rope_theta, scale) -> torch.Tensor:
    """Decode attention of `qkv [B, (Hq+2Hk)·D]` on rows 0..B-1 of one
    layer's contiguous slabs: RoPE on the strided qkv row fused with the KV
    append at `positions`, then GQA attention over `ctx = positions + 1`
    rows. Returns [B, Hq·D]."""
    B = qkv.shape[0]
    k, v = k_cache[:B], v_cache[:B]
    q = ops.rope_append_kv(
        qkv, k, v, positions, num_q_heads, num_kv_heads, rope_theta
    )
    return ops.gqa_decode_attn(q, k, v, ctx, scale).reshape(B, -1)


def prefill_qkv(qkv, positions, cfg):
    """Split prefill rows `qkv [T, (Hq+2Hk)·D]` into q [T, Hq, D] and
    k [T, Hk, D], both contiguous and roped in place at `positions [T]`
    (HIP kernel), and v [T, Hk, D]."""
    T, D = qkv.shape[0], cfg.head_dim
    q, k, v = qkv.split([cfg.q_size, cfg.kv_size, cfg.kv_size], dim=-1)
    q = q.reshape(T, cfg.num_q_heads, D).contiguous()
    k = k.reshape(T, cfg.num_kv_heads, D).contiguous()
    ops.rope(q, k, positions, cfg.rope_theta)
    return q, k, v.reshape(T, cfg.num_kv_heads, D)


def write_prefill_kv(k_cache, v_cache, k, v, B, S) -> None:
    """Copy a one-shot prefill's roped k and v [B·S, Hk, D] into rows 0..S-1
    of sequences 0..B-1 of one layer's head-major slabs."""
    for cache, new in ((k_cache, k), (v_cache, v)):
        cache[:B, :, :S].copy_(
            new.reshape(B, S, *new.shape[1:]).permute(0, 2, 1, 3)
        )


def causal_mask(S, device) -> torch.Tensor:
    """The additive fp32 [S, S] mask of causal_attn_reference."""
    return torch.full(
        (S, S), float("-inf"), device=device, dtype=torch.float32
    ).triu(1)


def causal_attn_reference(q, k_cache, v_cache, B, S, scale, causal):
    """CPU numerics reference of ops.prefill_attn: explicit causal matmul
    attention of q [B·S, Hq, D] over rows 0..S-1 of the populated slabs.
    Returns [B·S, Hq·D]."""
    Hq, D = q.shape[1], q.shape[2]
    Hk = k_cache.shape[1]
    G = Hq // Hk
    qh = (
        q.reshape(B, S, Hk, G, D)
        .permute(0, 2, 3, 1, 4)
        .reshape(B * Hk * G, S, D)
    )
    kh, vh = (
        cache[:B, :, :S].to(q.dtype)
        .unsqueeze(2)
        .expand(B, Hk, G, S, D)
        .reshape(B * Hk * G, S, D)
        for cache in (k_cache, v_cache)
    )
    scores = torch.bmm(qh, kh.transpose(1, 2)).float() * scale + causal
    p = torch.softmax(scores, dim=-1).to(q.dtype)
    attn = torch.bmm(p, vh)  # [B*Hq, S, D]
    return (
        attn.reshape(B, Hq, S, D).permute(0, 2, 1, 3).reshape(B * S, Hq * D)
    ).contiguous()


def prefill_attn(qkv, k_cache, v_cache, positions, cfg, B, S, scale,
                 causal) -> torch.Tensor:
    """One-shot prefill attention of `qkv [B·S, (Hq+2Hk)·D]`: rope, write
    K/V to one layer's slabs, then causal attention over them — the
    hand-written MFMA flash-prefill kernel (gfx950) on the GPU,
    causal_attn_reference with the mask `causal` on the CPU. Returns
    [B·S, Hq·D]."""
    q, k, v = prefill_qkv(qkv, positions, cfg)
    write_prefill_kv(k_cache, v_cache, k, v, B, S)
    if q.is_cuda:
        return ops.prefill_attn(q, k_cache, v_cache, B, S, scale).reshape(
            B * S, -1
        )
    return causal_attn_reference(q, k_cache, v_cache, B, S, scale, causal)
