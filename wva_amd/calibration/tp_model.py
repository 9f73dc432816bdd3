"""Tensor-parallel Llama decode engine over RCCL/xGMI.

The autoscaler's capacity model is TP-aware: service-rate records are
keyed by (model, accelerator, gpuCount) and the α of the ITL model grows
with the per-layer all-reduce term on xGMI. This engine
measures that directly: Megatron-style TP sharding of the calibration
decode model with `torch.distributed` all-reduce (backend "nccl" IS RCCL
on ROCm; "gloo" for CPU tests).

Sharding (standard column/row parallel):
  * wqkv, w_gate_up: column-parallel — each rank owns Hq/N query heads,
    Hk/N kv heads and I/N intermediate columns; no communication in.
  * wo, w_down: row-parallel — partial sums all-reduced (2 all-reduces
    per layer, ring over 7×153 GB/s xGMI links intra-node).
  * Attention + KV cache: local to the rank's heads.
  * Embedding/lm_head replicated (calibration-scale simplification).

The layer weights, KV slab, layer loop and decode attention block are the
single-GPU engine's (calibration/blocks.py), given this rank's shard sizes.

Run per-TP calibration on an 8-GPU node with:
  torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node N \
      scripts/calibrate_tp.py --model 8b
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.distributed as dist

from .. import ops
from . import blocks
from .model import LlamaConfig


class TPShardInfo:
    def __init__(self, cfg: LlamaConfig, tp: int, rank: int):
        if cfg.num_q_heads % tp or cfg.num_kv_heads % tp:
            raise ValueError(
                f"heads ({cfg.num_q_heads}/{cfg.num_kv_heads}) must divide "
                f"by tp={tp}"
            )
        if cfg.intermediate_size % tp:
            raise ValueError("intermediate_size must divide by tp")
        self.tp = tp
        self.rank = rank
        self.num_q_heads = cfg.num_q_heads // tp
        self.num_kv_heads = cfg.num_kv_heads // tp
        self.inter = cfg.intermediate_size // tp
        self.q_size = self.num_q_heads * cfg.head_dim
        self.kv_size = self.num_kv_heads * cfg.head_dim


class TPLlamaDecodeModel:
    """One rank of a TP=N decode engine; construct once per process."""

    def __init__(
        self,
        cfg: LlamaConfig,
        max_batch: int = 64,
        max_seq: int = 1024,
        device: str = "cuda",
        seed: int = 0,
        group: Optional[dist.ProcessGroup] = None,
        kv_dtype: str = "bf16",
    ):
        self.cfg = cfg
        self.kv_dtype = kv_dtype
        self.cache_dtype = (
            torch.float8_e4m3fn if kv_dtype == "fp8" else torch.bfloat16
        )
        self.group = group
        self.tp = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.shard = TPShardInfo(cfg, self.tp, self.rank)
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        self.max_batch = max_batch
        self.max_seq = max_seq
        gen = torch.Generator(device=self.device)
        # same seed on every rank for the replicated parts; shard-unique
        # seed for the sharded weights
        gen.manual_seed(seed)
        draw = (self.device, self.dtype, gen)
        self.embed = blocks.w(cfg.vocab_size, cfg.hidden_size, *draw)
        gen.manual_seed(seed * 1000 + self.rank + 1)
        shard = self.shard
        self.layers = [
            blocks.DenseLayer(
                cfg.hidden_size, shard.q_size, shard.kv_size, shard.inter,
                *draw,
            )
            for _ in range(cfg.num_layers)
        ]
        self.final_norm = torch.ones(
            cfg.hidden_size, device=self.device, dtype=self.dtype
        )
        gen.manual_seed(seed)
        self.lm_head = blocks.w(cfg.vocab_size, cfg.hidden_size, *draw)

        self.k_cache, self.v_cache = blocks.alloc_kv_slabs(
            cfg.num_layers, max_batch, shard.num_kv_heads, max_seq,
            cfg.head_dim, self.device, self.cache_dtype,
        )
        self.context_lens = torch.zeros(
            max_batch, dtype=torch.int32, device=self.device
        )
        self.scale = 1.0 / math.sqrt(cfg.head_dim)

    def _all_reduce(self, x: torch.Tensor) -> torch.Tensor:
        if self.tp > 1:
            dist.all_reduce(x, group=self.group)
        return x

    def reset(self, batch: int, context_len: int) -> None:
        blocks.reset_kv_slabs(
            self.context_lens, self.k_cache, self.v_cache, batch, context_len
        )

    @torch.no_grad()
    def decode_step(self, token_ids: torch.Tensor) -> torch.Tensor:
        cfg, shard = self.cfg, self.shard
        B = token_ids.shape[0]
        positions = self.context_lens[:B].clone()

        ctx = positions + 1  # includes the new token (hoisted: one
        # launch per step, not per layer — profiling showed 32 redundant
        # int-add launches/step, profiles/decode8b_r2_kernel_stats.txt)
        x = self.embed.index_select(0, token_ids)

        def attn(li, layer, h):
            a = blocks.decode_attn(
                ops.linear(h, layer.wqkv),  # local heads only
                self.k_cache[li], self.v_cache[li], positions, ctx,
                shard.num_q_heads, shard.num_kv_heads, cfg.rope_theta,
                self.scale,
            )
            # row-parallel o-proj: partials all-reduced over RCCL/xGMI
            return self._all_reduce(ops.linear(a, layer.wo))

        def mlp(layer, h2):
            act = ops.silu_mul_fused(ops.linear(h2, layer.w_gate_up))
            return self._all_reduce(ops.linear(act, layer.w_down))

        final = blocks.run_layers(
            self.layers, x, self.final_norm, cfg.rms_eps, attn, mlp
        )
        logits = ops.linear(final, self.lm_head)
        self.context_lens[:B] += 1
        return logits
