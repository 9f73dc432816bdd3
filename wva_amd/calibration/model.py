"""MI355X-native Llama-family decode engine for capacity calibration.

The reference's capacity model runs on parameters fit OFFLINE from vLLM
benchmarks on NVIDIA/MI300X hardware (docs/design/modeling-optimization.md
:46-84). This module is the MI355X-native replacement: a real bf16 decode
step of the target architecture (random-init weights — no network for
checkpoints) built from this repo's HIP/CDNA4 kernels (wva_amd.ops) with
GEMMs on hipBLASLt via torch.matmul, used to MEASURE ITL-vs-batch curves
and KV capacity on the actual GPU.

Single-GPU by design: TP over RCCL/xGMI shards these same GEMMs; the
autoscaler consumes per-(model, gpuCount) profiles, measured per TP degree
(capacity_store keys records by gpu_count).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import torch

from .. import ops
from .paged_kv import BlockAllocator, blocks_for, full_blocks


@dataclass
class LlamaConfig:
    name: str = "llama"
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_q_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    vocab_size: int = 128256
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5

    @property
    def q_size(self) -> int:
        return self.num_q_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_kv_heads * self.head_dim

    def kv_bytes_per_token(self, dtype_bytes: int = 2) -> int:
        return 2 * self.num_layers * self.kv_size * dtype_bytes

    def weight_bytes(self, dtype_bytes: int = 2) -> int:
        per_layer = (
            self.hidden_size * (self.q_size + 2 * self.kv_size)  # qkv
            + self.q_size * self.hidden_size  # o
            + 3 * self.hidden_size * self.intermediate_size  # gate/up/down
            + 2 * self.hidden_size  # norms
        )
        return dtype_bytes * (
            self.num_layers * per_layer
            + 2 * self.vocab_size * self.hidden_size  # embed + lm_head
            + self.hidden_size
        )


LLAMA_3_8B = LlamaConfig(
    name="meta-llama/Llama-3.1-8B",
    hidden_size=4096,
    intermediate_size=14336,
    num_layers=32,
    num_q_heads=32,
    num_kv_heads=8,
)

LLAMA_3_70B = LlamaConfig(
    name="meta-llama/Llama-3.1-70B",
    hidden_size=8192,
    intermediate_size=28672,
    num_layers=80,
    num_q_heads=64,
    num_kv_heads=8,
)

# Tiny config for smoke tests (same topology, minutes → milliseconds)
TINY = LlamaConfig(
    name="tiny-llama",
    hidden_size=1024,
    intermediate_size=2816,
    num_layers=2,
    num_q_heads=8,
    num_kv_heads=2,
    vocab_size=32000,
)


def _quantize_fp8(w: torch.Tensor):
    """Per-channel (rowwise) e4m3 quantization: (w_fp8 [N,K], scale [N]).
    Row scales commute with the GEMM's k-sum, so they fold into the
    output store exactly (csrc/skinny_gemm.hip W_FP8)."""
    scale = (w.abs().amax(dim=1).float() / 448.0).clamp_min(1e-12)  # [N]
    w8 = (
        (w.float() / scale[:, None]).clamp(-448.0, 448.0)
        .to(torch.float8_e4m3fn)
    )
    return w8.contiguous(), scale.contiguous()


class _DecoderLayer:
    def __init__(self, cfg: LlamaConfig, device, dtype, gen):
        h, std = cfg.hidden_size, 0.02
        def w(rows, cols):
            return torch.empty(rows, cols, device=device, dtype=dtype).normal_(
                0.0, std, generator=gen
            )

        self.input_norm = torch.ones(h, device=device, dtype=dtype)
        self.post_attn_norm = torch.ones(h, device=device, dtype=dtype)
        self.wqkv = w(cfg.q_size + 2 * cfg.kv_size, h)
        self.wo = w(h, cfg.q_size)
        self.w_gate_up = w(2 * cfg.intermediate_size, h)
        self.w_down = w(h, cfg.intermediate_size)


class LlamaDecodeModel:
    """Llama decode engine (plus prefill and chunked prefill) over a
    per-layer KV cache in one of two layouts:

    * kv_layout="contiguous" (default): a head-major slab
      [max_batch, Hk, max_seq, D] per layer.
    * kv_layout="paged": a pool [num_gpu_blocks, Hk, block_size, D] per layer
      and one block table [max_batch, max_seq / block_size] shared by all
      layers (vLLM's num_gpu_blocks x block_size layout). `num_gpu_blocks`
      defaults to max_batch * max_seq / block_size, the slab's bytes; a
      smaller pool holds many short sequences. Decode path only: the
      prefill-family methods raise NotImplementedError.
    """

    def __init__(
        self,
        cfg: LlamaConfig,
        max_batch: int = 256,
        max_seq: int = 2048,
        device: str = "cuda",
        seed: int = 0,
        kv_dtype: str = "bf16",
        weights_dtype: str = "bf16",
        kv_layout: str = "contiguous",
        block_size: int = 16,
        num_gpu_blocks: Optional[int] = None,
    ):
        self.cfg = cfg
        if kv_layout not in ("contiguous", "paged"):
            raise ValueError(
                f"kv_layout must be contiguous|paged, got {kv_layout}")
        self.kv_layout = kv_layout
        self.paged = kv_layout == "paged"
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        # fp8 weights: per-tensor e4m3 quantization, GEMMs via
        # torch._scaled_mm (W8A8 with dynamic per-tensor activation
        # scales) — the quantized-serving configuration (vLLM --dtype
        # fp8 analog); halves GEMM weight streaming. Calibration-variant
        # only: the headline bench stays bf16 weights.
        if weights_dtype not in ("bf16", "fp8"):
            raise ValueError(f"weights_dtype must be bf16|fp8")
        self.weights_dtype = weights_dtype
        # fp8 (e4m3) KV storage: half the attention HBM traffic, double
        # the KV capacity; compute stays bf16 (kernels up-convert at
        # fragment build — see csrc/attention.hip KV_FP8)
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype must be bf16|fp8, got {kv_dtype}")
        self.kv_dtype = kv_dtype
        self.cache_dtype = (
            torch.float8_e4m3fn if kv_dtype == "fp8" else torch.bfloat16
        )
        self.max_batch = max_batch
        self.max_seq = max_seq
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)

        self.embed = torch.empty(
            cfg.vocab_size, cfg.hidden_size, device=self.device, dtype=self.dtype
        ).normal_(0.0, 0.02, generator=gen)
        self.layers: List[_DecoderLayer] = [
            _DecoderLayer(cfg, self.device, self.dtype, gen)
            for _ in range(cfg.num_layers)
        ]
        self.final_norm = torch.ones(
            cfg.hidden_size, device=self.device, dtype=self.dtype
        )
        self.lm_head = torch.empty(
            cfg.vocab_size, cfg.hidden_size, device=self.device, dtype=self.dtype
        ).normal_(0.0, 0.02, generator=gen)
        if weights_dtype == "fp8":
            for layer in self.layers:
                for attr in ("wqkv", "wo", "w_gate_up", "w_down"):
                    setattr(layer, attr + "_q",
                            _quantize_fp8(getattr(layer, attr)))
                    setattr(layer, attr, None)  # free the bf16 copy
            self.lm_head_q = _quantize_fp8(self.lm_head)
            self.lm_head = None

        self.context_lens = torch.zeros(
            max_batch, dtype=torch.int32, device=self.device
        )
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        if self.paged:
            self._init_paged(block_size, num_gpu_blocks, seed)
            return
        # Head-major contiguous KV cache per layer: [B, Hk, S, D] — each
        # (sequence, kv-head) is one sequential HBM stream for the
        # attention kernel's tile staging (docs/mi355x-kernels.md)
        self.k_cache = [
            torch.zeros(
                max_batch, cfg.num_kv_heads, max_seq, cfg.head_dim,
                device=self.device, dtype=self.cache_dtype,
            )
            for _ in range(cfg.num_layers)
        ]
        self.v_cache = [torch.zeros_like(self.k_cache[0]) for _ in range(cfg.num_layers)]

    # --- paged KV cache ---

    def _init_paged(self, block_size, num_gpu_blocks, seed) -> None:
        cfg = self.cfg
        if block_size not in (16, 32, 64):
            raise ValueError(f"block_size must be 16|32|64, got {block_size}")
        if self.max_seq % block_size:
            raise ValueError(
                f"max_seq={self.max_seq} must be a multiple of "
                f"block_size={block_size}")
        self.block_size = block_size
        self.max_blocks = self.max_seq // block_size
        if num_gpu_blocks is None:
            num_gpu_blocks = self.max_batch * self.max_blocks
        if num_gpu_blocks < 1:
            raise ValueError(f"num_gpu_blocks must be >= 1")
        self.num_gpu_blocks = num_gpu_blocks
        self.allocator = BlockAllocator(num_gpu_blocks, seed=seed)
        self.k_pages = [
            torch.zeros(
                num_gpu_blocks, cfg.num_kv_heads, block_size, cfg.head_dim,
                device=self.device, dtype=self.cache_dtype,
            )
            for _ in range(cfg.num_layers)
        ]
        self.v_pages = [
            torch.zeros_like(self.k_pages[0]) for _ in range(cfg.num_layers)
        ]
        # One table for all layers. Its storage never changes: reset writes
        # into it in place, so a captured graph keeps seeing it. Unreserved
        # entries hold -1.
        self.block_tables = torch.full(
            (self.max_batch, self.max_blocks), -1, dtype=torch.int32,
            device=self.device,
        )

    def _reset_paged(self, batch, context_len, headroom, shared_prefix):
        bs = self.block_size
        if batch > self.max_batch:
            raise ValueError(f"batch={batch}, max_batch={self.max_batch}")
        reserve = (
            self.max_seq if headroom is None else context_len + headroom
        )
        if context_len > reserve or reserve > self.max_seq:
            raise ValueError(
                f"context {context_len}, reservation {reserve}, "
                f"max_seq={self.max_seq}")
        if shared_prefix < 0 or shared_prefix > context_len:
            raise ValueError(
                f"shared_prefix={shared_prefix} outside the context "
                f"{context_len}")
        per_seq = blocks_for(reserve, bs)
        shared = full_blocks(shared_prefix, bs)
        alloc = self.allocator
        alloc.reset()  # frees everything
        need = per_seq * batch - shared * max(batch - 1, 0)
        if need > alloc.num_free:
            raise RuntimeError(
                f"paged KV pool too small: {batch} sequences x {per_seq} "
                f"blocks ({shared} shared) need {need} blocks, "
                f"{alloc.num_free} free of {self.num_gpu_blocks}")
        tables = torch.full(
            (self.max_batch, self.max_blocks), -1, dtype=torch.int32)
        for b in range(batch):
            if b and shared:
                alloc.share(0, b, shared)
                alloc.allocate(b, per_seq - shared)
            else:
                alloc.allocate(b, per_seq)
            tables[b, :per_seq] = torch.tensor(
                alloc.blocks(b), dtype=torch.int32)
        self.block_tables.copy_(tables)  # in place
        self.context_lens.zero_()
        self.context_lens[:batch] = context_len
        # random-fill the pages that hold live rows
        live = blocks_for(context_len, bs)
        if batch == 0 or live == 0:
            return
        ids = torch.unique(tables[:batch, :live].reshape(-1)).long().to(
            self.device)
        shape = (ids.numel(),) + tuple(self.k_pages[0].shape[1:])
        for layer in range(self.cfg.num_layers):
            for pool in (self.k_pages, self.v_pages):
                fill = torch.randn(
                    shape, device=self.device, dtype=torch.bfloat16
                ).to(self.cache_dtype)
                ops._as_bytes(pool[layer])[ids] = ops._as_bytes(fill)

    def _decode_only(self) -> None:
        if self.paged:
            raise NotImplementedError("paged KV: decode path only")

    def reset(
        self,
        batch: int,
        context_len: int,
        headroom: Optional[int] = None,
        shared_prefix: int = 0,
    ) -> None:
        """Random-fill KV up to context_len for `batch` sequences.

        Paged layout: frees every block, then reserves
        ceil((context_len + headroom) / block_size) blocks per sequence
        (`headroom=None`: up to max_seq), handed out in a seeded, shuffled
        order so that sequences are scattered over the pool. With
        `shared_prefix > 0` the first shared_prefix // block_size blocks of
        every sequence are the same physical blocks (the prefix-cache-hit
        layout). Writes the block table in place and raises RuntimeError
        when the pool cannot cover the reservation. `headroom` and
        `shared_prefix` have no meaning for the contiguous layout."""
        if self.paged:
            self._reset_paged(batch, context_len, headroom, shared_prefix)
            return
        if headroom is not None or shared_prefix:
            raise ValueError(
                "headroom and shared_prefix need kv_layout=\"paged\"")
        self.context_lens.zero_()
        self.context_lens[:batch] = context_len
        for layer in range(self.cfg.num_layers):
            if self.cache_dtype == torch.bfloat16:
                self.k_cache[layer][:batch, :, :context_len].normal_(0.0, 1.0)
                self.v_cache[layer][:batch, :, :context_len].normal_(0.0, 1.0)
            else:  # normal_ unsupported on float8: generate + cast
                shape = self.k_cache[layer][:batch, :, :context_len].shape
                for cache in (self.k_cache, self.v_cache):
                    cache[layer][:batch, :, :context_len] = torch.randn(
                        shape, device=self.device, dtype=torch.bfloat16
                    ).to(self.cache_dtype)

    def _linear(self, x: torch.Tensor, layer, name: str) -> torch.Tensor:
        """bf16: ops.linear (hipBLASLt); fp8 weights: weight-only W8A16
        on the in-tree streaming kernel (activations stay bf16; weights
        up-convert in-fragment; per-channel scales fold into the store).
        W8A8 via torch._scaled_mm measured 2.4× slower at decode sizes
        (dynamic-quant launch overhead — docs/mi355x-kernels.md), so the
        weight-only form is the fp8 GEMM path."""
        if self.weights_dtype == "bf16":
            w = getattr(layer, name) if layer is not None else self.lm_head
            return ops.linear(x, w)
        w8, w_scale = (
            getattr(layer, name + "_q") if layer is not None else self.lm_head_q
        )
        # CPU: the dequantized matmul reference, at any size
        if not x.is_cuda or (x.shape[0] <= 64 and x.shape[1] % 128 == 0):
            return ops.skinny_linear(x, w8, w_scale)
        # large-M fallback (prefill-scale): dequantize and use hipBLASLt
        return (x @ (w8.to(x.dtype) * w_scale[:, None].to(x.dtype)).t())

    @torch.no_grad()
    def decode_step(self, token_ids: torch.Tensor) -> torch.Tensor:
        """One decode iteration for `B = len(token_ids)` sequences.
        Appends each sequence's new KV at position context_lens[b] and
        returns logits [B, vocab].

        Paged layout: the append and the attention go through the block
        table on the device; the step does no host work and no allocation,
        so it is graph-capturable as it is. Stepping a sequence past the
        blocks that `reset` reserved for it is the caller's error: by the
        kernels' addressing rules (an append without a page is skipped, an
        unreserved table entry is clamped into the pool) it produces wrong
        numbers and no bad access."""
        cfg = self.cfg
        B = token_ids.shape[0]
        positions = self.context_lens[:B].clone()

        ctx = positions + 1  # includes the new token (hoisted: one
        # launch per step, not per layer — profiling showed 32 redundant
        # int-add launches/step, profiles/decode8b_r2_kernel_stats.txt)
        x = self.embed.index_select(0, token_ids)  # [B, H]
        residual: Optional[torch.Tensor] = None

        for li, layer in enumerate(self.layers):
            if residual is None:
                residual = x.clone()
                h = ops.rmsnorm(x, layer.input_norm, None, cfg.rms_eps)
            else:
                h = ops.rmsnorm(x, layer.input_norm, residual, cfg.rms_eps)

            qkv = self._linear(h, layer, "wqkv")
            # fused: RoPE on the strided qkv row + KV-cache append
            if self.paged:
                tables = self.block_tables[:B]
                q = ops.rope_append_kv_paged(
                    qkv, self.k_pages[li], self.v_pages[li], tables,
                    positions, cfg.num_q_heads, cfg.num_kv_heads,
                    cfg.rope_theta,
                )
                attn = ops.paged_decode_attn(
                    q, self.k_pages[li], self.v_pages[li], tables, ctx,
                    self.scale,
                )
            else:
                q = ops.rope_append_kv(
                    qkv, self.k_cache[li][:B], self.v_cache[li][:B],
                    positions, cfg.num_q_heads, cfg.num_kv_heads,
                    cfg.rope_theta,
                )
                attn = ops.gqa_decode_attn(
                    q, self.k_cache[li][:B], self.v_cache[li][:B], ctx,
                    self.scale,
                )
            x = self._linear(attn.reshape(B, cfg.q_size), layer, "wo")

            h2 = ops.rmsnorm(x, layer.post_attn_norm, residual, cfg.rms_eps)
            gate_up = self._linear(h2, layer, "w_gate_up")
            act = ops.silu_mul_fused(gate_up)
            x = self._linear(act, layer, "w_down")

        final = ops.rmsnorm(x, self.final_norm, residual, cfg.rms_eps)
        logits = self._linear(final, None, "lm_head")
        self.context_lens[:B] += 1
        return logits

    @torch.no_grad()
    def prefill(
        self, token_ids: torch.Tensor, chunk_size: Optional[int] = None
    ) -> torch.Tensor:
        """Prefill `token_ids [B, S]`: computes all S positions in one
        pass (causal attention), fills the KV cache, sets context_lens=S
        and returns last-position logits [B, vocab].

        With an integer `chunk_size` the prompt is prefilled from an empty
        cache in chunks of that many tokens through `prefill_chunk` (the
        last chunk may be shorter) and the last chunk's logits are returned.

        Grounds the ServiceProfile's prefill_tokens_per_s (the TTFT
        model's input) with a measured value instead of a constant.
        Attention here is explicit matmul attention on hipBLASLt —
        prefill is GEMM-shaped compute (S×S scores), exactly what the
        library is for; the hand-written kernels cover the memory-bound
        decode path. RMSNorm/RoPE/SwiGLU reuse the HIP kernels (they are
        row-shaped and batch-size-agnostic).
        """
        self._decode_only()
        if chunk_size is not None:
            return self._prefill_chunked(token_ids, int(chunk_size))
        cfg = self.cfg
        if self.weights_dtype != "bf16":
            raise NotImplementedError(
                "prefill with fp8 weights is not implemented (the "
                "weight-only fp8 mode targets decode; prefill would "
                "dequantize every layer per pass)"
            )
        B, S = token_ids.shape
        T = B * S
        if S > self.max_seq:
            raise ValueError(f"S={S} exceeds max_seq={self.max_seq}")
        positions = (
            torch.arange(S, device=self.device, dtype=torch.int32)
            .repeat(B)
        )  # [T] per-token position

        x = self.embed.index_select(0, token_ids.reshape(-1))  # [T, H]
        residual: Optional[torch.Tensor] = None

        causal = torch.full(
            (S, S), float("-inf"), device=self.device, dtype=torch.float32
        ).triu(1)

        for li, layer in enumerate(self.layers):
            if residual is None:
                residual = x.clone()
                h = ops.rmsnorm(x, layer.input_norm, None, cfg.rms_eps)
            else:
                h = ops.rmsnorm(x, layer.input_norm, residual, cfg.rms_eps)

            qkv = h @ layer.wqkv.t()  # [T, (Hq+2Hk)·D] — prefill M is large
            q, k, v = qkv.split(
                [cfg.q_size, cfg.kv_size, cfg.kv_size], dim=-1
            )
            q = q.reshape(T, cfg.num_q_heads, cfg.head_dim).contiguous()
            k = k.reshape(T, cfg.num_kv_heads, cfg.head_dim).contiguous()
            ops.rope(q, k, positions, cfg.rope_theta)  # in-place HIP kernel
            v = v.reshape(T, cfg.num_kv_heads, cfg.head_dim)

            # append to the head-major cache [B, Hk, S_max, D]
            k_b = k.reshape(B, S, cfg.num_kv_heads, cfg.head_dim)
            v_b = v.reshape(B, S, cfg.num_kv_heads, cfg.head_dim)
            self.k_cache[li][:B, :, :S].copy_(k_b.permute(0, 2, 1, 3))
            self.v_cache[li][:B, :, :S].copy_(v_b.permute(0, 2, 1, 3))

            if q.is_cuda:
                # hand-written MFMA flash-prefill kernel (gfx950)
                attn = ops.prefill_attn(
                    q, self.k_cache[li], self.v_cache[li], B, S, self.scale
                ).reshape(T, cfg.q_size)
            else:
                # CPU numerics reference: explicit causal matmul attention
                G = cfg.num_q_heads // cfg.num_kv_heads
                qh = (
                    q.reshape(B, S, cfg.num_kv_heads, G, cfg.head_dim)
                    .permute(0, 2, 3, 1, 4)
                    .reshape(B * cfg.num_kv_heads * G, S, cfg.head_dim)
                )
                kh = (
                    self.k_cache[li][:B, :, :S].to(self.dtype)
                    .unsqueeze(2)
                    .expand(B, cfg.num_kv_heads, G, S, cfg.head_dim)
                    .reshape(B * cfg.num_kv_heads * G, S, cfg.head_dim)
                )
                vh = (
                    self.v_cache[li][:B, :, :S].to(self.dtype)
                    .unsqueeze(2)
                    .expand(B, cfg.num_kv_heads, G, S, cfg.head_dim)
                    .reshape(B * cfg.num_kv_heads * G, S, cfg.head_dim)
                )
                scores = (
                    torch.bmm(qh, kh.transpose(1, 2)).float() * self.scale
                    + causal
                )
                p = torch.softmax(scores, dim=-1).to(self.dtype)
                attn = torch.bmm(p, vh)  # [B*Hq, S, D]
                attn = (
                    attn.reshape(B, cfg.num_q_heads, S, cfg.head_dim)
                    .permute(0, 2, 1, 3)
                    .reshape(T, cfg.q_size)
                ).contiguous()
            x = attn @ layer.wo.t()

            h2 = ops.rmsnorm(x, layer.post_attn_norm, residual, cfg.rms_eps)
            gate_up = h2 @ layer.w_gate_up.t()
            act = ops.silu_mul_fused(gate_up)
            x = act @ layer.w_down.t()

        final = ops.rmsnorm(x, self.final_norm, residual, cfg.rms_eps)
        last = final.reshape(B, S, cfg.hidden_size)[:, -1].contiguous()
        logits = last @ self.lm_head.t()
        self.context_lens.zero_()
        self.context_lens[:B] = S
        return logits

    # --- chunked prefill: a block of new tokens per sequence attends to a
    # KV prefix that is already in the cache (vLLM's default scheduling) ---

    def _prefill_chunked(
        self, token_ids: torch.Tensor, chunk_size: int
    ) -> torch.Tensor:
        B, S = token_ids.shape
        if chunk_size < 1:
            raise ValueError(f"chunk_size must be >= 1, got {chunk_size}")
        if S > self.max_seq:
            raise ValueError(f"S={S} exceeds max_seq={self.max_seq}")
        self.context_lens.zero_()
        logits = None
        for start in range(0, S, chunk_size):
            logits = self.prefill_chunk(
                token_ids[:, start:start + chunk_size].contiguous()
            )
        return logits

    @torch.no_grad()
    def prefill_chunk(self, token_ids: torch.Tensor) -> torch.Tensor:
        """Continue sequences 0..B-1 by a chunk `token_ids [B, C]` from
        their own `context_lens[b]` (which may differ): the chunk's K/V go
        to cache rows context_lens[b] .. +C-1, its queries attend to the
        cached prefix plus the chunk (ops.extend_attn), context_lens[:B]
        advances by C. Returns the chunk's last-position logits
        [B, vocab]. Everything per-sequence stays on the device; the
        caller keeps context_lens[b] + C within max_seq."""
        self._decode_only()
        return self._chunk_step(None, token_ids)

    @torch.no_grad()
    def mixed_step(
        self, decode_tokens: torch.Tensor, chunk_tokens: torch.Tensor
    ) -> torch.Tensor:
        """One iteration that mixes decode and chunked prefill: cache rows
        0..Bd-1 decode one token each (`decode_tokens [Bd]`), rows
        Bd..Bd+Bp-1 prefill a chunk each (`chunk_tokens [Bp, C]`). All
        Bd + Bp*C token rows share the norms and linears (one pass over the
        weights); only attention splits by row range. Returns logits
        [Bd+Bp, vocab]: the decode rows, then each chunk's last position.
        context_lens advances by 1 and by C respectively."""
        self._decode_only()
        return self._chunk_step(decode_tokens, chunk_tokens)

    def _chunk_step(
        self, decode_tokens: Optional[torch.Tensor], chunk_tokens: torch.Tensor
    ) -> torch.Tensor:
        cfg = self.cfg
        if self.weights_dtype != "bf16":
            raise NotImplementedError(
                "chunked prefill with fp8 weights is not implemented"
            )
        Bd = 0 if decode_tokens is None else decode_tokens.shape[0]
        Bp, C = chunk_tokens.shape
        if C < 1 or C > self.max_seq:
            raise ValueError(f"chunk of {C} tokens, max_seq={self.max_seq}")
        if Bd + Bp > self.max_batch:
            raise ValueError(f"{Bd}+{Bp} sequences, max_batch={self.max_batch}")
        T = Bp * C
        Hk, D = cfg.num_kv_heads, cfg.head_dim

        # per-call index tensors, built on the device (no host read)
        prefix = self.context_lens[Bd:Bd + Bp].clone()  # [Bp] int32
        pos = prefix[:, None] + torch.arange(
            C, device=self.device, dtype=torch.int32
        )  # [Bp, C] absolute positions
        positions = pos.reshape(-1)
        # cache rows of the chunk; clamped so that a write stays in the slab
        row_idx = pos.long().clamp_(max=self.max_seq - 1)
        seq_idx = torch.arange(Bd, Bd + Bp, device=self.device)[:, None]
        tokens = chunk_tokens.reshape(-1)
        if Bd:
            tokens = torch.cat([decode_tokens, tokens])

        def write_kv(cache, new):  # new [Bp, C, Hk, D], already cache dtype
            if cache.dtype != self.dtype:  # e4m3: indexed write as bytes
                cache, new = cache.view(torch.uint8), new.view(torch.uint8)
            cache[seq_idx, :, row_idx] = new

        def chunk_attn(li, q, k, v):
            write_kv(self.k_cache[li],
                     k.reshape(Bp, C, Hk, D).to(self.cache_dtype))
            write_kv(self.v_cache[li],
                     v.reshape(Bp, C, Hk, D).to(self.cache_dtype))
            return ops.extend_attn(
                q, self.k_cache[li][Bd:Bd + Bp], self.v_cache[li][Bd:Bd + Bp],
                prefix, C, self.scale,
            )

        final = self._mixed_layers(tokens, Bd, T, positions, chunk_attn)
        last = final[Bd:].reshape(Bp, C, cfg.hidden_size)[:, -1]
        logits = torch.cat([final[:Bd], last]) @ self.lm_head.t()
        self.context_lens[:Bd] += 1
        self.context_lens[Bd:Bd + Bp] += C
        return logits

    def _mixed_layers(self, tokens, Bd, T, positions, chunk_attn):
        """The layer loop of one mixed iteration over `tokens [Bd + T]`:
        rows 0..Bd-1 decode on cache rows 0..Bd-1 (rope_append_kv +
        gqa_decode_attn), rows Bd.. are T prefill rows at `positions [T]`
        whose K/V write and attention are `chunk_attn(li, q, k, v)` (q, k
        roped [T, H*, D], v [T, Hk, D]) -> [T, Hq, D]. Norms and linears
        run once over all rows. Returns the final-normed hidden states."""
        cfg = self.cfg
        Hq, Hk, D = cfg.num_q_heads, cfg.num_kv_heads, cfg.head_dim
        if Bd:
            d_pos = self.context_lens[:Bd].clone()
            d_ctx = d_pos + 1
        x = self.embed.index_select(0, tokens)  # [Bd + T, H]
        residual: Optional[torch.Tensor] = None
        for li, layer in enumerate(self.layers):
            if residual is None:
                residual = x.clone()
                h = ops.rmsnorm(x, layer.input_norm, None, cfg.rms_eps)
            else:
                h = ops.rmsnorm(x, layer.input_norm, residual, cfg.rms_eps)
            qkv = h @ layer.wqkv.t()

            q, k, v = qkv[Bd:].split(
                [cfg.q_size, cfg.kv_size, cfg.kv_size], dim=-1
            )
            q = q.reshape(T, Hq, D).contiguous()
            k = k.reshape(T, Hk, D).contiguous()
            ops.rope(q, k, positions, cfg.rope_theta)
            attn = chunk_attn(li, q, k, v.reshape(T, Hk, D)).reshape(
                T, cfg.q_size
            )
            if Bd:
                qd = ops.rope_append_kv(
                    qkv[:Bd], self.k_cache[li][:Bd], self.v_cache[li][:Bd],
                    d_pos, Hq, Hk, cfg.rope_theta,
                )
                attn_d = ops.gqa_decode_attn(
                    qd, self.k_cache[li][:Bd], self.v_cache[li][:Bd], d_ctx,
                    self.scale,
                )
                attn = torch.cat([attn_d.reshape(Bd, cfg.q_size), attn])
            x = attn @ layer.wo.t()

            h2 = ops.rmsnorm(x, layer.post_attn_norm, residual, cfg.rms_eps)
            gate_up = h2 @ layer.w_gate_up.t()
            act = ops.silu_mul_fused(gate_up)
            x = act @ layer.w_down.t()

        return ops.rmsnorm(x, self.final_norm, residual, cfg.rms_eps)

    @torch.no_grad()
    def ragged_step(
        self,
        decode_tokens: Optional[torch.Tensor],
        chunk_tokens: torch.Tensor,
        chunk_lens: torch.Tensor,
        max_chunk: int,
    ) -> torch.Tensor:
        """One iteration with chunks of unequal length: cache rows 0..Bd-1
        decode one token each (`decode_tokens [Bd]` or None), rows
        Bd..Bd+Bp-1 each continue by chunk_lens[b] tokens from their own
        context_lens. `chunk_tokens [T]` packs the chunks one after another
        (T >= sum of chunk_lens >= 1; rows past that sum are computed but
        written nowhere), `chunk_lens [Bp]` is int32 on the device and `max_chunk`
        its host-side upper bound. All Bd + T token rows share the norms and
        linears; the chunks share one ops.extend_attn_ragged launch per
        layer. Nothing per-sequence is read on the host. Returns logits
        [Bd+Bp, vocab]: the decode rows, then each sequence's last chunk row
        (unspecified for a sequence with chunk_lens[b] == 0, whose
        context_lens and cache rows stay as they are). context_lens advances
        by 1 and by chunk_lens respectively; the caller keeps
        context_lens[b] + chunk_lens[b] within max_seq."""
        self._decode_only()
        if self.weights_dtype != "bf16":
            raise NotImplementedError(
                "chunked prefill with fp8 weights is not implemented"
            )
        Bd = 0 if decode_tokens is None else decode_tokens.shape[0]
        Bp, T = chunk_lens.shape[0], chunk_tokens.shape[0]
        if max_chunk < 1 or max_chunk > self.max_seq:
            raise ValueError(
                f"max_chunk={max_chunk}, max_seq={self.max_seq}")
        if Bp < 1 or T < 1:
            raise ValueError("ragged_step needs a chunk sequence and a row")
        if Bd + Bp > self.max_batch:
            raise ValueError(f"{Bd}+{Bp} sequences, max_batch={self.max_batch}")

        # per-row sequence index and position, built on the device
        lens = chunk_lens.to(torch.int32).clamp(0, max_chunk)
        ends = torch.cumsum(lens, 0)             # int64
        q_starts = ends - lens
        prefix = self.context_lens[Bd:Bd + Bp].clone()  # [Bp] int32
        rows = torch.arange(T, device=self.device)
        owned = rows < ends[-1]
        # a row past the packed chunks rewrites row 0's K/V at row 0's place
        src = torch.where(owned, rows, torch.zeros_like(rows))
        seq = torch.searchsorted(ends, src, right=True).clamp_(max=Bp - 1)
        pos = prefix[seq] + (src - q_starts[seq])  # [T] absolute positions
        positions = pos.to(torch.int32)
        row_idx = pos.long().clamp_(max=self.max_seq - 1)
        seq_idx = seq + Bd
        tokens = chunk_tokens
        if Bd:
            tokens = torch.cat([decode_tokens, tokens])

        def write_kv(cache, new):  # new [T, Hk, D], already cache dtype
            if cache.dtype != self.dtype:  # e4m3: indexed write as bytes
                cache, new = cache.view(torch.uint8), new.view(torch.uint8)
            cache[seq_idx, :, row_idx] = new.index_select(0, src)

        def chunk_attn(li, q, k, v):
            write_kv(self.k_cache[li], k.to(self.cache_dtype))
            write_kv(self.v_cache[li], v.to(self.cache_dtype))
            return ops.extend_attn_ragged(
                q, self.k_cache[li][Bd:Bd + Bp], self.v_cache[li][Bd:Bd + Bp],
                prefix, lens, max_chunk, self.scale,
            )

        final = self._mixed_layers(tokens, Bd, T, positions, chunk_attn)
        last = final[Bd:].index_select(0, (ends - 1).clamp_(0, T - 1))
        logits = torch.cat([final[:Bd], last]) @ self.lm_head.t()
        self.context_lens[:Bd] += 1
        self.context_lens[Bd:Bd + Bp] += lens
        return logits
