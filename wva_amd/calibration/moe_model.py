"""Mixtral-family (sparse MoE) decode engine for MI355X calibration.

BASELINE config #4 pairs Llama-3-8B with Mixtral-8×7B under service-class
priorities; this engine provides the measured service profile for the MoE
family the same way calibration/model.py does for dense Llama. Mixtral
8×7B bf16 is ≈ 94 GB of weights — resident on a single 288 GB MI355X (a
192 GB MI300X needs TP=2), which is itself an MI355X capacity statement
the cost solver exploits.

Architecture: Llama-style attention (the layer loop, attention blocks and
KV slab of calibration/blocks.py, shared with the Llama engines: fused
add-RMSNorm, rope_append_kv, GQA decode attention) + top-2 routed expert
MLPs. At decode batches the expert MLPs run DENSE-batched — one hipBLASLt
strided-batched GEMM pair per layer over all experts (see _moe_mlp) —
because decode MoE is weight-streaming-bound and the sparse gather path's
per-expert `nonzero()` syncs dominate. `moe_impl="grouped"` instead routes
on the device and multiplies only the routed (token, expert) pairs
(ops.moe_mlp, csrc/moe.hip): what a serving engine's fused MoE does.
With `weights_dtype="fp8"` that path keeps the experts (≈ 90 of the 94 GB)
as weight-only e4m3 with per-row scales and nothing in bf16.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .. import ops
from . import blocks
from .model import LlamaConfig


@dataclass
class MixtralConfig(LlamaConfig):
    name: str = "mistralai/Mixtral-8x7B"
    vocab_size: int = 32000
    rope_theta: float = 1000000.0
    num_experts: int = 8
    top_k: int = 2

    def weight_bytes(self, dtype_bytes: int = 2) -> int:
        # the dense layer's one MLP becomes num_experts of them + a router
        per_layer_extra = (
            (self.num_experts - 1) * 3 * self.hidden_size
            * self.intermediate_size
            + self.hidden_size * self.num_experts
        )
        return super().weight_bytes(dtype_bytes) + (
            dtype_bytes * self.num_layers * per_layer_extra
        )


MIXTRAL_8X7B = MixtralConfig()

TINY_MOE = MixtralConfig(
    name="tiny-mixtral",
    hidden_size=512,
    intermediate_size=1024,
    num_layers=2,
    num_q_heads=4,
    num_kv_heads=1,
    vocab_size=1000,
    num_experts=4,
    top_k=2,
)


class _MoELayer(blocks.AttnLayer):
    def __init__(self, cfg: MixtralConfig, device, dtype, gen, fp8=False):
        h, inter = cfg.hidden_size, cfg.intermediate_size
        super().__init__(h, cfg.q_size, cfg.kv_size, device, dtype, gen)
        self.w_router = blocks.w(cfg.num_experts, h, device, dtype, gen)
        if fp8:
            # same draws in the same order as below, quantised expert by
            # expert: a layer never holds a second, bf16 copy of its experts
            self.w_gate_up_stacked, self.w_gate_up_scale = self._draw_fp8(
                cfg.num_experts, 2 * inter, h, device, dtype, gen)
            self.w_down_stacked, self.w_down_scale = self._draw_fp8(
                cfg.num_experts, h, inter, device, dtype, gen)
            return
        self.set_expert_weights(
            torch.stack([
                blocks.w(2 * inter, h, device, dtype, gen)
                for _ in range(cfg.num_experts)
            ]),
            torch.stack([
                blocks.w(h, inter, device, dtype, gen)
                for _ in range(cfg.num_experts)
            ]),
        )

    @staticmethod
    def _draw_fp8(num_experts, rows, cols, device, dtype, gen):
        """(e4m3 stack [E, rows, cols], fp32 scales [E, rows]) of seeded
        expert weights (ops.quantize_moe_weights)."""
        q = torch.empty(
            num_experts, rows, cols, device=device, dtype=torch.float8_e4m3fn
        )
        scale = torch.empty(
            num_experts, rows, device=device, dtype=torch.float32
        )
        for e in range(num_experts):
            q_e, s_e = ops.quantize_moe_weights(
                blocks.w(rows, cols, device, dtype, gen).unsqueeze(0)
            )
            q[e], scale[e] = q_e[0], s_e[0]
        return q, scale

    def set_expert_weights(self, gate_up_stacked, down_stacked) -> None:
        """Replace expert weights, recomputing every derived operand
        (tests copy weights between devices through this)."""
        # experts as STACKED tensors [E, 2I, H] / [E, H, I]: the decode
        # path runs them as one strided-batched GEMM pair per layer (see
        # MixtralDecodeModel._moe_mlp); per-expert views kept for the
        # sparse reference path
        self.w_gate_up_stacked = gate_up_stacked
        self.w_down_stacked = down_stacked
        self.w_gate_up_scale = self.w_down_scale = None  # bf16 operands
        self.w_gate_up = list(gate_up_stacked)
        self.w_down = list(down_stacked)
        # dense-path operands (no transposed VIEWS at run time — hipBLASLt
        # takes a catastrophically slow route for strided-batched GEMMs on
        # transposed views of these shapes; measured 11 ms/layer):
        #  * gate_up runs as ONE flat GEMM against [E·2I, H] (a free view)
        #  * down runs as bmm against a pre-transposed CONTIGUOUS [E, I, H]
        e2i, h = (
            gate_up_stacked.shape[0] * gate_up_stacked.shape[1],
            gate_up_stacked.shape[2],
        )
        self.w_gate_up_flat = gate_up_stacked.reshape(e2i, h)
        self.w_down_t = down_stacked.transpose(1, 2).contiguous()


# expert-MLP implementations selectable per engine:
#   auto    — dense for decode B ≤ 64, sparse above and for prefill
#   dense   — every expert on every token (one GEMM pair per layer)
#   sparse  — per-expert gather with a host sync per expert
#   grouped — device-side routing + grouped MFMA GEMMs (ops.moe_mlp):
#             only routed experts stream, no host sync, graph-capturable
MOE_IMPLS = ("auto", "dense", "sparse", "grouped")


class MixtralDecodeModel:
    """Mixtral decode and one-shot prefill engine over the contiguous KV
    slab (blocks.alloc_kv_slabs)."""

    def __init__(
        self,
        cfg: MixtralConfig,
        max_batch: int = 256,
        max_seq: int = 2048,
        device: str = "cuda",
        seed: int = 0,
        kv_dtype: str = "bf16",
        moe_impl: str = "auto",
        weights_dtype: str = "bf16",
    ):
        if moe_impl not in MOE_IMPLS:
            raise ValueError(
                f"moe_impl must be one of {MOE_IMPLS}, got {moe_impl!r}"
            )
        if weights_dtype not in ("bf16", "fp8"):
            raise ValueError(
                f'weights_dtype must be "bf16" or "fp8", got {weights_dtype!r}'
            )
        if weights_dtype == "fp8" and moe_impl != "grouped":
            # the dense and sparse paths multiply bf16 operands; keeping a
            # bf16 copy for them would give the halved memory back
            raise ValueError(
                'weights_dtype="fp8" needs moe_impl="grouped", got '
                f"{moe_impl!r}"
            )
        self.cfg = cfg
        self.moe_impl = moe_impl
        # "fp8": weight-only e4m3 expert stacks with per-row scales (W8A16,
        # ops.moe_mlp); attention, router, embeddings and lm_head stay bf16
        self.weights_dtype = weights_dtype
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        self.kv_dtype = kv_dtype
        self.cache_dtype = (
            torch.float8_e4m3fn if kv_dtype == "fp8" else torch.bfloat16
        )
        self.max_batch = max_batch
        self.max_seq = max_seq
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)

        draw = (self.device, self.dtype, gen)
        self.embed = blocks.w(cfg.vocab_size, cfg.hidden_size, *draw)
        self.layers = [
            _MoELayer(cfg, *draw, fp8=weights_dtype == "fp8")
            for _ in range(cfg.num_layers)
        ]
        self.final_norm = torch.ones(
            cfg.hidden_size, device=self.device, dtype=self.dtype
        )
        self.lm_head = blocks.w(cfg.vocab_size, cfg.hidden_size, *draw)

        self.k_cache, self.v_cache = blocks.alloc_kv_slabs(
            cfg.num_layers, max_batch, cfg.num_kv_heads, max_seq,
            cfg.head_dim, self.device, self.cache_dtype,
        )
        self.context_lens = torch.zeros(
            max_batch, dtype=torch.int32, device=self.device
        )
        self.scale = 1.0 / math.sqrt(cfg.head_dim)

    def reset(self, batch: int, context_len: int) -> None:
        blocks.reset_kv_slabs(
            self.context_lens, self.k_cache, self.v_cache, batch, context_len
        )

    def _moe_mlp(self, layer: _MoELayer, h2: torch.Tensor) -> torch.Tensor:
        """MoE MLP; dense-batched for decode batches (B ≤ 64).

        Decode MoE on MI355X is weight-streaming-bound: once B ≳
        top_k·E/2 every expert's weights stream from HBM each step, so a
        GEMM over all B tokens costs the same as one over the ~B·k/E
        routed tokens. Running every expert on the full batch as ONE
        strided-batched GEMM pair per layer (torch.bmm → hipBLASLt
        strided-batched) replaces 3·E launches + a per-expert
        `mask.nonzero()` that forces a device→host sync — E·layers = 256
        pipeline stalls per step, the dominant cost of the sparse path
        (measured 48.6 ms at B=64 vs an ~11 ms streaming floor,
        profiles/calibration_mixtral.json). Non-routed expert outputs are
        zero-weighted in the combine einsum. Larger batches take the
        sparse gather path (compute starts to matter), which is also the
        numerics reference for the GPU tests.
        """
        return self._moe_mlp_impl(layer, h2, dense=h2.shape[0] <= 64)

    def _moe_mlp_impl(self, layer: _MoELayer, h2, dense: bool):
        """Route and run the expert MLP; `dense` is what moe_impl="auto"
        picks for this call (decode B ≤ 64), the forced impls ignore it."""
        cfg = self.cfg
        router_logits = (h2.float() @ layer.w_router.t().float())  # [B, E]
        if self.moe_impl == "grouped":
            return ops.moe_mlp(
                h2, router_logits, layer.w_gate_up_stacked,
                layer.w_down_stacked, cfg.top_k,
                w_gate_up_scale=layer.w_gate_up_scale,
                w_down_scale=layer.w_down_scale,
            )
        weights, selected = torch.topk(router_logits, cfg.top_k, dim=-1)
        weights = torch.softmax(weights, dim=-1).to(h2.dtype)  # [B, K]

        if self.moe_impl != "auto":
            dense = self.moe_impl == "dense"
        if dense:
            return self._moe_mlp_dense(layer, h2, weights, selected)
        return self._moe_mlp_sparse(layer, h2, weights, selected)

    def _moe_mlp_dense(self, layer, h2, weights, selected):
        cfg = self.cfg
        B = h2.shape[0]
        E, I = cfg.num_experts, cfg.intermediate_size
        w_full = torch.zeros(B, E, device=h2.device, dtype=h2.dtype)
        w_full.scatter_(1, selected, weights)
        # all experts' gate_up as one plain GEMM: [B, H] @ [H, E*2I]
        gate_up = ops.linear(h2, layer.w_gate_up_flat)  # [B, E*2I]
        act = ops.silu_mul_fused(
            gate_up.reshape(B * E, 2 * I)
        ).reshape(B, E, I)
        # down per expert: bmm over contiguous pre-transposed weights
        y = torch.bmm(act.transpose(0, 1).contiguous(), layer.w_down_t)
        # combine: broadcast-mul + sum — NOT einsum, which routes this
        # 4 MB contraction through an 11 ms path on ROCm (measured;
        # profiles/moe_dense_breakdown.txt)
        return (y * w_full.t().unsqueeze(-1)).sum(dim=0)

    def _moe_mlp_sparse(self, layer, h2, weights, selected):
        cfg = self.cfg
        out = torch.zeros_like(h2)
        for e in range(cfg.num_experts):
            # tokens with expert e among their top-k
            mask = selected == e  # [B, K]
            token_idx, k_idx = mask.nonzero(as_tuple=True)
            if token_idx.numel() == 0:
                continue
            x_e = h2.index_select(0, token_idx)
            gate_up = ops.linear(x_e, layer.w_gate_up[e])
            act = ops.silu_mul_fused(gate_up)
            y = ops.linear(act, layer.w_down[e])
            w_e = weights[token_idx, k_idx].unsqueeze(-1)
            out.index_add_(0, token_idx, (y * w_e).to(out.dtype))
        return out

    @torch.no_grad()
    def decode_step(self, token_ids: torch.Tensor) -> torch.Tensor:
        cfg = self.cfg
        B = token_ids.shape[0]
        positions = self.context_lens[:B].clone()
        ctx = positions + 1  # hoisted out of the layer loop

        x = self.embed.index_select(0, token_ids)

        def attn(li, layer, h):
            a = blocks.decode_attn(
                ops.linear(h, layer.wqkv), self.k_cache[li], self.v_cache[li],
                positions, ctx, cfg.num_q_heads, cfg.num_kv_heads,
                cfg.rope_theta, self.scale,
            )
            return ops.linear(a, layer.wo)

        final = blocks.run_layers(
            self.layers, x, self.final_norm, cfg.rms_eps, attn, self._moe_mlp
        )
        logits = ops.linear(final, self.lm_head)
        self.context_lens[:B] += 1
        return logits

    @torch.no_grad()
    def prefill(self, token_ids: torch.Tensor) -> torch.Tensor:
        """Prefill [B, S]: one causal pass (MFMA flash-prefill kernel on
        GPU), fills the KV caches, returns last-position logits.

        The expert MLP takes the SPARSE gather path here: prefill is
        compute-bound (each expert sees ~T·k/E of T = B·S tokens, and
        T is large), so dense-batching would genuinely 4× the MLP FLOPs —
        the opposite trade from decode (see _moe_mlp). The per-expert
        `nonzero()` syncs amortize over one large pass. A forced
        `moe_impl` (dense / sparse / grouped) applies here too.
        """
        cfg = self.cfg
        B, S = token_ids.shape
        if S > self.max_seq:
            raise ValueError(f"S={S} exceeds max_seq={self.max_seq}")
        positions = (
            torch.arange(S, device=self.device, dtype=torch.int32).repeat(B)
        )

        x = self.embed.index_select(0, token_ids.reshape(-1))
        causal = None if x.is_cuda else blocks.causal_mask(S, self.device)

        def attn(li, layer, h):
            a = blocks.prefill_attn(
                h @ layer.wqkv.t(), self.k_cache[li], self.v_cache[li],
                positions, cfg, B, S, self.scale, causal,
            )
            return a @ layer.wo.t()

        def mlp(layer, h2):
            return self._moe_mlp_impl(layer, h2, dense=False)

        final = blocks.run_layers(
            self.layers, x, self.final_norm, cfg.rms_eps, attn, mlp
        )
        last = final.reshape(B, S, cfg.hidden_size)[:, -1].contiguous()
        logits = last @ self.lm_head.t()
        self.context_lens.zero_()
        self.context_lens[:B] = S
        return logits
