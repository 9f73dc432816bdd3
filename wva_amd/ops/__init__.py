"""MI355X (gfx950) fused op library.

Hand-written HIP/CDNA4 kernels for the calibration decode path's hot
non-GEMM ops (GEMMs go through hipBLASLt via torch.matmul — guide rule:
library GEMMs stay in the library). The extension is built in-tree
(`wva_amd/ops/_wva_ops*.so`, see setup.py / __graft_entry__.build).

Fail-loud contract: on a ROCm GPU the HIP extension MUST load — there is
no silent eager fallback on the GPU path (the driver verifies the .so is
actually loaded). Pure-CPU processes (unit tests, the control plane) use
the fp32 torch reference implementations below, which are also the
numerics references for the GPU tests.
"""
from __future__ import annotations

import glob
import importlib.util
import math
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_ext = None
_ext_error: Optional[str] = None


def _try_load_extension():
    global _ext, _ext_error
    if _ext is not None:
        return _ext
    candidates = sorted(glob.glob(os.path.join(_HERE, "_wva_ops*.so")))
    if not candidates:
        _ext_error = (
            f"HIP extension _wva_ops*.so not found in {_HERE}; build it with "
            "`python -m wva_amd.ops.build` (or __graft_entry__.build())"
        )
        return None
    spec = importlib.util.spec_from_file_location("_wva_ops", candidates[0])
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except Exception as e:  # noqa: BLE001
        _ext_error = f"failed to load {candidates[0]}: {e}"
        return None
    _ext = mod
    return _ext


def extension_available() -> bool:
    return _try_load_extension() is not None


def _require_ext():
    ext = _try_load_extension()
    if ext is None:
        raise RuntimeError(
            f"wva_amd.ops: GPU tensor passed but HIP extension unavailable: "
            f"{_ext_error}"
        )
    return ext


# --- fp32 torch reference implementations (CPU tests + GPU numerics refs) ---


def rmsnorm_ref(
    input: torch.Tensor,
    weight: torch.Tensor,
    residual: Optional[torch.Tensor] = None,
    eps: float = 1e-5,
):
    x = input.float()
    if residual is not None:
        x = x + residual.float()
    folded = x
    rms = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    out = x * rms * weight.float()
    return out, folded


def rope_ref(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor,
    theta: float = 500000.0,
):
    """NeoX half-rotation RoPE, fp32."""

    def rot(x):
        t, h, d = x.shape
        half = d // 2
        xf = x.float()
        inv_freq = theta ** (
            -2.0 * torch.arange(half, dtype=torch.float32, device=x.device) / d
        )
        angle = positions.float()[:, None] * inv_freq[None, :]  # [T, half]
        cos = angle.cos()[:, None, :]
        sin = angle.sin()[:, None, :]
        x1, x2 = xf[..., :half], xf[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)

    return rot(q), rot(k)


def silu_mul_ref(gate: torch.Tensor, up: torch.Tensor):
    g = gate.float()
    return torch.nn.functional.silu(g) * up.float()


def gqa_decode_attn_ref(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
):
    """fp32 reference: per-sequence masked softmax attention.
    Cache layout is head-major [B, Hk, S, D]."""
    B, Hq, D = q.shape
    _, Hk, S, _ = k_cache.shape
    G = Hq // Hk
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=q.device)
    for b in range(B):
        ctx = int(context_lens[b])
        k = k_cache[b, :, :ctx].float()  # [Hk, ctx, D]
        v = v_cache[b, :, :ctx].float()
        for h in range(Hq):
            kvh = h // G
            scores = (k[kvh] @ (q[b, h].float() * scale))  # [ctx]
            p = torch.softmax(scores, dim=0)
            out[b, h] = p @ v[kvh]
    return out


def _as_bytes(t: torch.Tensor) -> torch.Tensor:
    """e4m3 tensors are indexed as bytes (a view of the same storage)."""
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


def gather_pages(
    pages: torch.Tensor, block_tables: torch.Tensor, context_lens: torch.Tensor
) -> torch.Tensor:
    """Materialise a paged pool [num_blocks, Hk, block_size, D] as the
    contiguous head-major cache [B, Hk, max_blocks * block_size, D] that the
    paged kernels see, by their addressing rules: the effective context is
    min(context_lens[b], max_blocks * block_size), only the table entries
    below ceil(ctx / block_size) are looked at, and an id is clamped into
    [0, num_blocks - 1]. Rows of pages that are not looked at stay 0."""
    num_blocks, Hk, bs, D = pages.shape
    B, max_blocks = block_tables.shape
    out = torch.zeros(
        B, Hk, max_blocks * bs, D, dtype=pages.dtype, device=pages.device
    )
    src, dst = _as_bytes(pages), _as_bytes(out)
    for b in range(B):
        ctx = min(int(context_lens[b]), max_blocks * bs)
        n = (ctx + bs - 1) // bs
        if n <= 0:
            continue
        ids = block_tables[b, :n].long().clamp(0, num_blocks - 1)
        dst[b, :, : n * bs] = (
            src[ids].permute(1, 0, 2, 3).reshape(Hk, n * bs, D)
        )
    return out


def paged_decode_attn_ref(
    q: torch.Tensor,
    k_pages: torch.Tensor,
    v_pages: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
):
    """fp32 reference of paged decode attention: gather each sequence's
    pages into a contiguous cache (gather_pages) and run
    gqa_decode_attn_ref on it."""
    max_ctx = block_tables.shape[1] * k_pages.shape[2]
    ctx = context_lens.clamp(min=0, max=max_ctx)
    return gqa_decode_attn_ref(
        q,
        gather_pages(k_pages, block_tables, ctx),
        gather_pages(v_pages, block_tables, ctx),
        ctx,
        scale,
    )


def extend_attn_ref(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    prefix_lens: torch.Tensor,
    chunk: int,
    scale: float,
):
    """fp32 reference of chunked-prefill attention. q [B*chunk, Hq, D];
    sequence b's chunk sits at positions P_b .. P_b+chunk-1 of the
    head-major caches [B, Hk, S, D] (P_b = prefix_lens[b]); query i sees
    key kp iff kp <= P_b + i. Rows at or past P_b + chunk are never read."""
    T, Hq, D = q.shape
    Hk = k_cache.shape[1]
    G = Hq // Hk
    B = T // chunk
    qf = q.float().reshape(B, chunk, Hk, G, D)
    out = torch.zeros(B, chunk, Hk, G, D, dtype=torch.float32, device=q.device)
    rows = torch.arange(chunk, device=q.device)
    for b in range(B):
        p0 = int(prefix_lens[b])
        n = p0 + chunk
        k = k_cache[b, :, :n].float()  # [Hk, n, D]
        v = v_cache[b, :, :n].float()
        scores = torch.einsum("qhgd,hsd->hgqs", qf[b], k) * scale
        seen = torch.arange(n, device=q.device)[None, :] <= (p0 + rows)[:, None]
        scores = scores.masked_fill(~seen, float("-inf"))
        p = torch.softmax(scores, dim=-1)
        out[b] = torch.einsum("hgqs,hsd->qhgd", p, v)
    return out.reshape(T, Hq, D)


def extend_attn_ragged_ref(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    prefix_lens: torch.Tensor,
    chunk_lens: torch.Tensor,
    max_chunk: int,
    scale: float,
):
    """fp32 reference of ragged chunked-prefill attention. q is packed
    [T, Hq, D]: sequence b owns the chunk_lens[b] <= max_chunk rows from the
    exclusive cumsum of chunk_lens and sits at positions P_b .. P_b+len_b-1
    (P_b = prefix_lens[b]). Per sequence it is extend_attn_ref with B = 1
    and chunk = len_b, so cache rows at or past P_b + len_b are never read;
    rows of q that no sequence owns give 0."""
    T, Hq, D = q.shape
    out = torch.zeros(T, Hq, D, dtype=torch.float32, device=q.device)
    start = 0
    for b, n in enumerate(chunk_lens.tolist()):
        n = min(max(int(n), 0), max_chunk, T - start)
        if n:
            out[start:start + n] = extend_attn_ref(
                q[start:start + n], k_cache[b:b + 1], v_cache[b:b + 1],
                prefix_lens[b:b + 1], n, scale,
            )
        start += n
    return out


def moe_route_ref(router_logits: torch.Tensor, top_k: int):
    """MoE routing reference.

    Returns (topk_idx [T,K] int32 in descending logit order — lowest
    expert index wins an exact tie, topk_w [T,K] fp32 softmax over the K
    selected logits, expert_offsets [E+1] int32 exclusive prefix of
    per-expert slot counts, sorted_slots [T*K] int32 slot ids t*K+k
    grouped by expert and ascending within an expert)."""
    logits = router_logits.float()
    E = logits.shape[1]
    # a stable descending sort keeps the lower index first among equals
    vals, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
    vals, idx = vals[:, :top_k], idx[:, :top_k]
    topk_w = torch.softmax(vals, dim=-1)
    flat = idx.reshape(-1)
    sorted_slots = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=E)
    offsets = torch.zeros(E + 1, dtype=torch.int64, device=logits.device)
    offsets[1:] = torch.cumsum(counts, dim=0)
    return (
        idx.to(torch.int32).contiguous(),
        topk_w.contiguous(),
        offsets.to(torch.int32),
        sorted_slots.to(torch.int32),
    )


def moe_gate_up_swiglu_ref(
    x: torch.Tensor,
    w_gate_up: torch.Tensor,
    expert_offsets: torch.Tensor,
    sorted_slots: torch.Tensor,
    top_k: int,
) -> torch.Tensor:
    """fp32 [T*K, I]: silu(g)*u of x[slot // K] @ w_gate_up[e].T for the
    expert e owning each sorted position; w_gate_up is [E, 2I, H]."""
    E, two_i, _ = w_gate_up.shape
    inter = two_i // 2
    offs = expert_offsets.tolist()
    tokens = torch.div(sorted_slots.long(), top_k, rounding_mode="floor")
    out = torch.zeros(
        sorted_slots.numel(), inter, dtype=torch.float32, device=x.device
    )
    for e in range(E):
        lo, hi = offs[e], offs[e + 1]
        if hi == lo:
            continue
        gu = x[tokens[lo:hi]].float() @ w_gate_up[e].float().t()
        out[lo:hi] = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
    return out


def moe_down_combine_ref(
    act_sorted: torch.Tensor,
    w_down: torch.Tensor,
    topk_w: torch.Tensor,
    expert_offsets: torch.Tensor,
    sorted_slots: torch.Tensor,
) -> torch.Tensor:
    """fp32 [T, H]: sum_k topk_w[t,k] * (act_sorted[pos(t,k)] @
    w_down[e].T); w_down is [E, H, I]."""
    E, hidden, _ = w_down.shape
    T, K = topk_w.shape
    offs = expert_offsets.tolist()
    y = torch.zeros(T * K, hidden, dtype=torch.float32, device=w_down.device)
    slots = sorted_slots.long()
    for e in range(E):
        lo, hi = offs[e], offs[e + 1]
        if hi == lo:
            continue
        y[slots[lo:hi]] = act_sorted[lo:hi].float() @ w_down[e].float().t()
    return (y.reshape(T, K, hidden) * topk_w.float().unsqueeze(-1)).sum(dim=1)


def moe_mlp_ref(
    x: torch.Tensor,
    router_logits: torch.Tensor,
    w_gate_up: torch.Tensor,
    w_down: torch.Tensor,
    top_k: int,
) -> torch.Tensor:
    """fp32 routed expert MLP; `act` is rounded to bf16 between the two
    GEMMs exactly as the kernels do."""
    _, topk_w, offsets, slots = moe_route_ref(router_logits, top_k)
    act = moe_gate_up_swiglu_ref(x, w_gate_up, offsets, slots, top_k)
    return moe_down_combine_ref(
        act.to(torch.bfloat16), w_down, topk_w, offsets, slots
    )


# --- dispatching public ops (GPU → HIP kernel, CPU → reference) ---


def rmsnorm(
    input: torch.Tensor,
    weight: torch.Tensor,
    residual: Optional[torch.Tensor] = None,
    eps: float = 1e-5,
) -> torch.Tensor:
    if input.is_cuda:
        return _require_ext().rmsnorm(input, weight, residual, eps)
    out, folded = rmsnorm_ref(input, weight, residual, eps)
    if residual is not None:
        residual.copy_(folded.to(residual.dtype))
    return out.to(input.dtype)


def rope(
    q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor,
    theta: float = 500000.0,
) -> None:
    if q.is_cuda:
        _require_ext().rope(q, k, positions.to(torch.int32), theta)
        return
    qr, kr = rope_ref(q, k, positions, theta)
    q.copy_(qr.to(q.dtype))
    k.copy_(kr.to(k.dtype))


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    if gate.is_cuda:
        return _require_ext().silu_mul(gate, up)
    return silu_mul_ref(gate, up).to(gate.dtype)


def rope_append_kv(
    qkv: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    positions: torch.Tensor,
    num_q_heads: int,
    num_kv_heads: int,
    theta: float = 500000.0,
) -> torch.Tensor:
    """Decode fast path: strided qkv row -> RoPE'd q + KV-cache append.
    Returns contiguous q [B, Hq, D]."""
    if qkv.is_cuda:
        return _require_ext().rope_append_kv(
            qkv, k_cache, v_cache, positions.to(torch.int32),
            num_q_heads, num_kv_heads, theta,
        )
    B = qkv.shape[0]
    q, k, v = _rope_split_qkv(
        qkv, k_cache.shape[3], positions, num_q_heads, num_kv_heads, theta
    )
    # head-major cache [B, Hk, S, D]
    idx = torch.arange(B)
    k_cache[idx, :, positions.long()] = k.to(k_cache.dtype)
    v_cache[idx, :, positions.long()] = v.to(v_cache.dtype)
    return q


def _rope_split_qkv(qkv, D, positions, num_q_heads, num_kv_heads, theta):
    """CPU reference of the append ops' rotation: the qkv row split into
    RoPE'd q [B, Hq, D] and k [B, Hk, D] (rounded to qkv's dtype) and the
    raw v [B, Hk, D]."""
    B = qkv.shape[0]
    q = qkv[:, : num_q_heads * D].reshape(B, num_q_heads, D).contiguous()
    k = (
        qkv[:, num_q_heads * D : (num_q_heads + num_kv_heads) * D]
        .reshape(B, num_kv_heads, D)
        .contiguous()
    )
    v = qkv[:, (num_q_heads + num_kv_heads) * D :].reshape(B, num_kv_heads, D)
    qr, kr = rope_ref(q, k, positions, theta)
    q.copy_(qr.to(q.dtype))
    k.copy_(kr.to(k.dtype))
    return q, k, v


def rope_append_kv_paged(
    qkv: torch.Tensor,
    k_pages: torch.Tensor,
    v_pages: torch.Tensor,
    block_tables: torch.Tensor,
    positions: torch.Tensor,
    num_q_heads: int,
    num_kv_heads: int,
    theta: float = 500000.0,
) -> torch.Tensor:
    """rope_append_kv into a paged pool [num_blocks, Hk, block_size, D]:
    sequence b's K/V row goes to page block_tables[b, pos // block_size],
    row pos % block_size. If pos // block_size is past the table or the
    entry is outside [0, num_blocks), that sequence's K/V stores are
    skipped; q is produced all the same. block_tables [B, max_blocks] and
    positions [B] are read on the device (graph-capturable). Returns
    contiguous q [B, Hq, D]."""
    if qkv.is_cuda:
        return _require_ext().rope_append_kv_paged(
            qkv, k_pages, v_pages, block_tables.to(torch.int32),
            positions.to(torch.int32), num_q_heads, num_kv_heads, theta,
        )
    num_blocks, _, bs, D = k_pages.shape
    max_blocks = block_tables.shape[1]
    q, k, v = _rope_split_qkv(
        qkv, D, positions, num_q_heads, num_kv_heads, theta
    )
    pos = positions.long()
    entry = torch.div(pos, bs, rounding_mode="floor")
    in_table = (pos >= 0) & (entry < max_blocks)
    seq = torch.arange(qkv.shape[0])
    ids = block_tables.long()[seq, entry.clamp(0, max_blocks - 1)]
    ok = in_table & (ids >= 0) & (ids < num_blocks)
    ids, rows = ids[ok], (pos % bs)[ok]
    _as_bytes(k_pages)[ids, :, rows] = _as_bytes(k.to(k_pages.dtype))[ok]
    _as_bytes(v_pages)[ids, :, rows] = _as_bytes(v.to(v_pages.dtype))[ok]
    return q


def silu_mul_fused(gate_up: torch.Tensor) -> torch.Tensor:
    """SwiGLU on the fused [rows, 2*inter] gate_up GEMM output."""
    if gate_up.is_cuda:
        return _require_ext().silu_mul_fused(gate_up)
    inter = gate_up.shape[1] // 2
    return silu_mul_ref(gate_up[:, :inter], gate_up[:, inter:]).to(
        gate_up.dtype
    )


def gqa_decode_attn(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    context_lens: torch.Tensor,
    scale: Optional[float] = None,
    num_splits: Optional[int] = None,
    variant: str = "auto",
) -> torch.Tensor:
    """GQA decode attention over contiguous head-major caches [B, Hk, S,
    128]. `num_splits` and `variant` are those of paged_decode_attn; None
    asks gqa_decode_num_splits over S."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda:
        return _require_ext().gqa_decode_attn(
            q, k_cache, v_cache, context_lens.to(torch.int32), scale,
            variant, num_splits,
        )
    return gqa_decode_attn_ref(q, k_cache, v_cache, context_lens, scale).to(
        q.dtype
    )


def gqa_decode_num_splits(batch: int, num_kv_heads: int, max_seq: int) -> int:
    """Split-KV factor the decode attention launch picks for a
    [batch, num_kv_heads, max_seq, 128] cache (1 = unsplit, no merge)."""
    return int(
        _require_ext().gqa_decode_attn_splits(batch, num_kv_heads, max_seq)
    )


def paged_decode_num_splits(
    batch: int, num_kv_heads: int, max_blocks: int, block_size: int
) -> int:
    """Split-KV factor paged_decode_attn picks for block tables of
    `max_blocks` entries: that of a contiguous cache of max_blocks *
    block_size rows."""
    return gqa_decode_num_splits(batch, num_kv_heads, max_blocks * block_size)


def paged_decode_attn(
    q: torch.Tensor,
    k_pages: torch.Tensor,
    v_pages: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: Optional[float] = None,
    num_splits: Optional[int] = None,
    variant: str = "auto",
) -> torch.Tensor:
    """GQA decode attention over a paged KV pool. k_pages / v_pages are
    [num_blocks, Hk, block_size, 128] (bf16 or float8_e4m3fn, block_size
    16, 32 or 64); block_tables [B, max_blocks] int32 maps sequence b's
    block i to a physical page and context_lens [B] int32 gives its length.
    Both are read on the device only (no host sync, graph-capturable).

    The effective context is min(context_lens[b], max_blocks * block_size);
    table entries at or past ceil(ctx / block_size) are never looked at and
    an id outside [0, num_blocks) is clamped into the pool, so a corrupt
    table gives wrong numbers, never an out-of-bounds access. `num_splits`
    forces the split-KV factor; None asks paged_decode_num_splits.
    `variant` pins "v4" or "v5"; "auto" applies the rule measured on the
    contiguous layout."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda:
        return _require_ext().paged_decode_attn(
            q, k_pages, v_pages, block_tables.to(torch.int32),
            context_lens.to(torch.int32), scale, num_splits, variant,
        )
    return paged_decode_attn_ref(
        q, k_pages, v_pages, block_tables, context_lens, scale
    ).to(q.dtype)


def moe_route(router_logits: torch.Tensor, top_k: int):
    """Device-side MoE routing from fp32 router logits [T, E]; see
    moe_route_ref for the four outputs. Nothing is read back to the host,
    so the op is graph-capturable."""
    if router_logits.is_cuda:
        return tuple(
            _require_ext().moe_route(
                router_logits.float().contiguous(), top_k
            )
        )
    return moe_route_ref(router_logits, top_k)


def moe_gate_up_swiglu(
    x: torch.Tensor,
    w_gate_up: torch.Tensor,
    expert_offsets: torch.Tensor,
    sorted_slots: torch.Tensor,
    top_k: int,
) -> torch.Tensor:
    """Grouped gate_up GEMM + SwiGLU over the routed rows only: bf16
    [T*K, I] in expert-sorted order, against the stacked [E, 2I, H]."""
    if x.is_cuda:
        return _require_ext().moe_gate_up_swiglu(
            x, w_gate_up, expert_offsets, sorted_slots, top_k
        )
    return moe_gate_up_swiglu_ref(
        x, w_gate_up, expert_offsets, sorted_slots, top_k
    ).to(x.dtype)


def moe_down_combine(
    act_sorted: torch.Tensor,
    w_down: torch.Tensor,
    topk_w: torch.Tensor,
    expert_offsets: torch.Tensor,
    sorted_slots: torch.Tensor,
) -> torch.Tensor:
    """Grouped down GEMM against the stacked [E, H, I] + top-k combine:
    bf16 [T, H], summed in a fixed order (deterministic)."""
    if act_sorted.is_cuda:
        return _require_ext().moe_down_combine(
            act_sorted, w_down, topk_w, expert_offsets, sorted_slots
        )
    return moe_down_combine_ref(
        act_sorted, w_down, topk_w, expert_offsets, sorted_slots
    ).to(act_sorted.dtype)


def moe_down_num_splits(
    tokens: int, top_k: int, num_experts: int, hidden: int, inter: int
) -> int:
    """Split-K factor the down GEMM kernel picks for these static shapes."""
    return int(
        _require_ext().moe_down_splits(
            tokens, top_k, num_experts, hidden, inter
        )
    )


def moe_mlp(
    x: torch.Tensor,
    router_logits: torch.Tensor,
    w_gate_up: torch.Tensor,
    w_down: torch.Tensor,
    top_k: int,
) -> torch.Tensor:
    """Routed expert MLP: x [T, H] bf16, router_logits [T, E] fp32,
    stacked expert weights [E, 2I, H] / [E, H, I] → bf16 [T, H].

    Only routed experts' weights are streamed and only routed tokens are
    multiplied; no step syncs with the host (csrc/moe.hip)."""
    if x.is_cuda:
        _, topk_w, offsets, slots = moe_route(router_logits, top_k)
        act = moe_gate_up_swiglu(x, w_gate_up, offsets, slots, top_k)
        return moe_down_combine(act, w_down, topk_w, offsets, slots)
    return moe_mlp_ref(x, router_logits, w_gate_up, w_down, top_k).to(x.dtype)


def enable_tuned_gemms() -> bool:
    """Load the committed TunableOp GEMM solution table for gfx950.

    `wva_amd/ops/tunableop_gfx950.csv` holds hipBLASLt/rocBLAS solution
    choices autotuned on MI355X for the decode GEMM shapes (qkv/o/
    gate_up/down/lm_head at batches 1-64) — measured α drops ~10% vs the
    default heuristics (profiles/tunableop_ab.json). Solutions are keyed
    to PyTorch/hipBLASLt versions via the CSV's Validator rows; on a
    mismatched stack TunableOp discards them and falls back to defaults.
    Returns True if the table was loaded.
    """
    path = os.path.join(_HERE, "tunableop_gfx950.csv")
    if not torch.cuda.is_available() or not os.path.exists(path):
        return False
    tun = torch.cuda.tunable
    tun.enable(True)
    tun.tuning_enable(False)  # read-only: never autotune in production
    tun.read_file(path)
    return True


def skinny_linear(
    x: torch.Tensor, w: torch.Tensor, w_scale: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """y = x @ w.T ([M,K] @ [N,K]^T, M <= 64, K % 128 == 0) on the
    weight-streaming MFMA kernel (csrc/skinny_gemm.hip). With `w_scale` [N]
    the weights are weight-only fp8: w is float8_e4m3fn with per-channel
    float32 scales and y = x @ (w * w_scale[:, None]).T. On CPU it is that
    matmul in float32."""
    if x.is_cuda:
        if w_scale is None:
            return _require_ext().skinny_linear(x, w)
        return _require_ext().skinny_linear_fp8(x, w, w_scale)
    wf = w.float() if w_scale is None else w.float() * w_scale[:, None]
    return (x.float() @ wf.t()).to(x.dtype)


def skinny_linear_num_splits(M: int, N: int, K: int) -> int:
    """Split-K factor skinny_linear picks for x [M, K] and w [N, K]
    (1 = unsplit, no workspace and no merge). Static shapes only; the same
    for bf16 and fp8 weights."""
    return int(_require_ext().skinny_linear_splits(M, N, K))


def linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Decode linear y = x @ w.T ([M,K] @ [N,K]^T).

    Dispatch is measurement-driven and currently ALWAYS hipBLASLt: the
    in-tree weight-streaming MFMA kernel (skinny_linear) beat hipBLASLt on
    isolated small-N/small-M microbenches but loses IN CONTEXT inside the decode step, where the
    activation matrix is not L2-hot between layers (decode b=1 measured
    5.27 ms/step pure-blaslt vs 5.41 with the kernel dispatched on
    qkv/o). Full history: profiles/skinny_gemm_ab.txt and
    docs/mi355x-kernels.md (negative results). Set WVA_FORCE_SKINNY=1
    to re-enable the measured window for experiments.
    """
    if (
        os.environ.get("WVA_FORCE_SKINNY")
        and x.is_cuda
        and x.shape[0] <= 16
        and x.shape[1] % 128 == 0
        and x.shape[1] <= 8192
        and w.shape[0] <= 8192
    ):
        return skinny_linear(x, w)
    return x @ w.t()


def prefill_attn(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    batch: int,
    seq: int,
    scale: float,
) -> torch.Tensor:
    """Causal GQA flash-prefill over the (populated) head-major caches.

    GPU-only (fail-loud): the CPU prefill reference lives in
    calibration/model.py's matmul branch.
    """
    return _require_ext().prefill_attn(q, k_cache, v_cache, batch, seq, scale)


def extend_attn(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    prefix_lens: torch.Tensor,
    chunk: int,
    scale: float,
) -> torch.Tensor:
    """Chunked-prefill attention: `chunk` new query rows per sequence over
    a cached prefix. q [B*chunk, Hq, 128]; the caches already hold sequence
    b's prefix and its chunk at rows prefix_lens[b] .. prefix_lens[b] +
    chunk - 1. prefix_lens [B] is read on the device (no host sync)."""
    if q.is_cuda:
        return _require_ext().extend_attn(
            q, k_cache, v_cache, prefix_lens.to(torch.int32), chunk, scale
        )
    return extend_attn_ref(q, k_cache, v_cache, prefix_lens, chunk, scale).to(
        q.dtype
    )


def extend_attn_ragged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    prefix_lens: torch.Tensor,
    chunk_lens: torch.Tensor,
    max_chunk: int,
    scale: float,
    num_splits: Optional[int] = None,
) -> torch.Tensor:
    """Ragged chunked-prefill attention: one launch for sequences whose
    chunks differ in length. q is packed [T, Hq, 128]; sequence b owns the
    chunk_lens[b] rows that start at the exclusive cumsum of chunk_lens and
    continues from prefix_lens[b] (its K/V already in the caches at rows
    prefix_lens[b] .. + chunk_lens[b] - 1). `max_chunk` is a host-side upper
    bound of chunk_lens that sizes the launch; prefix_lens, chunk_lens and
    the row starts stay on the device (no host sync, graph-capturable).
    Rows of q that no sequence owns come back as 0. `num_splits` forces the
    split-KV factor; None asks extend_attn_ragged_num_splits."""
    if q.is_cuda:
        if num_splits is None:
            num_splits = extend_attn_ragged_num_splits(
                chunk_lens.shape[0], q.shape[1], max_chunk, k_cache.shape[2]
            )
        lens = chunk_lens.to(torch.int32)
        q_starts = torch.cumsum(lens, 0, dtype=torch.int32) - lens
        return _require_ext().extend_attn_ragged(
            q, k_cache, v_cache, prefix_lens.to(torch.int32), q_starts, lens,
            max_chunk, scale, num_splits,
        )
    return extend_attn_ragged_ref(
        q, k_cache, v_cache, prefix_lens, chunk_lens, max_chunk, scale
    ).to(q.dtype)


def extend_attn_ragged_num_splits(
    batch: int, num_q_heads: int, max_chunk: int, max_seq: int
) -> int:
    """Split-KV factor extend_attn_ragged picks for `batch` sequences of at
    most `max_chunk` rows over a [*, *, max_seq, 128] cache (1 = unsplit, no
    merge). Static shapes only."""
    return int(
        _require_ext().extend_attn_ragged_splits(
            batch, num_q_heads, max_chunk, max_seq
        )
    )
