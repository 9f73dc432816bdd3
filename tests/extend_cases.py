"""Float64 reference, case builders and the shape grid for chunked-prefill
("extend") attention: a chunk of C query rows per sequence over a cached
prefix of P_b rows.

Plain helper module on top of attn_oracle.py: torch on CPU only. The cases
are the causal census and sentinel of attn_oracle at S = max(P) + C with
only the query rows P_b .. P_b+C-1 of each sequence kept, so the census
counts the positions <= P_b + i per residue, the sentinel's parity dims
lose a dropped newest key and its dim 2 lights on a read past S. The bound
is attn_oracle.attn_bound(p_bf16=True), as for the one-shot prefill kernel.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

import attn_oracle as ao
from attn_oracle import D

# The smallest shapes at which each mistake can occur: a prefix of 0, inside
# the first tile, one short of / one past a tile edge, past two tiles; chunks
# of one row, part of a q-tile, exactly one, one more, and more than two.
PREFIX_PAIRS = ((0, 0), (1, 64), (63, 65), (130, 7), (200, 128))
CHUNKS = (1, 17, 64, 65, 130)
HEADS = ((8, 2), (8, 1), (4, 4))
FAMILIES = ("census", "sentinel")
LONG_PREFIX = (2053, 1000)
LONG_CHUNK = 130


def extend_ref64(q, k_cache, v_cache, prefix_lens, chunk, scale):
    """Float64 chunked-prefill attention. q [B*chunk, Hq, D], caches
    [B, Hk, S_max, D]; query i of sequence b sits at position P_b + i and
    sees key kp iff kp <= P_b + i. Rows at or past P_b + chunk, which no
    query may see, are never read (they may hold NaN). Returns (ref, absref)
    = (P.V, P.|V|), both [B*chunk, Hq, D] float64."""
    T, Hq, d = q.shape
    B, Hk, S_max, _ = k_cache.shape
    G = Hq // Hk
    P = torch.as_tensor(prefix_lens).long().reshape(B)
    qd = ao.f64(q).reshape(B, chunk, Hk, G, d)
    pos = torch.arange(S_max)
    live = pos[None, :] < (P + chunk)[:, None]                    # [B, S]
    rows = live[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float64)
    k = torch.where(rows, ao.f64(k_cache), zero)
    v = torch.where(rows, ao.f64(v_cache), zero)
    scores = torch.einsum("bqhgd,bhsd->bhgqs", qd, k) * scale
    qpos = P[:, None] + torch.arange(chunk)[None, :]              # [B, C]
    mask = pos[None, None, :] <= qpos[:, :, None]                 # [B, C, S]
    ref, absref = ao._masked_softmax_pv(scores, v[:, :, None],
                                        mask[:, None, None])
    shape = (T, Hq, d)
    return (ref.permute(0, 3, 1, 2, 4).reshape(shape),
            absref.permute(0, 3, 1, 2, 4).reshape(shape))


def extend_case(family, prefixes, chunk, hq, hk, dtype, seed=None):
    """`family` case of attn_oracle at S = max(prefixes) + chunk, query rows
    P_b .. P_b+chunk-1 of sequence b kept. `lens` = P_b + chunk is the first
    dead row of each sequence; the caches have S + 8 rows."""
    B = len(prefixes)
    S = max(prefixes) + chunk
    if family == "census":
        base = ao.prefill_census_case(B, hq, hk, S, dtype)
    else:
        base = ao.prefill_sentinel_case(B, hq, hk, S, dtype,
                                        seed=S if seed is None else seed)
    q = base.q.reshape(B, S, hq, D)
    q = torch.stack([q[b, p:p + chunk] for b, p in enumerate(prefixes)])
    return SimpleNamespace(
        q=q.reshape(B * chunk, hq, D).contiguous(), k=base.k, v=base.v,
        prefix_lens=torch.tensor(prefixes, dtype=torch.int32), chunk=chunk,
        batch=B, lens=[p + chunk for p in prefixes], scale=base.scale,
        fp8=base.fp8)


@functools.lru_cache(maxsize=None)
def cached_extend(family, prefixes, chunk, hq, hk, dtype):
    """(case, ref, absref), built once per process and shared."""
    c = extend_case(family, prefixes, chunk, hq, hk, dtype)
    ref, absref = extend_ref64(c.q, c.k, c.v, c.prefix_lens, c.chunk, c.scale)
    return c, ref, absref


def bound(ref, absref):
    return ao.attn_bound(ref, absref, p_bf16=True)
