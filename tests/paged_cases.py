"""Scatter the contiguous [B, Hk, S, D] caches of an attn_oracle case into a
paged pool [num_blocks, Hk, block_size, D] with block tables.

Plain helper module: torch on the CPU only. The layout is adversarial on
purpose:
  * the physical block order is a seeded permutation;
  * the pool has a few pages more than the sequences need;
  * every unused page is poisoned, and so is every row at or past lens[b]
    in a sequence's last page (bf16 NaN / the e4m3 byte 0x7f, as in
    attn_oracle.poison_dead_rows);
  * every table entry at index >= ceil(lens[b] / block_size) points at one
    of the poisoned pages: a valid id whose contents must never matter.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from attn_oracle import BF16, FP8, D

SPARE_PAGES = 3
# the append tests: one sequence per position, caches of APPEND_S rows
# rounded up to whole blocks
APPEND_POSITIONS = (0, 15, 16, 17, 31, 63, 64, 130)
APPEND_S = 136
APPEND_HQ, APPEND_HK = 8, 2


def raw(t: torch.Tensor) -> torch.Tensor:
    """A view that can be indexed, compared and moved whatever the dtype:
    e4m3 as bytes, bf16 as int16 (NaN compares equal to itself)."""
    return t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)


def poisoned(shape, dtype) -> torch.Tensor:
    if dtype == FP8:
        return torch.full(shape, 0x7F, dtype=torch.uint8).view(FP8)
    return torch.full(shape, math.nan, dtype=dtype)


def blocks_of(n: int, block_size: int) -> int:
    return (int(n) + block_size - 1) // block_size


def layout(lens, S, block_size, seed=0, shared_blocks=0):
    """Block tables [B, ceil(S / block_size)] int32 and the pool size for
    sequences of `lens` tokens. With `shared_blocks` > 0 every sequence's
    first `shared_blocks` entries are sequence 0's."""
    lens = [int(n) for n in lens]
    need = [blocks_of(n, block_size) for n in lens]
    own = [n - (shared_blocks if b else 0) for b, n in enumerate(need)]
    assert all(n >= 0 for n in own)
    num_blocks = sum(own) + SPARE_PAGES
    g = torch.Generator().manual_seed(1000 + 7 * seed + block_size)
    perm = torch.randperm(num_blocks, generator=g).to(torch.int32)
    spare = perm[sum(own):]
    max_blocks = blocks_of(S, block_size)
    tables = torch.empty(len(lens), max_blocks, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        head = shared_blocks if b else 0
        tables[b, :head] = tables[0, :head]
        tables[b, head:n] = perm[at:at + n - head]
        at += n - head
        # dead entries: a valid id of a poisoned page
        dead = torch.arange(max_blocks - n)
        tables[b, n:] = spare[(dead + b) % SPARE_PAGES]
    return tables, num_blocks


def scatter(k, v, lens, block_size, seed=0, shared_blocks=0):
    """Pool and tables of contiguous caches k, v [B, Hk, S, D]. With
    `shared_blocks`, the shared pages hold sequence 0's rows."""
    B, Hk, S, D = k.shape
    tables, num_blocks = layout(lens, S, block_size, seed, shared_blocks)
    pools = []
    for cache in (k, v):
        pool = poisoned((num_blocks, Hk, block_size, D), cache.dtype)
        dst, src = raw(pool), raw(cache)
        for b, n in enumerate(int(x) for x in lens):
            for i in range(blocks_of(n, block_size)):
                if b and i < shared_blocks:
                    continue
                lo = i * block_size
                hi = min(lo + block_size, n)
                dst[int(tables[b, i]), :, :hi - lo] = src[b, :, lo:hi]
        pools.append(pool)
    return SimpleNamespace(
        k_pages=pools[0], v_pages=pools[1], tables=tables,
        lens=torch.as_tensor(lens, dtype=torch.int32),
        block_size=block_size, num_blocks=num_blocks)


def scatter_case(c, block_size, seed=0):
    """The pool of an attn_oracle case (fields q, k, v, lens)."""
    return scatter(c.k, c.v, c.lens, block_size, seed)


def gather_row(pool, tables, b, pos, block_size):
    """Row [Hk, D] of sequence b's position `pos`, as raw()."""
    page = int(tables[b, pos // block_size])
    return raw(pool)[page, :, pos % block_size]


def append_inputs(dtype, block_size, seed=3):
    """(qkv, k, v, positions, lens): one sequence per position of
    APPEND_POSITIONS over full random caches [B, Hk, S, D] of S =
    max_blocks * block_size rows."""
    g = torch.Generator().manual_seed(seed)
    B = len(APPEND_POSITIONS)
    S = blocks_of(APPEND_S, block_size) * block_size
    qkv = torch.randn(B, (APPEND_HQ + 2 * APPEND_HK) * D, generator=g).to(BF16)
    k = torch.randn(B, APPEND_HK, S, D, generator=g).to(BF16).to(dtype)
    v = torch.randn(B, APPEND_HK, S, D, generator=g).to(BF16).to(dtype)
    pos = torch.tensor(APPEND_POSITIONS, dtype=torch.int32)
    return qkv, k, v, pos, [S] * B
