"""The one case of the chunk-append tests (CPU and GPU), on top of
paged_cases.py: chunks at (prefix, len) = (0, 17), (15, 1), (63, 65),
(130, 0), one of 8 rows at 131064 whose hand-built table holds a single live
entry (the last), and one with 2 rows in a live page, then `bs` rows on a -1
entry, then 3 rows past the end of its table.

Plain helper module: torch on the CPU only.
"""
from types import SimpleNamespace

import torch

import paged_cases as pc
from attn_oracle import BF16, D

HQ, HK = pc.APPEND_HQ, pc.APPEND_HK
MAX_POS = 131072


def append_case(dtype, bs):
    """Packed qkv rows, a random pool, shuffled pages; `paged[r]` says
    whether packed row r has a page."""
    g = torch.Generator().manual_seed(11 + bs)
    seqs = [(0, 17), (15, 1), (63, 65), (130, 0), (MAX_POS - 8, 8),
            (MAX_POS - bs - 2, bs + 5)]
    need = [pc.blocks_of(p + n, bs) for p, n in seqs[:4]]
    num_blocks = sum(need) + 2 + pc.SPARE_PAGES
    perm = torch.randperm(num_blocks, generator=g).to(torch.int32)
    tables = torch.full((len(seqs), MAX_POS // bs), -1, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        tables[b, :n] = perm[at:at + n]
        at += n
    tables[4, -1], tables[5, -2] = perm[at], perm[at + 1]
    lens = torch.tensor([n for _, n in seqs], dtype=torch.int32)
    T = int(lens.sum())
    pool = lambda: torch.randn(num_blocks, HK, bs, D,
                               generator=g).to(BF16).to(dtype)
    paged = torch.ones(T, dtype=torch.bool)
    paged[T - bs - 3:] = False
    return SimpleNamespace(
        qkv=torch.randn(T, (HQ + 2 * HK) * D, generator=g).to(BF16),
        k_pages=pool(), v_pages=pool(), tables=tables, lens=lens,
        prefix=torch.tensor([p for p, _ in seqs], dtype=torch.int32),
        max_chunk=int(lens.max()), paged=paged,
        seq=torch.repeat_interleave(torch.arange(len(seqs)), lens.long()),
        pos=torch.cat([p + torch.arange(n) for p, n in seqs]))
