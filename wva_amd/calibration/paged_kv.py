"""Host-side block allocator of the paged KV cache.

The pool is `num_blocks` pages of `block_size` token rows (vLLM's
`num_gpu_blocks x block_size`). A sequence owns an ordered list of page ids,
entry i holding its positions i*block_size .. (i+1)*block_size-1; the device
only ever sees those lists as rows of a block table. This module is pure
bookkeeping: a free list and reference counts, no device work.

Two sequences may share leading pages (a prefix-cache hit): `share` puts the
first k pages of one sequence at the head of another and bumps their
reference counts. Only full blocks are shared; there is no copy-on-write, so
a shared page must not be appended to.
"""
from __future__ import annotations

import random
from typing import Dict, Hashable, List, Optional


class BlockAllocator:
    def __init__(self, num_blocks: int, seed: Optional[int] = None):
        """`seed` shuffles the order in which free pages are handed out (so
        that sequences are scattered over the pool); None hands them out in
        ascending order."""
        if num_blocks < 1:
            raise ValueError(f"num_blocks must be >= 1, got {num_blocks}")
        self.num_blocks = num_blocks
        self.seed = seed
        self.reset()

    def reset(self) -> None:
        """Free everything and restore the initial hand-out order."""
        order = list(range(self.num_blocks))
        if self.seed is not None:
            random.Random(self.seed).shuffle(order)
        # pages are popped from the end
        self._free: List[int] = order[::-1]
        self._refs: List[int] = [0] * self.num_blocks
        self._seqs: Dict[Hashable, List[int]] = {}

    @property
    def num_free(self) -> int:
        return len(self._free)

    @property
    def num_live(self) -> int:
        """Pages with a reference count above 0."""
        return self.num_blocks - len(self._free)

    def blocks(self, seq: Hashable) -> List[int]:
        """The page ids of `seq`, in position order (a copy)."""
        return list(self._seqs.get(seq, ()))

    def refcount(self, block: int) -> int:
        return self._refs[block]

    def allocate(self, seq: Hashable, n: int) -> List[int]:
        """Append `n` fresh pages to `seq`; returns them."""
        if n < 0:
            raise ValueError(f"cannot allocate {n} blocks")
        if n > len(self._free):
            raise RuntimeError(
                f"paged KV pool exhausted: {n} blocks requested, "
                f"{len(self._free)} free of {self.num_blocks}"
            )
        new = [self._free.pop() for _ in range(n)]
        for blk in new:
            self._refs[blk] = 1
        self._seqs.setdefault(seq, []).extend(new)
        return new

    def share(self, src: Hashable, dst: Hashable, k: int) -> List[int]:
        """Make the first `k` pages of `src` the first pages of `dst`, which
        must not own any page yet. The pages must be full: the caller passes
        k = shared_tokens // block_size (see `full_blocks`)."""
        have = self._seqs.get(src, [])
        if k < 0 or k > len(have):
            raise ValueError(
                f"cannot share {k} blocks of a sequence that owns {len(have)}"
            )
        if self._seqs.get(dst):
            raise ValueError("the receiving sequence already owns blocks")
        shared = have[:k]
        for blk in shared:
            self._refs[blk] += 1
        self._seqs[dst] = list(shared)
        return list(shared)

    def free(self, seq: Hashable) -> None:
        """Drop `seq`; a page returns to the free list when its reference
        count reaches 0."""
        for blk in self._seqs.pop(seq, ()):
            self._refs[blk] -= 1
            if self._refs[blk] == 0:
                self._free.append(blk)


def full_blocks(tokens: int, block_size: int) -> int:
    """Pages that `tokens` leading tokens fill completely - the only ones a
    prefix may share."""
    return max(tokens, 0) // block_size


def blocks_for(tokens: int, block_size: int) -> int:
    """Pages needed to hold `tokens` tokens."""
    return (max(tokens, 0) + block_size - 1) // block_size
