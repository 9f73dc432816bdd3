"""Case builders and the shape grid for ragged chunked-prefill attention:
sequence b continues by len_b query rows over a cached prefix of P_b rows,
the rows of all sequences packed one after another.

Plain helper module on top of extend_cases.py: torch on CPU only. A ragged
case is `ec.extend_case(...)` at chunk = max(lens) with only the first len_b
query rows of each sequence kept and packed. Row i < len_b of sequence b does
not depend on len_b (it sees the keys <= P_b + i and nothing else), so the
float64 reference is row i of `ec.extend_ref64` at chunk = max(lens): no new
mathematics. `lens_kv` = P_b + len_b is the first dead cache row of each
sequence, which is earlier than the uncut case's P_b + max(lens). The bound
is `ec.bound`. The split partials (m, s, o) are float32 and so is their
merge, as in the decode kernels whose tests use the same bound at 2-39
splits: no merge term is added.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

import extend_cases as ec
from attn_oracle import D

# One launch holds: a prefix of 0 with more than two q-tiles, a single row
# behind a long prefix, exactly one q-tile that starts one short of a kv
# tile edge, one row more than a q-tile, part of a q-tile past two kv tiles,
# and a sequence with no rows. The reverse pairing gives every prefix another
# length and puts the empty sequence first.
PREFIXES = (0, 200, 63, 1, 130, 64)
LENS = (130, 1, 64, 65, 17, 0)
PAIRINGS = {"forward": LENS, "reverse": LENS[::-1]}
SPLITS = (1, 2, 3, 7)       # 7 > tile count of the short sequences
LONG_PREFIXES = (2053, 1000)
LONG_LENS = (130, 7)


def pack(rows, lens, max_chunk):
    """[B*max_chunk, ...] -> the first lens[b] rows of each sequence."""
    rows = rows.reshape(len(lens), max_chunk, *rows.shape[1:])
    return torch.cat([rows[b, :n] for b, n in enumerate(lens)])


def ragged_case(family, prefixes, lens, hq, hk, dtype, pad_rows=0):
    """Packed ragged case; `pad_rows` rows of NaN that no sequence owns are
    appended to q (an op must neither read them into a result nor write
    them)."""
    max_chunk = max(lens)
    c = ec.extend_case(family, prefixes, max_chunk, hq, hk, dtype)
    q = pack(c.q, lens, max_chunk)
    if pad_rows:
        q = torch.cat([q, torch.full((pad_rows, hq, D), float("nan"),
                                     dtype=q.dtype)])
    chunk_lens = torch.tensor(lens, dtype=torch.int32)
    return SimpleNamespace(
        q=q.contiguous(), k=c.k, v=c.v, prefix_lens=c.prefix_lens,
        chunk_lens=chunk_lens,
        q_starts=(torch.cumsum(chunk_lens, 0) - chunk_lens).to(torch.int32),
        max_chunk=max_chunk, batch=len(lens), rows=sum(lens),
        lens_kv=[p + n for p, n in zip(prefixes, lens)], scale=c.scale,
        fp8=c.fp8)


@functools.lru_cache(maxsize=None)
def cached_ragged(family, prefixes, lens, hq, hk, dtype):
    """(case, ref, absref), built once per process and shared; ref and
    absref are [sum(lens), Hq, D] float64."""
    c = ragged_case(family, prefixes, lens, hq, hk, dtype)
    full = ec.extend_case(family, prefixes, c.max_chunk, hq, hk, dtype)
    ref, absref = ec.extend_ref64(full.q, full.k, full.v, full.prefix_lens,
                                  c.max_chunk, c.scale)
    return c, pack(ref, lens, c.max_chunk), pack(absref, lens, c.max_chunk)
