"""CPU side of the paged chunked-prefill tests: the CPU routes of
ops.extend_attn_ragged_paged and ops.rope_append_kv_chunk_paged (which carry
the kernels' clamp and skip rules) against the ops they extend, and
LlamaDecodeModel.paged_ragged_step against the contiguous ragged_step.

The append case is paged_chunk_case.py, shared with test_extend_paged_gpu.py.
"""
import pytest
import torch

import attn_oracle as ao
import paged_cases as pc
import ragged_cases as rc
from attn_oracle import BF16, FP8
from paged_chunk_case import HK, HQ, append_case
from wva_amd import ops
from wva_amd.calibration.model import LlamaConfig, LlamaDecodeModel

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", (16, 64))
def test_chunk_append_equals_row_by_row_paged_append(bs, dtype):
    """One call for all chunks against rope_append_kv_paged a row at a time:
    q equal, pools byte-equal (the rows without a page were skipped by both),
    and the rows with a page were written."""
    c = append_case(dtype, bs)
    k0, v0 = c.k_pages.clone(), c.v_pages.clone()
    q = ops.rope_append_kv_chunk_paged(
        c.qkv, c.k_pages, c.v_pages, c.tables, c.prefix, c.lens, c.max_chunk,
        HQ, HK, ao.ROPE_THETA)
    for r in range(c.qkv.shape[0]):
        b = int(c.seq[r])
        q_r = ops.rope_append_kv_paged(
            c.qkv[r:r + 1], k0, v0, c.tables[b:b + 1],
            c.pos[r:r + 1].to(torch.int32), HQ, HK, ao.ROPE_THETA)
        assert torch.equal(q[r:r + 1], q_r), r
    assert torch.equal(pc.raw(c.k_pages), pc.raw(k0))
    assert torch.equal(pc.raw(c.v_pages), pc.raw(v0))
    fresh = append_case(dtype, bs)
    changed = (pc.raw(c.v_pages) != pc.raw(fresh.v_pages)).any(dim=3).any(dim=1)
    assert int(changed.sum()) == int(c.paged.sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", (16, 64))
@pytest.mark.parametrize("pairing", list(rc.PAIRINGS))
def test_paged_attention_route_equals_contiguous_route(pairing, bs, dtype):
    c, _, _ = rc.cached_ragged("sentinel", rc.PREFIXES, rc.PAIRINGS[pairing],
                               8, 2, dtype)
    p = pc.scatter(c.k, c.v, c.lens_kv, bs)
    want = ops.extend_attn_ragged(c.q, c.k, c.v, c.prefix_lens, c.chunk_lens,
                                  c.max_chunk, c.scale)
    got = ops.extend_attn_ragged_paged(
        c.q, p.k_pages, p.v_pages, p.tables, c.prefix_lens, c.chunk_lens,
        c.max_chunk, c.scale)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, want)


MICRO = LlamaConfig(name="micro", hidden_size=256, intermediate_size=512,
                    num_layers=2, num_q_heads=2, num_kv_heads=1,
                    vocab_size=64)


def test_engine_paged_ragged_step_equals_contiguous_ragged_step():
    """Prompts of 11 tokens through a ragged step from an empty cache, then
    one mixed iteration (1 decode row, chunks of 9, 4 and 0), then a decode
    step: equal logits and context_lens."""
    kw = dict(max_batch=4, max_seq=64, device="cpu", seed=3)
    ref = LlamaDecodeModel(MICRO, **kw)
    m = LlamaDecodeModel(MICRO, kv_layout="paged", block_size=16, **kw)
    ref.reset(4, 0)
    m.reset(4, 0, headroom=40)
    g = torch.Generator().manual_seed(1)
    toks = lambda n: torch.randint(0, MICRO.vocab_size, (n,), generator=g)
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)
    steps = [(None, toks(44), i32(11, 11, 11, 11), 11),
             (toks(1), toks(13), i32(9, 4, 0), 9)]
    for dec, chunk, lens, max_chunk in steps:
        want = ref.ragged_step(dec, chunk, lens, max_chunk)
        got = m.paged_ragged_step(dec, chunk, lens, max_chunk)
        keep = torch.cat([torch.ones(len(got) - len(lens), dtype=torch.bool),
                          lens > 0])        # a row of no tokens is unspecified
        assert torch.equal(got[keep], want[keep])
        assert torch.equal(m.context_lens, ref.context_lens)
    tok = toks(4)
    assert torch.equal(m.decode_step(tok), ref.decode_step(tok))
    assert m.context_lens.tolist() == [13, 21, 16, 12]
    with pytest.raises(ValueError, match="paged"):
        ref.paged_ragged_step(None, toks(4), i32(4), 4)
