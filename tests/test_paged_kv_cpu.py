"""CPU tests of the paged KV cache: the references of the two paged ops
(which carry the kernels' skip, clamp and effective-context rules), the
block allocator, and LlamaDecodeModel(kv_layout="paged") on the CPU.

The clamp and skip guards are shown here and by reading the kernels; no GPU
test feeds a table entry outside the pool or a position past a reservation.
"""
import pytest
import torch

import attn_oracle as ao
import paged_cases as pc
from attn_oracle import BF16, FP8
from wva_amd import ops
from wva_amd.calibration.model import TINY, LlamaConfig, LlamaDecodeModel
from wva_amd.calibration.paged_kv import BlockAllocator

BLOCK_SIZES = (16, 32, 64)
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
APPEND_POSITIONS = pc.APPEND_POSITIONS
HQ, HK, D = pc.APPEND_HQ, pc.APPEND_HK, ao.D
append_inputs = pc.append_inputs


# --------------------------------------------------------------------------
# paged_decode_attn_ref
# --------------------------------------------------------------------------

@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_reference_equals_contiguous_reference(block_size):
    """Scattered over shuffled pages, with NaN in every unused page, dead
    row and behind every dead table entry, the paged reference is the
    contiguous reference bit for bit."""
    c = ao.edge_case(4, BF16, 1.0)
    p = pc.scatter_case(c, block_size)
    want = ops.gqa_decode_attn_ref(c.q, c.k, c.v, c.lens, c.scale)
    got = ops.paged_decode_attn_ref(c.q, p.k_pages, p.v_pages, p.tables,
                                    c.lens, c.scale)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    # the dispatching op takes the CPU reference
    out = ops.paged_decode_attn(c.q, p.k_pages, p.v_pages, p.tables, c.lens,
                                c.scale)
    assert torch.equal(out, want.to(BF16))


def test_reference_clamps_ids_and_context():
    """An id outside the pool is clamped into it, a context past the table
    is cut to max_blocks * block_size, and entries past the context are
    never looked at (here they are far outside the pool)."""
    c = ao.edge_case(4, BF16, 1.0)
    p = pc.scatter_case(c, 16)
    B, max_blocks = p.tables.shape
    tables = p.tables.clone()
    for b, n in enumerate(int(x) for x in c.lens):
        tables[b, pc.blocks_of(n, 16):] = 10 ** 6
    want = ops.gqa_decode_attn_ref(c.q, c.k, c.v, c.lens, c.scale)
    got = ops.paged_decode_attn_ref(c.q, p.k_pages, p.v_pages, tables,
                                    c.lens, c.scale)
    assert torch.equal(got, want)
    # ids below 0 / past the pool read page 0 / the last page
    lo = torch.full_like(tables, -5)
    hi = torch.full_like(tables, p.num_blocks + 9)
    zero = torch.zeros_like(tables)
    last = torch.full_like(tables, p.num_blocks - 1)
    full = torch.full((B,), max_blocks * 16, dtype=torch.int32)
    kz = torch.nan_to_num(p.k_pages.float()).to(BF16)
    vz = torch.nan_to_num(p.v_pages.float()).to(BF16)
    for bad, good in ((lo, zero), (hi, last)):
        assert torch.equal(
            ops.paged_decode_attn_ref(c.q, kz, vz, bad, full, c.scale),
            ops.paged_decode_attn_ref(c.q, kz, vz, good, full, c.scale))
    # context_lens past the table: the effective context is the table's span
    assert torch.equal(
        ops.paged_decode_attn_ref(c.q, kz, vz, zero, full + 1000, c.scale),
        ops.paged_decode_attn_ref(c.q, kz, vz, zero, full, c.scale))


# --------------------------------------------------------------------------
# rope_append_kv_paged
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_append_equals_contiguous_append_then_scatter(block_size, dtype):
    qkv, k, v, pos, lens = append_inputs(dtype, block_size)
    p = pc.scatter(k, v, lens, block_size)
    q_want = ops.rope_append_kv(qkv, k, v, pos, HQ, HK, ao.ROPE_THETA)
    want = pc.scatter(k, v, lens, block_size)   # same seed, same layout
    assert torch.equal(want.tables, p.tables)
    q_got = ops.rope_append_kv_paged(qkv, p.k_pages, p.v_pages, p.tables,
                                     pos, HQ, HK, ao.ROPE_THETA)
    assert torch.equal(q_got, q_want)
    assert torch.equal(pc.raw(p.k_pages), pc.raw(want.k_pages))
    assert torch.equal(pc.raw(p.v_pages), pc.raw(want.v_pages))
    # and something was written: the appended rows differ from before
    before = pc.scatter(*append_inputs(dtype, block_size)[1:3], lens,
                        block_size)
    assert not torch.equal(pc.raw(p.k_pages), pc.raw(before.k_pages))


@pytest.mark.parametrize("dtype", DTYPES)
def test_append_without_a_page_is_skipped(dtype):
    """An entry of -1, an entry past the pool or a position past
    max_blocks * block_size leaves the pool byte-identical and still
    returns q."""
    bs = 16
    qkv, k, v, pos, lens = append_inputs(dtype, bs)
    p = pc.scatter(k, v, lens, bs)
    q_want = ops.rope_append_kv_paged(
        qkv, p.k_pages.clone(), p.v_pages.clone(), p.tables, pos, HQ, HK,
        ao.ROPE_THETA)
    k0, v0 = pc.raw(p.k_pages).clone(), pc.raw(p.v_pages).clone()
    for bad in (-1, p.num_blocks, -(2 ** 31)):
        tables = torch.full_like(p.tables, bad)
        q = ops.rope_append_kv_paged(qkv, p.k_pages, p.v_pages, tables, pos,
                                     HQ, HK, ao.ROPE_THETA)
        assert torch.equal(q, q_want), bad
        assert torch.equal(pc.raw(p.k_pages), k0), bad
        assert torch.equal(pc.raw(p.v_pages), v0), bad
    # positions past the table (and a negative one): no store, q is RoPE'd
    max_pos = p.tables.shape[1] * bs
    far = torch.tensor([max_pos, max_pos + 1, max_pos + 16, 10 ** 6,
                        2 ** 31 - 1, -1, max_pos + 3, max_pos + 130],
                       dtype=torch.int32)
    q = ops.rope_append_kv_paged(qkv, p.k_pages, p.v_pages, p.tables, far,
                                 HQ, HK, ao.ROPE_THETA)
    assert torch.equal(pc.raw(p.k_pages), k0)
    assert torch.equal(pc.raw(p.v_pages), v0)
    q_in = qkv[:, :HQ * D].reshape(-1, HQ, D)
    q_ref, _ = ops.rope_ref(q_in, q_in[:, :1], far, ao.ROPE_THETA)
    assert torch.equal(q, q_ref.to(BF16))
    # one skipped sequence does not disturb its neighbours
    tables = p.tables.clone()
    tables[2, APPEND_POSITIONS[2] // bs] = -1
    ops.rope_append_kv_paged(qkv, p.k_pages, p.v_pages, tables, pos, HQ, HK,
                             ao.ROPE_THETA)
    page = int(p.tables[2, APPEND_POSITIONS[2] // bs])
    assert torch.equal(pc.raw(p.k_pages)[page], k0[page])
    changed = (pc.raw(p.k_pages) != k0).flatten(1).any(dim=1).sum()
    assert int(changed) == len(APPEND_POSITIONS) - 1


# --------------------------------------------------------------------------
# BlockAllocator
# --------------------------------------------------------------------------

class TestBlockAllocator:
    def test_free_plus_live_is_total(self):
        a = BlockAllocator(10, seed=1)
        assert (a.num_free, a.num_live) == (10, 0)
        got = a.allocate("a", 3) + a.allocate("b", 4)
        assert len(set(got)) == 7 and all(0 <= g < 10 for g in got)
        assert (a.num_free, a.num_live) == (3, 7)
        a.allocate("a", 1)
        assert a.blocks("a") == got[:3] + a.blocks("a")[3:]
        assert a.num_free + a.num_live == 10
        a.free("a")
        assert (a.num_free, a.num_live) == (6, 4)
        a.free("b")
        assert (a.num_free, a.num_live) == (10, 0)

    def test_seeded_shuffle(self):
        a, b = BlockAllocator(64, seed=5), BlockAllocator(64, seed=5)
        x = a.allocate(0, 64)
        assert x == b.allocate(0, 64)
        assert sorted(x) == list(range(64)) and x != list(range(64))
        assert BlockAllocator(64).allocate(0, 64) == list(range(64))
        a.reset()
        assert a.allocate(0, 64) == x

    def test_sharing_keeps_blocks_until_both_are_freed(self):
        for first, second in (("a", "b"), ("b", "a")):
            a = BlockAllocator(8, seed=0)
            a.allocate("a", 4)
            shared = a.share("a", "b", 2)
            assert shared == a.blocks("a")[:2] == a.blocks("b")
            a.allocate("b", 2)
            assert a.blocks("b")[:2] == shared
            assert (a.num_free, a.num_live) == (2, 6)
            assert [a.refcount(s) for s in shared] == [2, 2]
            a.free(first)
            assert [a.refcount(s) for s in shared] == [1, 1]
            assert (a.num_free, a.num_live) == (4, 4)
            # the shared blocks are not handed out again
            assert not set(a.allocate("c", 4)) & set(shared)
            a.free("c")
            a.free(second)
            assert (a.num_free, a.num_live) == (8, 0)
            assert sorted(a.allocate("d", 8)) == list(range(8))

    def test_exhaustion_raises_and_names_the_counts(self):
        a = BlockAllocator(4)
        a.allocate("a", 3)
        with pytest.raises(RuntimeError, match=r"2 blocks requested, 1 free"):
            a.allocate("b", 2)
        assert (a.num_free, a.num_live) == (1, 3)   # nothing was taken
        assert a.blocks("b") == []

    def test_only_full_blocks_are_shared(self):
        from wva_amd.calibration.paged_kv import full_blocks

        assert [full_blocks(n, 16) for n in (0, 15, 16, 17, 47, 48)] == \
            [0, 0, 1, 1, 2, 3]
        a = BlockAllocator(8)
        a.allocate("a", 2)
        with pytest.raises(ValueError):
            a.share("a", "b", 3)     # more than the sequence owns
        a.share("a", "b", 1)
        with pytest.raises(ValueError):
            a.share("a", "b", 1)     # the receiver already owns blocks


# --------------------------------------------------------------------------
# LlamaDecodeModel(kv_layout="paged") on the CPU
# --------------------------------------------------------------------------

MICRO = LlamaConfig(name="micro", hidden_size=256, intermediate_size=512,
                    num_layers=2, num_q_heads=2, num_kv_heads=1,
                    vocab_size=64)


def micro(**kw):
    kw.setdefault("max_batch", 4)
    kw.setdefault("max_seq", 128)
    return LlamaDecodeModel(MICRO, device="cpu", kv_layout="paged", **kw)


def test_model_paged_equals_contiguous_on_cpu():
    """TINY, paged (16) against contiguous with the same seed, both from
    reset(b, 0): after 20 identical decode steps the logits are equal."""
    kw = dict(max_batch=3, max_seq=32, device="cpu", seed=4)
    ref = LlamaDecodeModel(TINY, **kw)
    paged = LlamaDecodeModel(TINY, kv_layout="paged", block_size=16, **kw)
    ref.reset(3, 0)
    paged.reset(3, 0)
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        tok = torch.randint(0, TINY.vocab_size, (3,), generator=g)
        a, b = ref.decode_step(tok), paged.decode_step(tok)
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, b)
    assert torch.equal(ref.context_lens, paged.context_lens)
    assert int(paged.context_lens[0]) == 20


class TestPagedReset:
    def test_tables_are_shuffled_and_unreserved_entries_are_minus_one(self):
        m = micro()
        storage = m.block_tables.data_ptr()
        m.reset(3, 20, headroom=12)
        t = m.block_tables
        assert t.data_ptr() == storage and t.dtype == torch.int32
        assert t.shape == (4, 128 // 16)
        used = t[:3, :2].reshape(-1).tolist()
        assert len(set(used)) == 6 and all(0 <= u < 32 for u in used)
        assert used != sorted(used) and used != list(range(6))
        assert bool((t[:3, 2:] == -1).all()) and bool((t[3] == -1).all())
        assert m.context_lens.tolist() == [20, 20, 20, 0]
        assert m.allocator.num_live == 6
        # headroom=None reserves up to max_seq; reset frees what was there
        m.reset(2, 5)
        assert bool((m.block_tables[:2] >= 0).all())
        assert bool((m.block_tables[2:] == -1).all())
        assert m.allocator.num_live == 16
        assert m.block_tables.data_ptr() == storage

    def test_live_rows_are_filled(self):
        m = micro()
        m.reset(2, 20, headroom=0)
        ids = m.block_tables[:2, :2].reshape(-1).long()
        for pool in (*m.k_pages, *m.v_pages):
            assert bool((pool[ids].float().abs().sum(dim=(1, 2, 3)) > 0).all())
            rest = torch.ones(32, dtype=torch.bool)
            rest[ids] = False
            assert bool((pool[rest] == 0).all())

    @pytest.mark.parametrize("shared_prefix", (0, 15, 16, 40, 48))
    def test_shared_prefix_aliases_full_blocks_only(self, shared_prefix):
        m = micro()
        m.reset(4, 50, headroom=10, shared_prefix=shared_prefix)
        t = m.block_tables
        k = shared_prefix // 16
        assert bool((t[:, :k] == t[0, :k]).all())
        own = t[:, k:4].reshape(-1).tolist()
        assert len(set(own)) == len(own)            # nothing else aliases
        assert not set(own) & set(t[0, :k].tolist())
        assert m.allocator.num_live == k + 4 * (4 - k)

    def test_a_pool_too_small_raises(self):
        m = micro(num_gpu_blocks=6)
        m.reset(3, 20, headroom=12)                 # 3 x 2 blocks fit
        with pytest.raises(RuntimeError, match="pool too small"):
            m.reset(4, 20, headroom=12)
        with pytest.raises(RuntimeError, match="pool too small"):
            m.reset(1, 5)                           # up to max_seq: 8 blocks
        # many short sequences in a small pool
        m = micro(num_gpu_blocks=6, max_batch=6)
        m.reset(6, 10, headroom=4)
        assert m.allocator.num_free == 0
        # sharing makes room
        m = micro(num_gpu_blocks=6)
        m.reset(4, 32, headroom=0, shared_prefix=16)   # 1 + 4 blocks

    def test_bad_arguments(self):
        with pytest.raises(ValueError):
            micro(max_seq=100)                      # not a multiple of 16
        with pytest.raises(ValueError):
            micro(block_size=8)
        with pytest.raises(ValueError):
            LlamaDecodeModel(MICRO, device="cpu", max_batch=2, max_seq=32,
                             kv_layout="blocked")
        m = micro()
        with pytest.raises(ValueError):
            m.reset(2, 100, headroom=100)           # past max_seq

    def test_prefill_family_is_decode_only(self):
        m = micro()
        m.reset(2, 0)
        tok = torch.zeros(2, 4, dtype=torch.long)
        lens = torch.tensor([2, 2], dtype=torch.int32)
        for call in (
            lambda: m.prefill(tok),
            lambda: m.prefill(tok, chunk_size=2),
            lambda: m.prefill_chunk(tok),
            lambda: m.mixed_step(tok[:1, 0], tok[1:]),
            lambda: m.ragged_step(None, tok.reshape(-1)[:4], lens, 2),
        ):
            with pytest.raises(NotImplementedError,
                               match="paged KV: decode path only"):
                call()

    def test_contiguous_default_is_untouched(self):
        m = LlamaDecodeModel(MICRO, device="cpu", max_batch=2, max_seq=32)
        assert m.kv_layout == "contiguous" and not hasattr(m, "block_tables")
        assert m.k_cache[0].shape == (2, 1, 32, 128)
        with pytest.raises(ValueError):
            m.reset(2, 4, headroom=4)
