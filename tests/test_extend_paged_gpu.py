"""GPU tests of paged chunked prefill: ops.extend_attn_ragged_paged (the
PAGED instantiations of the flash-prefill kernel), ops.rope_append_kv_chunk_paged
(rope_append_kv_chunk_kernel) and the engine's paged_ragged_step.

The attention condition is derived, not tuned: PAGED changes addresses only,
so on the rows of a ragged_cases.py case scattered by paged_cases.py
(shuffled pages; NaN / 0x7f in every spare page, dead row and behind every
dead table entry) the output is torch.equal to ops.extend_attn_ragged on the
contiguous case at the same split count, and within `ec.bound` of its float64
reference. The append is held to the bounds of
test_attention_edges_gpu.py::test_rope_append_kv. No test launches a corrupt
table or an out-of-range length; the skip rule is exercised only through a -1
entry and the end of a table, which the kernel handles before any store.
"""
import pytest
import torch

import attn_oracle as ao
import extend_cases as ec
import paged_cases as pc
import ragged_cases as rc
from attn_oracle import BF16, FP8, D
from paged_chunk_case import HK, HQ, append_case
from wva_amd import ops

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def put(t, dev):
    """e4m3 tensors are moved as bytes."""
    if t.dtype == FP8:
        return t.view(torch.uint8).to(dev).view(FP8)
    return t.to(dev)


def paged_attn(c, p, dev, num_splits):
    return ops.extend_attn_ragged_paged(
        c.q.to(dev), put(p.k_pages, dev), put(p.v_pages, dev),
        p.tables.to(dev), c.prefix_lens.to(dev), c.chunk_lens.to(dev),
        c.max_chunk, c.scale, num_splits).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", (16, 64))
@pytest.mark.parametrize("pairing", list(rc.PAIRINGS))
@pytest.mark.parametrize("num_splits", (1, 3))
def test_attention_is_bit_equal_to_contiguous(dev, num_splits, pairing, bs,
                                              dtype):
    c, ref, absref = rc.cached_ragged("sentinel", rc.PREFIXES,
                                      rc.PAIRINGS[pairing], 8, 2, dtype)
    p = pc.scatter(c.k, c.v, c.lens_kv, bs)
    got = paged_attn(c, p, dev, num_splits)
    want = ops.extend_attn_ragged(
        c.q.to(dev), put(c.k, dev), put(c.v, dev), c.prefix_lens.to(dev),
        c.chunk_lens.to(dev), c.max_chunk, c.scale, num_splits).cpu()
    assert bool(torch.isfinite(got.float()).all())
    r = ao.assert_within(got, ref, ec.bound(ref, absref),
                         f"paged {pairing} bs={bs} splits={num_splits}")
    print(f"\n[paged-extend] {pairing} bs={bs} splits={num_splits} "
          f"ratio={r:.3f}")
    assert torch.equal(got, want), (
        f"max |diff| = {float((got.float() - want.float()).abs().max()):g}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_prefix_takes_the_split_path(dev, dtype):
    c, ref, absref = rc.cached_ragged("sentinel", rc.LONG_PREFIXES,
                                      rc.LONG_LENS, 8, 2, dtype)
    p = pc.scatter(c.k, c.v, c.lens_kv, 32)
    splits = ops.extend_attn_ragged_num_splits(2, 8, 130,
                                               p.tables.shape[1] * 32)
    assert splits > 1, splits
    r = ao.assert_within(paged_attn(c, p, dev, None), ref,
                         ec.bound(ref, absref), "paged long prefix")
    print(f"\n[paged-extend] long prefix splits={splits} ratio={r:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", (16, 64))
def test_chunk_append(dev, bs, dtype):
    """q and a bf16 K within the rope bound, an fp8 K within one e4m3 ulp of
    the quantised float64 rotation, V a copy; every pool byte outside the
    rows that have a page unchanged (so the rows on the -1 entry and past
    the table stored nothing), their q rows held to the same bound."""
    c = append_case(dtype, bs)
    kp, vp = put(c.k_pages, dev), put(c.v_pages, dev)
    q = ops.rope_append_kv_chunk_paged(
        c.qkv.to(dev), kp, vp, c.tables.to(dev), c.prefix.to(dev),
        c.lens.to(dev), c.max_chunk, HQ, HK, ao.ROPE_THETA).cpu()
    kp, vp = put(kp, "cpu"), put(vp, "cpu")
    T = c.qkv.shape[0]
    q_in, k_in, v_in = (t.reshape(T, -1, D) for t in c.qkv.split(
        [HQ * D, HK * D, HK * D], dim=1))
    ref = ao.rope_ref64(q_in, c.pos)
    ao.assert_within(q, ref, ao.rope_bound(q_in, ref, c.pos), "q")
    rows = torch.nonzero(c.paged).flatten()
    page = c.tables[c.seq[rows], c.pos[rows] // bs].long()
    slot = c.pos[rows] % bs
    k_new = pc.raw(kp)[page, :, slot].view(dtype)     # [rows, Hk, D]
    v_new = pc.raw(vp)[page, :, slot].view(dtype)
    k_ref = ao.rope_ref64(k_in, c.pos)[rows]
    if dtype == FP8:
        assert torch.equal(pc.raw(v_new), pc.raw(v_in[rows].to(FP8)))
        want = k_ref.float().to(FP8).float().double()
        ulp = ao.e4m3_ulp(torch.maximum(want.abs(), k_new.float().abs()))
        ao.assert_within(k_new.float(), want, ulp, "fp8 k")
    else:
        assert torch.equal(v_new, v_in[rows])
        ao.assert_within(k_new, k_ref,
                         ao.rope_bound(k_in, ao.rope_ref64(k_in, c.pos),
                                       c.pos)[rows], "bf16 k")
    for got, old in ((kp, c.k_pages), (vp, c.v_pages)):
        untouched = torch.ones(pc.raw(got).shape[:3], dtype=torch.bool)
        untouched.transpose(1, 2)[page, slot] = False
        assert int((~untouched).sum()) == len(rows) * HK
        assert torch.equal(pc.raw(got)[untouched], pc.raw(old)[untouched])


TOL = dict(atol=8e-2, rtol=8e-2)   # the engine tests of test_extend_ragged_gpu


@pytest.mark.parametrize("kv_dtype", ("bf16", "fp8"))
def test_engine_paged_ragged_step(dev, kv_dtype):
    """TINY: the prompts through paged_ragged_step from an empty cache
    (against prefill), one mixed iteration with chunks of 9, 4 and 0 (against
    ragged_step), one decode step. fp8 KV: finite logits and the lengths."""
    from wva_amd.calibration.model import TINY, LlamaDecodeModel

    kw = dict(max_batch=4, max_seq=64, seed=21, kv_dtype=kv_dtype)
    ref = LlamaDecodeModel(TINY, **kw)
    m = LlamaDecodeModel(TINY, kv_layout="paged", block_size=16, **kw)
    g = torch.Generator().manual_seed(3)
    toks = lambda *s: torch.randint(0, TINY.vocab_size, s, generator=g).to(dev)
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32, device=dev)
    prompt, dec, chunk, last = toks(4, 11), toks(1), toks(13), toks(4)
    m.reset(4, 0, headroom=40)
    pairs = [(m.paged_ragged_step(None, prompt.reshape(-1),
                                  i32(11, 11, 11, 11), 11),
              ref.prefill(prompt))]
    got = m.paged_ragged_step(dec, chunk, i32(9, 4, 0), 9)
    want = ref.ragged_step(dec, chunk, i32(9, 4, 0), 9)
    pairs += [(got[:3], want[:3]), (m.decode_step(last), ref.decode_step(last))]
    assert m.context_lens.tolist() == [13, 21, 16, 12]
    assert torch.equal(m.context_lens, ref.context_lens)
    for got, want in pairs:
        assert bool(torch.isfinite(got.float()).all())
        if kv_dtype == "bf16":
            torch.testing.assert_close(got.float(), want.float(), **TOL)


def test_binding_checks(dev):
    c, _, _ = rc.cached_ragged("sentinel", rc.PREFIXES, rc.LENS, 8, 2, BF16)
    p = pc.scatter(c.k, c.v, c.lens_kv, 16)
    q, kp, vp, t = (x.to(dev) for x in (c.q, p.k_pages, p.v_pages, p.tables))
    P, L = c.prefix_lens.to(dev), c.chunk_lens.to(dev)
    run = lambda kp=kp, vp=vp, t=t, n=1: ops.extend_attn_ragged_paged(
        q, kp, vp, t, P, L, c.max_chunk, c.scale, n)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        run(vp=vp.float())
    with pytest.raises(RuntimeError, match="block_tables"):
        run(t=t[:2])
    with pytest.raises(RuntimeError, match="block_size"):
        run(kp=kp[:, :, :8].contiguous(), vp=vp[:, :, :8].contiguous())
    with pytest.raises(RuntimeError, match="num_splits"):
        run(n=0)
    with pytest.raises(RuntimeError, match="qkv"):
        ops.rope_append_kv_chunk_paged(q.reshape(q.shape[0], -1), kp, vp, t,
                                       P, L, c.max_chunk, 8, 2)
