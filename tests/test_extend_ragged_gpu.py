"""GPU tests of ragged chunked-prefill attention (ops.extend_attn_ragged:
the RAGGED instantiation of the flash-prefill kernel, its split-KV sweep and
merge) and of the engine's ragged_step.

The cases and the grid are ragged_cases.py, the float64 reference is
extend_cases.extend_ref64 cut to the packed rows, the bound is `ec.bound`.
test_extend_ragged_cpu.py shows on the CPU that these cases and that bound
reject a kernel that takes P_b + max_chunk for the live rows, offsets rows
by b * max_chunk, merges without weights, counts an empty split, drops the
last tile of a sweep or writes a row for an empty sequence. No test here
launches an out-of-range length, start or prefix. Each test prints its worst
err/bound ratio (`-s` shows them; docs/testing.md records them).
"""
import pytest
import torch

import attn_oracle as ao
import extend_cases as ec
import ragged_cases as rc
from attn_oracle import BF16, FP8
from wva_amd import ops

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
PAIRINGS = list(rc.PAIRINGS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(what, dtype, ratio, note=""):
    name = "fp8" if dtype == FP8 else "bf16"
    print(f"\n[ragged] {what} dtype={name} ratio={ratio:.3f} {note}")


def ragged(c, dev, num_splits, k=None, v=None, q=None):
    k = c.k if k is None else k
    v = c.v if v is None else v
    q = c.q if q is None else q
    return ops.extend_attn_ragged(
        q.to(dev), k.to(dev), v.to(dev), c.prefix_lens.to(dev),
        c.chunk_lens.to(dev), c.max_chunk, c.scale, num_splits).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_unsplit_is_bit_equal_to_per_sequence_extend_attn(dev, pairing, dtype):
    """q-tiles start at the chunk's first row and kv tiles are aligned at 0
    in both, so each row goes through the same tiles, masks and
    floating-point sequence as in a launch of its sequence alone."""
    lens = rc.PAIRINGS[pairing]
    c, _, _ = rc.cached_ragged("sentinel", rc.PREFIXES, lens, 8, 2, dtype)
    got = ragged(c, dev, 1)
    parts = []
    for b, n in enumerate(lens):
        if n == 0:
            continue
        lo = int(c.q_starts[b])
        parts.append(ops.extend_attn(
            c.q[lo:lo + n].to(dev), c.k[b:b + 1].to(dev),
            c.v[b:b + 1].to(dev), c.prefix_lens[b:b + 1].to(dev), n,
            c.scale).cpu())
    want = torch.cat(parts)
    assert torch.equal(got, want), (
        f"max |diff| = {float((got.float() - want.float()).abs().max()):g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunk", (17, 65, 130))
def test_equal_lengths_unsplit_is_bit_equal_to_extend_attn(dev, chunk, dtype):
    c, _, _ = ec.cached_extend("sentinel", (63, 65), chunk, 8, 2, dtype)
    q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
    P = c.prefix_lens.to(dev)
    lens = torch.full((2,), chunk, dtype=torch.int32, device=dev)
    one = ops.extend_attn(q, k, v, P, chunk, c.scale)
    got = ops.extend_attn_ragged(q, k, v, P, lens, chunk, c.scale, 1)
    assert torch.equal(one, got), (
        f"max |diff| = {float((one.float() - got.float()).abs().max()):g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ec.HEADS)
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_shape_grid(dev, family, hq, hk, dtype):
    """Both pairings of the grid at 1, 2, 3 and 7 splits (7 is more than the
    tile count of the short sequences, so some splits are empty)."""
    worst = 0.0
    for name, lens in rc.PAIRINGS.items():
        c, ref, absref = rc.cached_ragged(family, rc.PREFIXES, lens, hq, hk,
                                          dtype)
        for n in rc.SPLITS:
            r = ao.assert_within(ragged(c, dev, n), ref,
                                 ec.bound(ref, absref),
                                 f"{family} {name} splits={n}")
            worst = max(worst, r)
    record(family, dtype, worst, f"{hq}/{hk} worst over the grid")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_splits", (1, 3))
@pytest.mark.parametrize("pairing,exact", [("forward", False),
                                           ("reverse", False),
                                           ("forward", True)])
def test_dead_rows_are_never_read(dev, pairing, exact, num_splits, dtype):
    """Cache rows >= P_b + len_b (not P_b + max_chunk) hold NaN, the largest
    finite value or zero: the three outputs are bit-equal, finite and within
    bound. With `exact` the caches are sliced so that max(P_b + len_b) ==
    S_max."""
    lens = rc.PAIRINGS[pairing]
    c, ref, absref = rc.cached_ragged("sentinel", rc.PREFIXES, lens, 8, 2,
                                      dtype)
    k, v = c.k, c.v
    if exact:
        S = max(c.lens_kv)
        k, v = k[:, :, :S].contiguous(), v[:, :, :S].contiguous()
        assert k.shape[2] == max(c.lens_kv)
    outs = {}
    for kind in ("zero", "nan", "max"):
        kp, vp = ao.poison_dead_rows(k, v, c.lens_kv, kind)
        outs[kind] = ragged(c, dev, num_splits, kp, vp)
    assert bool(torch.isfinite(outs["nan"].float()).all())
    assert torch.equal(outs["zero"], outs["nan"])
    assert torch.equal(outs["zero"], outs["max"])
    r = ao.assert_within(outs["zero"], ref, ec.bound(ref, absref),
                         f"poison {pairing} splits={num_splits}")
    record("poison", dtype, r,
           f"{pairing} splits={num_splits} exact={exact}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_splits", (1, 3))
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_empty_sequence_and_uncovered_rows(dev, pairing, num_splits, dtype):
    """T > sum(lens), the rows no sequence owns holding NaN: they come back
    as 0, and the other sequences' rows are bit-equal to the launch without
    the empty sequence."""
    lens = rc.PAIRINGS[pairing]
    c, _, _ = rc.cached_ragged("sentinel", rc.PREFIXES, lens, 8, 2, dtype)
    padded = rc.ragged_case("sentinel", rc.PREFIXES, lens, 8, 2, dtype,
                            pad_rows=5)
    got = ragged(c, dev, num_splits, q=padded.q)
    assert got.shape[0] == c.rows + 5
    assert bool((got[c.rows:] == 0).all())
    keep = [b for b, n in enumerate(lens) if n]
    assert len(keep) == len(lens) - 1
    without = ops.extend_attn_ragged(
        c.q.to(dev), c.k[keep].to(dev), c.v[keep].to(dev),
        c.prefix_lens[keep].to(dev), c.chunk_lens[keep].to(dev), c.max_chunk,
        c.scale, num_splits).cpu()
    assert torch.equal(got[:c.rows], without)


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_prefix_takes_the_split_path(dev, dtype):
    c, ref, absref = rc.cached_ragged("sentinel", rc.LONG_PREFIXES,
                                      rc.LONG_LENS, 8, 2, dtype)
    splits = ops.extend_attn_ragged_num_splits(2, 8, 130, c.k.shape[2])
    assert splits == 18, splits           # pairs of tiles in 2191 rows
    r = ao.assert_within(ragged(c, dev, None), ref, ec.bound(ref, absref),
                         f"long prefix P={rc.LONG_PREFIXES}")
    record("long-prefix", dtype, r,
           f"P={rc.LONG_PREFIXES} lens={rc.LONG_LENS} splits={splits}")


def test_split_heuristic_on_static_shapes():
    n = ops.extend_attn_ragged_num_splits
    assert n(1, 32, 2048, 2048) == 1       # the q-tiles fill the machine
    assert n(1, 32, 64, 100) == 1          # a single pair of kv tiles
    assert n(1, 32, 64, 8192 + 64) == 24   # the weak shape: the cap
    assert n(1, 32, 256, 8192 + 256) == 16
    assert n(1, 32, 512, 8192 + 512) == 8
    assert n(4, 32, 512, 8192 + 512) == 1


def test_binding_checks(dev):
    c, _, _ = rc.cached_ragged("sentinel", rc.PREFIXES, rc.LENS, 8, 2, BF16)
    ext = ops._require_ext()
    q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
    P, Q, L = (t.to(dev) for t in (c.prefix_lens, c.q_starts, c.chunk_lens))
    C = c.max_chunk
    with pytest.raises(RuntimeError, match="int32"):
        ext.extend_attn_ragged(q, k, v, P, Q, L.long(), C, c.scale, 1)
    with pytest.raises(RuntimeError, match="prefix_lens"):
        ext.extend_attn_ragged(q, k, v, P[:2], Q, L, C, c.scale, 1)
    with pytest.raises(RuntimeError, match="q_starts"):
        ext.extend_attn_ragged(q, k, v, P, Q[:2], L, C, c.scale, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.extend_attn_ragged(q, k, v, P, Q, c.chunk_lens, C, c.scale, 1)
    with pytest.raises(RuntimeError, match="max_chunk"):
        ext.extend_attn_ragged(q, k, v, P, Q, L, k.shape[2] + 1, c.scale, 1)
    with pytest.raises(RuntimeError, match="num_splits"):
        ext.extend_attn_ragged(q, k, v, P, Q, L, C, c.scale, 0)
    with pytest.raises(RuntimeError, match="fewer than B"):
        ext.extend_attn_ragged(q, k[:3], v[:3], P, Q, L, C, c.scale, 1)


# --------------------------------------------------------------------------
# engine (TINY; tolerance of test_extend_attn_gpu's engine tests)
# --------------------------------------------------------------------------

TOL = dict(atol=8e-2, rtol=8e-2)


def tiny(seed=21, max_batch=4, max_seq=64, **kw):
    from wva_amd.calibration.model import TINY, LlamaDecodeModel
    return LlamaDecodeModel(TINY, max_batch=max_batch, max_seq=max_seq,
                            seed=seed, **kw)


def tokens_of(shape, seed, dev):
    from wva_amd.calibration.model import TINY
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, TINY.vocab_size, shape, generator=g).to(dev)


class TestRaggedEngineGpu:
    def test_equal_lengths_match_mixed_step(self, dev):
        Bd, Bp, C, ctx = 2, 2, 9, 11
        prompt = tokens_of((Bd + Bp, ctx), 3, dev)
        dec = tokens_of((Bd,), 4, dev)
        chunk = tokens_of((Bp, C), 5, dev)
        rag, mixed = tiny(), tiny()
        for m in (rag, mixed):
            m.prefill(prompt)
            m.decode_step(prompt[:1, 0])                # row 0 is one ahead
        want = mixed.mixed_step(dec, chunk)
        lens = torch.full((Bp,), C, dtype=torch.int32, device=dev)
        got = rag.ragged_step(dec, chunk.reshape(-1), lens, C)
        torch.testing.assert_close(got.float(), want.float(), **TOL)
        assert torch.equal(rag.context_lens, mixed.context_lens)

    def test_unequal_lengths_match_separate_prefill_chunks(self, dev):
        Bd, lens, ctx = 1, (9, 4, 0), 11
        prompt = tokens_of((Bd + 3, ctx), 3, dev)
        dec = tokens_of((Bd,), 4, dev)
        chunks = [tokens_of((1, n), 10 + n, dev) for n in lens]
        m, ref = tiny(), tiny()
        for x in (m, ref):
            x.prefill(prompt)
        before = m.k_cache[0][Bd + 2].clone()
        got = m.ragged_step(
            dec, torch.cat([c[0] for c in chunks]),
            torch.tensor(lens, dtype=torch.int32, device=dev), max(lens))
        assert m.context_lens[:4].tolist() == [ctx + 1, ctx + 9, ctx + 4, ctx]
        assert torch.equal(m.k_cache[0][Bd + 2], before)
        want_dec = ref.decode_step(dec)
        torch.testing.assert_close(got[:Bd].float(), want_dec.float(), **TOL)
        for b, n in enumerate(lens):
            if n == 0:
                continue
            solo = tiny()
            solo.prefill(prompt[Bd + b:Bd + b + 1])
            want = solo.prefill_chunk(chunks[b])
            torch.testing.assert_close(got[Bd + b:Bd + b + 1].float(),
                                       want.float(), **TOL)

    def test_fp8_kv_ragged_step_then_decode(self, dev):
        m = tiny(kv_dtype="fp8")
        m.prefill(tokens_of((3, 8), 6, dev))
        lens = (5, 0, 12)
        logits = m.ragged_step(
            None, tokens_of((sum(lens),), 7, dev),
            torch.tensor(lens, dtype=torch.int32, device=dev), max(lens))
        assert m.context_lens[:3].tolist() == [13, 8, 20]
        assert bool(torch.isfinite(logits[[0, 2]].float()).all())
        logits = m.decode_step(tokens_of((3,), 8, dev))
        assert m.context_lens[:3].tolist() == [14, 9, 21]
        assert bool(torch.isfinite(logits.float()).all())

    def test_measure_ragged_itl_returns_a_positive_number(self, dev):
        from wva_amd.calibration.itl_benchmark import measure_ragged_itl

        m = tiny(max_batch=5, max_seq=64)
        assert measure_ragged_itl(m, decode_batch=2, context_len=16,
                                  chunk_lens=(16, 5, 0), iters=2,
                                  warmup=1) > 0
