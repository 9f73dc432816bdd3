"""CPU side of the ragged chunked-prefill attention tests.

A float32 emulation of prefill_attn_kernel<*, prefix, RAGGED> and its merge
(packed rows at q_starts[b], live cache rows P_b + len_b, 64-key tiles
aligned at 0 and dealt to the splits round-robin, unnormalised (m, s, o)
partials, the exp(m_s - m) merge, every clamp of the kernel) stays within
`ec.bound` on the grid of ragged_cases.py at 1, 2, 3 and 7 splits, and six
mutants of it are each far outside the bound, so test_extend_ragged_gpu.py
can see those mistakes in the HIP kernel. Also: the ragged reference against
a naive loop, ops.extend_attn_ragged_ref and the CPU routing of
ops.extend_attn_ragged, and the engine's ragged_step on the tiny config.
"""
import math

import pytest
import torch

import attn_oracle as ao
import extend_cases as ec
import ragged_cases as rc
from attn_oracle import BF16, FP8, TILE
from wva_amd import ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
MUTANTS = ("kv-len-max-chunk", "row-offset", "merge-unweighted",
           "empty-split-exp0", "drop-last-tile", "len0-writes")


def emulate_ragged(c, num_splits, mutant=None, k=None, v=None, q_starts=None,
                   chunk_lens=None, prefix_lens=None):
    """Float32 emulation of the ragged launch: the attention kernel on the
    grid (B·Hq, ceil(max_chunk/64), num_splits), then the merge. The three
    device tensors may be overridden with out-of-range contents; they only
    ever pass through the kernel's clamps."""
    T, Hq, D = c.q.shape
    B, Hk, S_max, _ = c.k.shape
    G = Hq // Hk
    N = num_splits
    q_starts = c.q_starts if q_starts is None else q_starts
    chunk_lens = c.chunk_lens if chunk_lens is None else chunk_lens
    prefix_lens = c.prefix_lens if prefix_lens is None else prefix_lens
    B = len(chunk_lens)
    qf = c.q.float()
    kf = (c.k if k is None else k).float()
    vf = (c.v if v is None else v).float()
    out = torch.zeros(T, Hq, D)              # the binding zero-fills
    ninf = torch.tensor(-math.inf)
    zero = torch.zeros(())
    order = sorted(range(B), key=lambda b: int(chunk_lens[b]) != 0,
                   reverse=True)             # empty sequences last
    for b in order:
        n = min(max(int(chunk_lens[b]), 0), min(c.max_chunk, T))
        if mutant == "len0-writes" and n == 0:
            n = min(1, T)
        start = min(max(int(q_starts[b]), 0), T - n)
        if mutant == "row-offset":
            start = min(b * c.max_chunk, T - n)
        P = min(max(int(prefix_lens[b]), 0), S_max)
        kv_len = min(P + n, S_max)
        if mutant == "kv-len-max-chunk":
            kv_len = min(P + c.max_chunk, S_max)
        for qt0 in range(0, n, TILE):
            qn = min(TILE, n - qt0)
            q = qf[start + qt0:start + qt0 + qn].reshape(qn, Hk, G, D)
            qpos = P + torch.arange(qt0, qt0 + qn)[:, None]
            kv_end = min(P + qt0 + TILE, kv_len)
            tiles = list(range(0, kv_end, TILE))
            if mutant == "drop-last-tile":
                tiles = tiles[:-1]
            parts = []
            for split in range(N):
                m = torch.full((Hq, qn), -math.inf)
                s = torch.zeros(Hq, qn)
                acc = torch.zeros(Hq, qn, D)
                mine = [t for t in tiles if (t // TILE) % N == split]
                for kt0 in mine:
                    kn = min(TILE, kv_len - kt0)
                    kp = torch.arange(kt0, kt0 + kn)[None, :]
                    mask = kp <= qpos
                    sc = torch.einsum("qhgd,htd->hgqt", q,
                                      kf[b, :, kt0:kt0 + kn])
                    sc = sc.reshape(Hq, qn, kn) * c.scale
                    sc = torch.where(mask[None], sc, ninf)
                    m_new = torch.maximum(m, sc.amax(dim=2))
                    p = torch.where(mask[None],
                                    torch.exp(sc - m_new[..., None]), zero)
                    corr = torch.where(m == ninf, zero, torch.exp(m - m_new))
                    s = s * corr + p.sum(dim=2)
                    p = p.to(BF16).float()
                    pv = torch.einsum(
                        "hgqt,htd->hgqd", p.reshape(Hk, G, qn, kn),
                        vf[b, :, kt0:kt0 + kn]).reshape(Hq, qn, D)
                    acc = acc * corr[..., None] + pv
                    m = m_new
                if mutant == "empty-split-exp0" and not mine:
                    m, s = torch.zeros(Hq, qn), torch.ones(Hq, qn)
                parts.append((m, s, acc))
            if N == 1:
                m, s, acc = parts[0]
            else:                            # the merge kernel
                m = torch.stack([p[0] for p in parts]).amax(dim=0)
                s = torch.zeros(Hq, qn)
                acc = torch.zeros(Hq, qn, D)
                for m_s, s_s, o_s in parts:
                    f = torch.where(m_s == ninf, zero, torch.exp(m_s - m))
                    if mutant == "merge-unweighted":
                        f = torch.where(m_s == ninf, zero, torch.ones(()))
                    s = s + s_s * f
                    acc = acc + o_s * f[..., None]
            inv = torch.where(s > 0, 1.0 / s, zero)
            out[start + qt0:start + qt0 + qn] = (
                acc * inv[..., None]).permute(1, 0, 2)
    return out.to(BF16)


def ratio(family, lens, hq, hk, dtype, num_splits, mutant=None, poison=None):
    c, ref, absref = rc.cached_ragged(family, rc.PREFIXES, lens, hq, hk,
                                      dtype)
    k = v = None
    if poison:
        k, v = ao.poison_dead_rows(c.k, c.v, c.lens_kv, poison)
    out = emulate_ragged(c, num_splits, mutant, k, v)
    return ao.error_ratio(out, ref, ec.bound(ref, absref))[0]


# --------------------------------------------------------------------------
# the references
# --------------------------------------------------------------------------

def test_ragged_ref64_agrees_with_naive_loop():
    prefixes, lens = (3, 0, 6), (5, 2, 0)
    c, ref, _ = rc.cached_ragged("sentinel", prefixes, lens, 4, 2, BF16)
    assert ref.shape[0] == c.rows == 7
    q, k, v = ao.f64(c.q), ao.f64(c.k), ao.f64(c.v)
    row = 0
    for b, (P, n) in enumerate(zip(prefixes, lens)):
        assert int(c.q_starts[b]) == row
        for i in range(n):
            for h in range(4):
                seen = P + i + 1
                p = torch.softmax(k[b, h // 2, :seen] @ q[row, h] * c.scale,
                                  dim=0)
                torch.testing.assert_close(ref[row, h],
                                           p @ v[b, h // 2, :seen],
                                           atol=1e-12, rtol=1e-12)
            row += 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ec.HEADS)
def test_ops_reference_within_bound(hq, hk, dtype):
    """ops.extend_attn_ragged_ref (fp32) on CPU against the float64 rows,
    with NaN in every dead cache row and in three rows no sequence owns."""
    for family in ec.FAMILIES:
        for lens in rc.PAIRINGS.values():
            c, ref, absref = rc.cached_ragged(family, rc.PREFIXES, lens, hq,
                                              hk, dtype)
            p = rc.ragged_case(family, rc.PREFIXES, lens, hq, hk, dtype,
                               pad_rows=3)
            k, v = ao.poison_dead_rows(c.k, c.v, c.lens_kv, "nan")
            out = ops.extend_attn_ragged_ref(p.q, k, v, c.prefix_lens,
                                             c.chunk_lens, c.max_chunk,
                                             c.scale)
            assert bool((out[c.rows:] == 0).all())
            ao.assert_within(out[:c.rows], ref, ec.bound(ref, absref),
                             f"{family} lens={lens}")


def test_extend_attn_ragged_routes_cpu_tensors_to_the_reference():
    c, ref, absref = rc.cached_ragged("sentinel", rc.PREFIXES, rc.LENS, 8, 2,
                                      BF16)
    out = ops.extend_attn_ragged(c.q, c.k, c.v, c.prefix_lens, c.chunk_lens,
                                 c.max_chunk, c.scale)
    want = ops.extend_attn_ragged_ref(c.q, c.k, c.v, c.prefix_lens,
                                      c.chunk_lens, c.max_chunk, c.scale)
    assert out.dtype == BF16 and torch.equal(out, want.to(BF16))
    ao.assert_within(out, ref, ec.bound(ref, absref), "cpu routing")


# --------------------------------------------------------------------------
# the emulation passes at every GPU shape and split count; its mutants do not
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ec.HEADS)
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_emulation_within_bound(family, hq, hk, dtype):
    worst = 0.0
    for name, lens in rc.PAIRINGS.items():
        for n in rc.SPLITS:
            r = ratio(family, lens, hq, hk, dtype, n, poison="nan")
            assert r <= 1.0, (name, n, r)
            worst = max(worst, r)
    print(f"\n[ragged-cpu] family={family} heads={hq}/{hk} worst={worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_long_prefix(dtype):
    c, ref, absref = rc.cached_ragged("sentinel", rc.LONG_PREFIXES,
                                      rc.LONG_LENS, 8, 2, dtype)
    for n in (1, 18):                        # 18: what the GPU launch picks
        r = ao.error_ratio(emulate_ragged(c, n), ref,
                           ec.bound(ref, absref))[0]
        print(f"\n[ragged-cpu] long prefix splits={n} ratio={r:.3f}")
        assert r <= 1.0, (n, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing", list(rc.PAIRINGS))
@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_rejected(mutant, pairing, dtype):
    """Each mistake this kernel can make, on each pairing of the grid: the
    worst census ratio over the split counts that reach the mistaken code
    is > 4x the bound (a NaN counts as infinite). The dead cache rows hold
    NaN, which is how a live-row count of P_b + max_chunk shows: the rows it
    adds are masked for every query, so only 0 x NaN in the PV product
    tells. The two merge mutants need a merge, so they run split only. The
    census carries the assertion and the sentinel is printed, except for the
    merge without weights: every census score is 0, so all its weights are
    exp(0) and that mutant is the correct merge there; the sentinel's
    running max moves by tens between tiles and carries it instead."""
    splits = {"merge-unweighted": (2, 3, 7),
              "empty-split-exp0": (7,)}.get(mutant, rc.SPLITS)
    lens = rc.PAIRINGS[pairing]
    worst = {f: max(ratio(f, lens, 8, 2, dtype, n, mutant=mutant,
                          poison="nan") for n in splits)
             for f in ec.FAMILIES}
    print(f"\n[ragged-cpu] mutant={mutant} pairing={pairing} worst={worst}")
    family = "sentinel" if mutant == "merge-unweighted" else "census"
    assert worst[family] > 4, (mutant, pairing, worst)


def test_out_of_range_device_values_are_clamped():
    """Lengths, starts and prefixes outside their ranges index nothing out
    of a buffer in the emulation (a slice past the end would change a shape
    and raise) and give what the clamped values give. This is the only
    place such values are exercised; no GPU test launches them."""
    c, _, _ = rc.cached_ragged("sentinel", (3, 0, 6), (5, 2, 0), 4, 2, BF16)
    T, S_max = c.q.shape[0], c.k.shape[2]
    i32 = dict(dtype=torch.int32)
    wild = emulate_ragged(
        c, 2, chunk_lens=torch.tensor([9, -4, 2 ** 30], **i32),
        q_starts=torch.tensor([-7, 2 ** 30, 6], **i32),
        prefix_lens=torch.tensor([-1, 2 ** 30, 6], **i32))
    tame = emulate_ragged(
        c, 2, chunk_lens=torch.tensor([5, 0, 5], **i32),
        q_starts=torch.tensor([0, T, 2], **i32),
        prefix_lens=torch.tensor([0, S_max, 6], **i32))
    assert torch.equal(wild, tame)


# --------------------------------------------------------------------------
# engine (TINY on the CPU; tolerance of test_extend_attn_cpu's engine tests)
# --------------------------------------------------------------------------

TOL = dict(atol=5e-2, rtol=5e-2)


def tiny(seed, max_batch=5, max_seq=32):
    from wva_amd.calibration.model import TINY, LlamaDecodeModel
    return LlamaDecodeModel(TINY, max_batch=max_batch, max_seq=max_seq,
                            device="cpu", seed=seed)


def tokens_of(shape, seed):
    from wva_amd.calibration.model import TINY
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, TINY.vocab_size, shape, generator=g)


class TestRaggedEngine:
    def test_equal_lengths_equal_mixed_step(self):
        Bd, Bp, C, ctx = 2, 2, 5, 6
        prompt = tokens_of((Bd + Bp, ctx), 3)
        dec = tokens_of((Bd,), 4)
        chunk = tokens_of((Bp, C), 5)
        ragged, mixed = tiny(9), tiny(9)
        for m in (ragged, mixed):
            m.prefill(prompt)
            m.context_lens[Bd] = ctx - 2        # unequal prefixes
        want = mixed.mixed_step(dec, chunk)
        got = ragged.ragged_step(dec, chunk.reshape(-1),
                                 torch.full((Bp,), C, dtype=torch.int32), C)
        assert torch.equal(got, want)
        assert torch.equal(ragged.context_lens, mixed.context_lens)
        assert torch.equal(ragged.k_cache[1], mixed.k_cache[1])
        assert torch.equal(ragged.v_cache[1], mixed.v_cache[1])

    def test_unequal_lengths_equal_separate_prefill_chunks(self):
        """Chunks of 9, 4 and 0 tokens behind one decode row: each sequence
        matches a prefill_chunk of its own on a twin model, and the
        zero-length sequence keeps its context_lens and cache rows."""
        Bd, lens, ctx = 1, (9, 4, 0), 6
        prompt = tokens_of((Bd + 3, ctx), 3)
        dec = tokens_of((Bd,), 4)
        chunks = [tokens_of((1, n), 10 + n) for n in lens]
        m = tiny(9)
        m.prefill(prompt)
        before = [c.clone() for c in m.k_cache + m.v_cache]
        got = m.ragged_step(dec, torch.cat([c[0] for c in chunks]),
                            torch.tensor(lens, dtype=torch.int32), max(lens))
        assert got.shape[0] == Bd + 3
        assert m.context_lens[:4].tolist() == [ctx + 1, ctx + 9, ctx + 4, ctx]
        for cache, old in zip(m.k_cache + m.v_cache, before):
            assert torch.equal(cache[Bd + 2], old[Bd + 2])
        ref = tiny(9)
        ref.prefill(prompt)
        want_dec = ref.decode_step(dec)
        torch.testing.assert_close(got[:Bd].float(), want_dec.float(), **TOL)
        for b, n in enumerate(lens):
            if n == 0:
                continue
            solo = tiny(9)
            solo.prefill(prompt[Bd + b:Bd + b + 1])
            want = solo.prefill_chunk(chunks[b])
            torch.testing.assert_close(got[Bd + b:Bd + b + 1].float(),
                                       want.float(), **TOL)
            torch.testing.assert_close(
                m.k_cache[0][Bd + b, :, :ctx + n].float(),
                solo.k_cache[0][0, :, :ctx + n].float(), **TOL)

    def test_rows_past_the_packed_chunks_write_nothing(self):
        """T > sum(chunk_lens): same logits, caches and context_lens as the
        exactly packed call."""
        lens, ctx = (3, 5), 6
        prompt = tokens_of((2, ctx), 3)
        packed = tokens_of((sum(lens),), 8)
        c_lens = torch.tensor(lens, dtype=torch.int32)
        a, b = tiny(9), tiny(9)
        for m in (a, b):
            m.prefill(prompt)
        want = a.ragged_step(None, packed, c_lens, 5)
        got = b.ragged_step(None, torch.cat([packed, tokens_of((4,), 2)]),
                            c_lens, 5)
        assert torch.equal(got, want)
        assert torch.equal(a.context_lens, b.context_lens)
        assert torch.equal(a.k_cache[0], b.k_cache[0])
        assert torch.equal(a.v_cache[1], b.v_cache[1])
