"""CPU side of the chunked-prefill ("extend") attention tests.

A float32 tile-by-tile emulation of the kernel's algorithm (64-key tiles
aligned at 0, one sweep per 64-row q-tile that ends at min(P + qt0 + 64,
P + C), P rounded to bf16 for the PV product) stays within the derived bound
on the whole shape grid of extend_cases.py, and four mutants of it (mask or
sweep end without the prefix, sweep end with the prefix rounded down to a
tile, strict mask) are far outside it, so test_extend_attn_gpu.py can see
those mistakes in the HIP kernel. Also: ops.extend_attn_ref against the
float64 reference, and the engine's prefill_chunk / prefill(chunk_size=) /
mixed_step on the tiny config.
"""
import math

import pytest
import torch

import attn_oracle as ao
import extend_cases as ec
from attn_oracle import BF16, FP8, TILE
from wva_amd import ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
NONZERO_PAIRS = [p for p in ec.PREFIX_PAIRS if any(p)]
PREFIX_MUTANTS = ("mask-no-prefix", "end-no-prefix", "end-prefix-floor")


def emulate_extend(c, mutant=None):
    """Float32 emulation of prefill_attn_kernel<*, HAS_PREFIX>."""
    B, C = c.batch, c.chunk
    T, Hq, D = c.q.shape
    Hk = c.k.shape[1]
    G = Hq // Hk
    q = c.q.float().reshape(B, C, Hk, G, D)
    k, v = c.k.float(), c.v.float()
    out = torch.zeros(B, C, Hq, D)
    ninf = torch.tensor(-math.inf)
    for b in range(B):
        P = int(c.prefix_lens[b])
        kv_len = P + C
        for qt0 in range(0, C, TILE):
            qn = min(TILE, C - qt0)
            qi = torch.arange(qt0, qt0 + qn)[:, None]       # chunk row
            qpos = qi if mutant == "mask-no-prefix" else P + qi
            start = {"end-no-prefix": 0,
                     "end-prefix-floor": P // TILE * TILE}.get(mutant, P)
            kv_end = min(start + qt0 + TILE, kv_len)
            m = torch.full((Hq, qn), -math.inf)
            s = torch.zeros(Hq, qn)
            acc = torch.zeros(Hq, qn, D)
            for kt0 in range(0, kv_end, TILE):
                kn = min(TILE, kv_len - kt0)
                kp = torch.arange(kt0, kt0 + kn)[None, :]
                mask = kp < qpos if mutant == "causal<" else kp <= qpos
                sc = torch.einsum("qhgd,htd->hgqt", q[b, qt0:qt0 + qn],
                                  k[b, :, kt0:kt0 + kn])
                sc = sc.reshape(Hq, qn, kn) * c.scale
                sc = torch.where(mask[None], sc, ninf)
                m_new = torch.maximum(m, sc.amax(dim=2))
                p = torch.where(mask[None], torch.exp(sc - m_new[..., None]),
                                torch.zeros(()))
                corr = torch.where(m == ninf, torch.zeros(()),
                                   torch.exp(m - m_new))
                s = s * corr + p.sum(dim=2)
                p = p.to(BF16).float()
                pv = torch.einsum("hgqt,htd->hgqd", p.reshape(Hk, G, qn, kn),
                                  v[b, :, kt0:kt0 + kn]).reshape(Hq, qn, D)
                acc = acc * corr[..., None] + pv
                m = m_new
            inv = torch.where(s > 0, 1.0 / s, torch.zeros(()))
            out[b, qt0:qt0 + qn] = (acc * inv[..., None]).permute(1, 0, 2)
    return out.reshape(T, Hq, D).to(BF16)


def ratio(family, pair, chunk, hq, hk, dtype, **kw):
    c, ref, absref = ec.cached_extend(family, pair, chunk, hq, hk, dtype)
    out = emulate_extend(c, **kw)
    return ao.error_ratio(out, ref, ec.bound(ref, absref))[0]


# --------------------------------------------------------------------------
# the reference itself
# --------------------------------------------------------------------------

def test_extend_ref64_agrees_with_naive_loop():
    c = ec.extend_case("sentinel", (3, 0), 5, 4, 2, BF16, seed=2)
    ref, _ = ec.extend_ref64(c.q, c.k, c.v, c.prefix_lens, c.chunk, c.scale)
    q, k, v = ao.f64(c.q), ao.f64(c.k), ao.f64(c.v)
    for b, P in enumerate((3, 0)):
        for i in range(5):
            for h in range(4):
                n = P + i + 1
                p = torch.softmax(k[b, h // 2, :n] @ q[b * 5 + i, h] * c.scale,
                                  dim=0)
                torch.testing.assert_close(ref[b * 5 + i, h],
                                           p @ v[b, h // 2, :n],
                                           atol=1e-12, rtol=1e-12)


def test_extend_ref64_at_prefix_zero_is_prefill_ref64():
    c = ec.extend_case("sentinel", (0, 0), 65, 8, 2, BF16)
    a = ec.extend_ref64(c.q, c.k, c.v, c.prefix_lens, c.chunk, c.scale)
    b = ao.prefill_ref64(c.q, c.k, c.v, 2, 65, c.scale)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_extend_ref64_never_reads_dead_rows(dtype):
    c = ec.extend_case("sentinel", (63, 65), 17, 8, 2, dtype)
    kp, vp = ao.poison_dead_rows(c.k, c.v, c.lens, "nan")
    a = ec.extend_ref64(c.q, c.k, c.v, c.prefix_lens, c.chunk, c.scale)
    b = ec.extend_ref64(c.q, kp, vp, c.prefix_lens, c.chunk, c.scale)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------------------------------------------
# the emulation passes at every GPU shape; its mutants do not
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ec.HEADS)
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_emulation_within_bound(family, hq, hk, dtype):
    worst = 0.0
    for pair in ec.PREFIX_PAIRS:
        for chunk in ec.CHUNKS:
            r = ratio(family, pair, chunk, hq, hk, dtype)
            assert r <= 1.0, (pair, chunk, r)
            worst = max(worst, r)
    print(f"\n[extend-cpu] family={family} heads={hq}/{hk} worst={worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", NONZERO_PAIRS)
@pytest.mark.parametrize("mutant", PREFIX_MUTANTS)
def test_prefix_mutants_rejected(mutant, pair, dtype):
    """A kernel that forgets the prefix in the mask or in the sweep end, or
    rounds it down to a tile there, is rejected on every pair that has a
    nonzero prefix (at prefix (0, 0) these mutants are the correct kernel).
    A given mutant coincides with the correct kernel at some chunk lengths
    of a pair (with C = 1 and P < 64 every sweep is the one tile 0), so the
    claim is per pair: its worst chunk is > 4x the bound. The census alone
    carries the assertion. The peaked sentinel is printed: where a mutant
    drops a single key (the rounded-down sweep end at P = 1 loses only row
    63's own key) that key may carry too little weight to show."""
    worst = {f: max(ratio(f, pair, chunk, 8, 2, dtype, mutant=mutant)
                    for chunk in ec.CHUNKS) for f in ec.FAMILIES}
    print(f"\n[extend-cpu] mutant={mutant} pair={pair} worst={worst}")
    assert worst["census"] > 4, (mutant, pair, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair", NONZERO_PAIRS)
def test_strict_mask_rejected(pair, dtype):
    """kp < P + i drops every row's own key: caught by every census case;
    the peaked sentinel may miss it where that key carries almost no weight,
    which is why both families run."""
    missed = []
    for chunk in ec.CHUNKS:
        assert ratio("census", pair, chunk, 8, 2, dtype, mutant="causal<") > 4
        if ratio("sentinel", pair, chunk, 8, 2, dtype, mutant="causal<") <= 4:
            missed.append(chunk)
    print(f"\n[extend-cpu] strict mask, sentinel misses at {pair}: {missed}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ec.HEADS)
def test_ops_reference_within_bound(hq, hk, dtype):
    """ops.extend_attn_ref (fp32) on CPU against extend_ref64."""
    for family in ec.FAMILIES:
        for pair in ec.PREFIX_PAIRS:
            for chunk in ec.CHUNKS:
                c, ref, absref = ec.cached_extend(family, pair, chunk, hq, hk,
                                                  dtype)
                out = ops.extend_attn_ref(c.q, c.k, c.v, c.prefix_lens,
                                          c.chunk, c.scale)
                ao.assert_within(out, ref, ec.bound(ref, absref),
                                 f"{family} {pair} C={chunk}")


def test_extend_attn_routes_cpu_tensors_to_the_reference():
    c = ec.extend_case("sentinel", (1, 64), 17, 8, 2, BF16)
    out = ops.extend_attn(c.q, c.k, c.v, c.prefix_lens, c.chunk, c.scale)
    want = ops.extend_attn_ref(c.q, c.k, c.v, c.prefix_lens, c.chunk, c.scale)
    assert out.dtype == BF16 and torch.equal(out, want.to(BF16))


# --------------------------------------------------------------------------
# engine (TINY on the CPU; tolerance of test_ops_cpu.TestPrefill)
# --------------------------------------------------------------------------

TOL = dict(atol=5e-2, rtol=5e-2)


def tiny(seed, max_batch=2, max_seq=32):
    from wva_amd.calibration.model import TINY, LlamaDecodeModel
    return LlamaDecodeModel(TINY, max_batch=max_batch, max_seq=max_seq,
                            device="cpu", seed=seed)


def tokens_of(shape, seed):
    from wva_amd.calibration.model import TINY
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, TINY.vocab_size, shape, generator=g)


class TestChunkedEngine:
    def test_chunked_prefill_matches_one_shot(self):
        m1, m2 = tiny(9), tiny(9)
        S = 13
        tokens = tokens_of((2, S), 1)
        one = m1.prefill(tokens)
        chunked = m2.prefill(tokens, chunk_size=4)      # 4 + 4 + 4 + 1
        torch.testing.assert_close(chunked.float(), one.float(), **TOL)
        assert torch.equal(m1.context_lens, m2.context_lens)
        for cache in ("k_cache", "v_cache"):
            torch.testing.assert_close(
                getattr(m2, cache)[0][:2, :, :S].float(),
                getattr(m1, cache)[0][:2, :, :S].float(), **TOL)

    def test_chunk_size_none_is_the_one_shot_path(self):
        m1, m2 = tiny(9), tiny(9)
        tokens = tokens_of((2, 10), 2)
        a = m1.prefill(tokens)
        b = m2.prefill(tokens, chunk_size=None)
        assert torch.equal(a, b)
        assert torch.equal(m1.k_cache[1], m2.k_cache[1])
        assert torch.equal(m1.context_lens, m2.context_lens)

    def test_prefill_chunk_continues_unequal_prefixes(self):
        """Sequences 0 and 1 hold 5 and 9 tokens; one prefill_chunk call
        then extends both by 4. Each must match a one-shot prefill of its
        own concatenation."""
        lens, C = (5, 9), 4
        prompts = [tokens_of((1, n + C), 10 + n) for n in lens]
        m = tiny(9)
        # fill the two prefixes one sequence at a time: cache row 1 through
        # a batch whose row 0 is scratch, then row 0 itself
        m.prefill(torch.cat([prompts[1][:, :lens[1]]] * 2))
        m.prefill(prompts[0][:, :lens[0]])
        m.context_lens[0], m.context_lens[1] = lens
        chunk = torch.cat([p[:, n:] for p, n in zip(prompts, lens)])
        got = m.prefill_chunk(chunk)
        assert m.context_lens[:2].tolist() == [n + C for n in lens]
        for b, n in enumerate(lens):
            ref = tiny(9)
            want = ref.prefill(prompts[b])
            torch.testing.assert_close(got[b:b + 1].float(), want.float(),
                                       **TOL)
            torch.testing.assert_close(
                m.k_cache[0][b, :, :n + C].float(),
                ref.k_cache[0][0, :, :n + C].float(), **TOL)

    def test_mixed_step_equals_separate_calls(self):
        """Rows 0-1 decode, row 2 prefills a chunk, against decode_step on
        the decode rows plus prefill_chunk on the chunk row of twin
        models."""
        Bd, C, ctx = 2, 5, 6
        prompt = tokens_of((3, ctx), 3)
        dec = tokens_of((Bd,), 4)
        chunk = tokens_of((1, C), 5)
        mixed, m_dec = tiny(9, max_batch=3), tiny(9, max_batch=3)
        for m in (mixed, m_dec):
            m.prefill(prompt)
        got = mixed.mixed_step(dec, chunk)
        want_dec = m_dec.decode_step(dec)
        # the chunk row alone, as sequence 0 of a model holding row 2's KV
        solo = tiny(9, max_batch=3)
        solo.prefill(prompt[2:3])
        want_chunk = solo.prefill_chunk(chunk)
        assert got.shape == (Bd + 1, want_dec.shape[1])
        torch.testing.assert_close(got[:Bd].float(), want_dec.float(), **TOL)
        torch.testing.assert_close(got[Bd:].float(), want_chunk.float(),
                                   **TOL)
        assert mixed.context_lens.tolist() == [ctx + 1, ctx + 1, ctx + C]
        torch.testing.assert_close(
            mixed.k_cache[0][2, :, :ctx + C].float(),
            solo.k_cache[0][0, :, :ctx + C].float(), **TOL)
        torch.testing.assert_close(
            mixed.k_cache[0][:Bd, :, :ctx + 1].float(),
            m_dec.k_cache[0][:Bd, :, :ctx + 1].float(), **TOL)

    def test_fp8_kv_chunked_prefill_then_decode(self):
        from wva_amd.calibration.model import TINY, LlamaDecodeModel
        m = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                             seed=9, kv_dtype="fp8")
        m.prefill(tokens_of((2, 11), 6), chunk_size=4)
        logits = m.decode_step(tokens_of((2,), 7))
        assert m.context_lens.tolist() == [12, 12]
        assert bool(torch.isfinite(logits.float()).all())
