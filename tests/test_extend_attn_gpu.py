"""GPU tests of chunked-prefill ("extend") attention, the HAS_PREFIX
instantiation of the flash-prefill kernel, and of the engine paths built on
it (prefill_chunk, prefill(chunk_size=), mixed_step).

The cases, the float64 reference and the shape grid are extend_cases.py;
the bound is attn_oracle.attn_bound(p_bf16=True), derived there.
test_extend_attn_cpu.py shows on the CPU that these cases and that bound
reject a kernel that forgets the prefix in the mask or the sweep end, rounds
it down to a tile, or masks strictly. Each test prints its worst err/bound
ratio (`-s` shows them; docs/testing.md records them).
"""
import pytest
import torch

import attn_oracle as ao
import extend_cases as ec
from attn_oracle import BF16, FP8
from wva_amd import ops

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(family, dtype, ratio, note=""):
    name = "fp8" if dtype == FP8 else "bf16"
    print(f"\n[extend] family={family} dtype={name} ratio={ratio:.3f} {note}")


def extend(c, dev, k=None, v=None):
    k = c.k if k is None else k
    v = c.v if v is None else v
    return ops.extend_attn(c.q.to(dev), k.to(dev), v.to(dev),
                           c.prefix_lens.to(dev), c.chunk, c.scale).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ec.HEADS)
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_shape_grid(dev, family, hq, hk, dtype):
    """Census (query i counts the positions <= P_b + i per residue) and
    sentinel (own key is the newest; rows past S never show) on every
    prefix pair x chunk length of the grid."""
    worst = 0.0
    for pair in ec.PREFIX_PAIRS:
        for chunk in ec.CHUNKS:
            c, ref, absref = ec.cached_extend(family, pair, chunk, hq, hk,
                                              dtype)
            r = ao.assert_within(extend(c, dev), ref, ec.bound(ref, absref),
                                 f"{family} P={pair} C={chunk}")
            worst = max(worst, r)
    record(family, dtype, worst, f"{hq}/{hk} worst over the grid")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pair,chunk,exact", [
    ((63, 65), 17, False), ((200, 128), 65, False), ((130, 7), 130, False),
    ((1, 64), 64, True), ((200, 128), 1, True),
])
def test_dead_rows_are_never_read(dev, pair, chunk, exact, dtype):
    """Rows >= P_b + C hold NaN, the largest finite value or zero: the three
    outputs are bit-equal, finite and within bound. With `exact` the caches
    are sliced to S rows, so max(P) + C == S_max."""
    c, ref, absref = ec.cached_extend("sentinel", pair, chunk, 8, 2, dtype)
    k, v = c.k, c.v
    if exact:
        S = max(pair) + chunk
        k, v = k[:, :, :S].contiguous(), v[:, :, :S].contiguous()
        assert k.shape[2] == max(c.lens)
    outs = {}
    for kind in ("zero", "nan", "max"):
        kp, vp = ao.poison_dead_rows(k, v, c.lens, kind)
        outs[kind] = extend(c, dev, kp, vp)
    assert bool(torch.isfinite(outs["nan"].float()).all())
    assert torch.equal(outs["zero"], outs["nan"])
    assert torch.equal(outs["zero"], outs["max"])
    r = ao.assert_within(outs["zero"], ref, ec.bound(ref, absref),
                         f"poison P={pair} C={chunk}")
    record("poison", dtype, r, f"P={pair} C={chunk} exact={exact}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", ao.PREFILL_S)
def test_prefix_zero_is_the_one_shot_kernel(dev, S, dtype):
    """Zero prefixes and C = S: the same tiles, masks and floating-point
    sequence as prefill_attn, so the same bits."""
    c = ao.prefill_sentinel_case(2, 8, 2, S, dtype, seed=S)
    q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
    zeros = torch.zeros(2, dtype=torch.int32, device=dev)
    one = ops.prefill_attn(q, k, v, 2, S, c.scale)
    ext = ops.extend_attn(q, k, v, zeros, S, c.scale)
    assert torch.equal(one, ext), (
        f"max |diff| = {float((one.float() - ext.float()).abs().max()):g}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_compose_to_the_whole_prompt(dev, dtype):
    """[0,64) [64,128) [128,200) one after another against a cache filled to
    200 rows (the later rows are live data that an earlier chunk must not
    see). Concatenated: within bound of prefill_ref64 at S = 200."""
    S, B, Hq = 200, 2, 8
    c = ao.prefill_sentinel_case(B, Hq, 2, S, dtype, seed=S)
    ref, absref = ao.prefill_ref64(c.q, c.k, c.v, B, S, c.scale)
    q = c.q.reshape(B, S, Hq, ao.D)
    k, v = c.k.to(dev), c.v.to(dev)
    parts = []
    for lo, hi in ((0, 64), (64, 128), (128, 200)):
        qc = q[:, lo:hi].reshape(B * (hi - lo), Hq, ao.D).contiguous()
        P = torch.full((B,), lo, dtype=torch.int32, device=dev)
        out = ops.extend_attn(qc.to(dev), k, v, P, hi - lo, c.scale)
        parts.append(out.reshape(B, hi - lo, Hq, ao.D))
    out = torch.cat(parts, dim=1).reshape(B * S, Hq, ao.D).cpu()
    r = ao.assert_within(out, ref, ao.attn_bound(ref, absref, True),
                         "composition S=200")
    one = ops.prefill_attn(c.q.to(dev), k, v, B, S, c.scale).cpu()
    record("composition", dtype, r,
           f"bit-equal to prefill_attn: {torch.equal(out, one)}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_prefix(dev, dtype):
    c, ref, absref = ec.cached_extend("sentinel", ec.LONG_PREFIX,
                                      ec.LONG_CHUNK, 8, 2, dtype)
    r = ao.assert_within(extend(c, dev), ref, ec.bound(ref, absref),
                         f"long prefix P={ec.LONG_PREFIX}")
    record("long-prefix", dtype, r, f"P={ec.LONG_PREFIX} C={ec.LONG_CHUNK}")


def test_binding_checks_prefix_lens(dev):
    c = ec.extend_case("sentinel", (1, 64), 17, 8, 2, BF16)
    ext = ops._require_ext()
    q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
    P = c.prefix_lens.to(dev)
    with pytest.raises(RuntimeError, match="int32"):
        ext.extend_attn(q, k, v, P.long(), 17, c.scale)
    with pytest.raises(RuntimeError, match="prefix_lens"):
        ext.extend_attn(q, k, v, P[:1], 17, c.scale)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.extend_attn(q, k, v, c.prefix_lens, 17, c.scale)
    with pytest.raises(RuntimeError, match="multiple of chunk"):
        ext.extend_attn(q, k, v, P, 16, c.scale)


# --------------------------------------------------------------------------
# engine (TINY; tolerance of test_ops_gpu.TestPrefillGpu)
# --------------------------------------------------------------------------

TOL = dict(atol=8e-2, rtol=8e-2)


def tiny(seed=21, max_batch=3, max_seq=64, **kw):
    from wva_amd.calibration.model import TINY, LlamaDecodeModel
    return LlamaDecodeModel(TINY, max_batch=max_batch, max_seq=max_seq,
                            seed=seed, **kw)


def tokens_of(shape, seed, dev):
    from wva_amd.calibration.model import TINY
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, TINY.vocab_size, shape, generator=g).to(dev)


class TestChunkedEngineGpu:
    def test_chunked_prefill_matches_one_shot(self, dev):
        m1, m2 = tiny(), tiny()
        S = 37
        tokens = tokens_of((2, S), 1, dev)
        one = m1.prefill(tokens)
        chunked = m2.prefill(tokens, chunk_size=16)     # 16 + 16 + 5
        torch.testing.assert_close(chunked.float(), one.float(), **TOL)
        assert torch.equal(m1.context_lens, m2.context_lens)
        torch.testing.assert_close(m2.k_cache[0][:2, :, :S].float(),
                                   m1.k_cache[0][:2, :, :S].float(), **TOL)

    def test_mixed_step_equals_separate_calls(self, dev):
        """Rows 0-1 decode at different lengths, row 2 prefills a chunk."""
        Bd, C, ctx = 2, 9, 11
        prompt = tokens_of((3, ctx), 3, dev)
        dec = tokens_of((Bd,), 4, dev)
        chunk = tokens_of((1, C), 5, dev)
        mixed, m_dec, solo = tiny(), tiny(), tiny()
        for m in (mixed, m_dec):
            m.prefill(prompt)
            m.decode_step(prompt[:1, 0])                # row 0 is one ahead
        solo.prefill(prompt[2:3])
        got = mixed.mixed_step(dec, chunk)
        want_dec = m_dec.decode_step(dec)
        want_chunk = solo.prefill_chunk(chunk)
        torch.testing.assert_close(got[:Bd].float(), want_dec.float(), **TOL)
        torch.testing.assert_close(got[Bd:].float(), want_chunk.float(),
                                   **TOL)
        assert mixed.context_lens.tolist() == [ctx + 2, ctx + 1, ctx + C]

    def test_fp8_kv_chunked_prefill_then_decode(self, dev):
        m = tiny(kv_dtype="fp8")
        ref = tiny(kv_dtype="fp8")
        tokens = tokens_of((2, 21), 6, dev)
        chunked = m.prefill(tokens, chunk_size=8)
        one = ref.prefill(tokens)
        torch.testing.assert_close(chunked.float(), one.float(), **TOL)
        logits = m.decode_step(tokens_of((2,), 7, dev))
        assert m.context_lens[:2].tolist() == [22, 22]
        assert bool(torch.isfinite(logits.float()).all())

    def test_measurements_return_positive_numbers(self, dev):
        from wva_amd.calibration.itl_benchmark import (
            measure_chunked_prefill_tps, measure_mixed_itl)

        m = tiny(max_batch=3, max_seq=64)
        assert measure_chunked_prefill_tps(m, batch=2, seq=48, chunk=16,
                                           iters=2) > 0
        assert measure_mixed_itl(m, decode_batch=2, context_len=16, chunk=16,
                                 iters=2, warmup=1) > 0
        assert measure_mixed_itl(m, decode_batch=2, context_len=16, chunk=0,
                                 iters=2, warmup=1) > 0
