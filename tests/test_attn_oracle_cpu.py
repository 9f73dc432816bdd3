"""CPU proof that the attention oracle (attn_oracle.py) has teeth.

A float32 emulation of the kernels' algorithm - 64-position tiles, online
softmax, optional bf16 P, interleaved split-KV plus merge - must stay inside
`attn_bound` on every case family at every shape the GPU tests use, and each
mutant of it (a dropped newest row, a dead row read, a lost split, ...) must
be rejected by the family named in its test.
"""
import math

import pytest
import torch

import attn_oracle as ao
from attn_oracle import BF16, FP8, TILE
from wva_amd import ops

DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
P_MODES = [pytest.param(False, id="v4"), pytest.param(True, id="v5")]


# --------------------------------------------------------------------------
# float32 emulation of the kernels, with mutants
# --------------------------------------------------------------------------

def emulate_decode(c, p_bf16, num_splits, mutant=None, quantize_q=True):
    Hk, S = c.k.shape[1], c.k.shape[2]
    B, Hq, D = c.q.shape
    G = Hq // Hk
    q = (ao.quantize_q_fp8(c.q, Hk) if c.fp8 and quantize_q
         else c.q.float()).reshape(B, Hk, G, D)
    k, v = c.k.float(), c.v.float()
    out = torch.zeros(B, Hq, D)
    ninf = torch.tensor(-math.inf)
    for b in range(B):
        ctx = int(c.lens[b])
        if mutant == "lens-1":
            ctx = max(ctx - 1, 0)
        elif mutant == "lens+1":
            ctx = min(ctx + 1, S)
        dup_t0 = (ctx // 2) // TILE * TILE if mutant == "dup_tile" else -1
        parts = []
        for sp in range(num_splits):
            m = torch.full((Hq,), -math.inf)
            s = torch.zeros(Hq)
            acc = torch.zeros(Hq, D)
            tiles = []
            for t0 in range(sp * TILE, ctx, num_splits * TILE):
                tiles += [t0, t0] if t0 == dup_t0 else [t0]
            for t0 in tiles:
                tn = min(TILE, ctx - t0)
                sc = torch.einsum("hgd,htd->hgt", q[b], k[b, :, t0:t0 + tn])
                sc = sc.reshape(Hq, tn) * c.scale
                m_new = torch.maximum(m, sc.amax(dim=1))
                p = torch.exp(sc - m_new[:, None])
                corr = torch.where(m == ninf, torch.zeros(()),
                                   torch.exp(m - m_new))
                s = s * corr + p.sum(dim=1)
                if mutant != "no_rescale":
                    acc = acc * corr[:, None]
                if p_bf16:
                    p = p.to(BF16).float()
                acc = acc + torch.einsum(
                    "hgt,htd->hgd", p.reshape(Hk, G, tn),
                    v[b, :, t0:t0 + tn]).reshape(Hq, D)
                m = m_new
            parts.append((m, s, acc))
        if mutant == "skip_split":
            del parts[min(1, num_splits - 1)]
        M = torch.stack([p[0] for p in parts]).amax(dim=0)
        S_sum = torch.zeros(Hq)
        o = torch.zeros(Hq, D)
        for m, s, acc in parts:
            f = torch.where(m == ninf, torch.zeros(()), torch.exp(m - M))
            if mutant == "no_merge_weights":
                f = (m != ninf).float()
            S_sum = S_sum + s * f
            o = o + acc * f[:, None]
        inv = torch.where(S_sum > 0, 1.0 / S_sum, torch.zeros(()))
        out[b] = o * inv[:, None]
    return out.to(BF16)


def emulate_prefill(c, mutant=None):
    B, S = c.batch, c.seq
    T, Hq, D = c.q.shape
    Hk = c.k.shape[1]
    G = Hq // Hk
    q = c.q.float().reshape(B, S, Hk, G, D)
    k, v = c.k.float(), c.v.float()
    out = torch.zeros(B, S, Hq, D)
    qr = torch.arange(S)[:, None]
    ninf = torch.tensor(-math.inf)
    for b in range(B):
        m = torch.full((Hq, S), -math.inf)
        s = torch.zeros(Hq, S)
        acc = torch.zeros(Hq, S, D)
        for kt0 in range(0, S, TILE):
            kn = min(TILE, S - kt0)
            kp = torch.arange(kt0, kt0 + kn)[None, :]
            mask = kp < qr if mutant == "causal<" else kp <= qr
            sc = torch.einsum("qhgd,htd->hgqt", q[b], k[b, :, kt0:kt0 + kn])
            sc = sc.reshape(Hq, S, kn) * c.scale
            sc = torch.where(mask[None], sc, ninf)
            m_new = torch.maximum(m, sc.amax(dim=2))
            p = torch.where(mask[None], torch.exp(sc - m_new[..., None]),
                            torch.zeros(()))
            corr = torch.where(m == ninf, torch.zeros(()),
                               torch.exp(m - m_new))
            s = s * corr + p.sum(dim=2)
            p = p.to(BF16).float()
            pv = torch.einsum("hgqt,htd->hgqd", p.reshape(Hk, G, S, kn),
                              v[b, :, kt0:kt0 + kn]).reshape(Hq, S, D)
            acc = acc * corr[..., None] + pv
            m = m_new
        inv = torch.where(s > 0, 1.0 / s, torch.zeros(()))
        out[b] = (acc * inv[..., None]).permute(1, 0, 2)
    return out.reshape(T, Hq, D).to(BF16)


def decode_ratio(c, p_bf16, num_splits, ref=None, **kw):
    if ref is None:
        ref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale, q_fp8=c.fp8)
    out = emulate_decode(c, p_bf16, num_splits, **kw)
    return ao.error_ratio(out, ref[0], ao.attn_bound(*ref, p_bf16))[0]


def prefill_ratio(c, **kw):
    ref = ao.prefill_ref64(c.q, c.k, c.v, c.batch, c.seq, c.scale)
    out = emulate_prefill(c, **kw)
    return ao.error_ratio(out, ref[0], ao.attn_bound(*ref, True))[0]


# --------------------------------------------------------------------------
# the unmutated emulation passes every family at every GPU shape
# --------------------------------------------------------------------------

@pytest.mark.parametrize("p_bf16", P_MODES)
@pytest.mark.parametrize("dtype", DTYPES)
class TestEmulationWithinBound:
    @pytest.mark.parametrize("gain", ao.GAINS)
    @pytest.mark.parametrize("G", ao.EDGE_GROUPS)
    def test_sentinel_tile_edges(self, G, gain, dtype, p_bf16):
        c, *ref = ao.cached_ref(ao.edge_case, G, dtype, gain)
        for splits in (1, ao.EDGE_SPLITS):
            assert decode_ratio(c, p_bf16, splits, ref) <= 1.0

    @pytest.mark.parametrize("gain", ao.GAINS)
    @pytest.mark.parametrize("S", list(ao.SPLIT_GRID))
    def test_sentinel_split_grid(self, S, gain, dtype, p_bf16):
        c, *ref = ao.cached_ref(ao.grid_case, S, dtype, gain)
        assert decode_ratio(c, p_bf16, ao.SPLIT_GRID[S], ref) <= 1.0

    @pytest.mark.parametrize("ctx", ao.CENSUS_CTX)
    def test_census(self, ctx, dtype, p_bf16):
        c = ao.census_case(ctx, ao.census_rows(ctx), 4, dtype)
        for splits in (1, ao.CENSUS_SPLITS[ctx]):
            assert decode_ratio(c, p_bf16, splits) <= 1.0

    @pytest.mark.parametrize("S", (64, 2048))
    def test_empty_and_poison_cases(self, S, dtype, p_bf16):
        for fn in (ao.empty_case, ao.poison_case):
            c, *ref = ao.cached_ref(fn, S, dtype)
            assert decode_ratio(c, p_bf16, ao.SPLIT_GRID[S], ref) <= 1.0


@pytest.mark.parametrize("p_bf16", P_MODES)
@pytest.mark.parametrize("direction", ao.RAMP_DIRECTIONS)
def test_emulation_within_bound_ramp(direction, p_bf16):
    for S, splits in [(ao.RAMP_UNSPLIT_S, 1), *ao.RAMP_SPLITS.items()]:
        c = ao.ramp_case(direction, S, peak_pos=ao.ramp_peak_pos(splits))
        assert decode_ratio(c, p_bf16, splits) <= 1.0, (S, splits)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ao.PREFILL_HEADS)
def test_emulation_within_bound_prefill(hq, hk, dtype):
    for S in ao.PREFILL_S:
        for c in (ao.prefill_census_case(2, hq, hk, S, dtype),
                  ao.prefill_sentinel_case(2, hq, hk, S, dtype, seed=S)):
            assert prefill_ratio(c) <= 1.0, S


def test_split_literals_match_heuristic_mirror():
    for S, n in ao.SPLIT_GRID.items():
        assert ao.heuristic_splits(1, S) == n
        assert ao.heuristic_splits(4, S) == n
    assert ao.heuristic_splits(len(ao.EDGE_LENS), ao.EDGE_S) == ao.EDGE_SPLITS
    for ctx, n in ao.CENSUS_SPLITS.items():
        assert ao.heuristic_splits(1, ao.census_rows(ctx)) == n
    for S, n in ao.RAMP_SPLITS.items():
        assert ao.heuristic_splits(1, S) == n
    for S in (ao.EDGE_S, ao.RAMP_UNSPLIT_S, 2048, ao.census_rows(2000)):
        assert ao.heuristic_splits(ao.UNSPLIT_REPLICAS, S) == 1


# --------------------------------------------------------------------------
# every mutant is rejected, by the family its test names
# --------------------------------------------------------------------------

@pytest.mark.parametrize("p_bf16", P_MODES)
class TestMutantsRejected:
    @pytest.mark.parametrize("dtype", DTYPES)
    @pytest.mark.parametrize("gain", ao.GAINS)
    def test_newest_row_dropped_caught_by_sentinel(self, gain, dtype, p_bf16):
        """lens-1: dim 1 of every row loses its only contribution."""
        c, *ref = ao.cached_ref(ao.grid_case, 2048, dtype, gain)
        assert decode_ratio(c, p_bf16, 16, ref, mutant="lens-1") > 50
        c, *ref = ao.cached_ref(ao.edge_case, 4, dtype, gain)
        assert decode_ratio(c, p_bf16, 1, ref, mutant="lens-1") > 50

    @pytest.mark.parametrize("dtype", DTYPES)
    @pytest.mark.parametrize("gain", ao.GAINS)
    def test_dead_row_read_caught_by_sentinel(self, gain, dtype, p_bf16):
        """lens+1: dim 2, whose bound is exactly 0, lights up."""
        c, *ref = ao.cached_ref(ao.edge_case, 4, dtype, gain)
        for splits in (1, ao.EDGE_SPLITS):
            assert decode_ratio(c, p_bf16, splits, ref,
                                mutant="lens+1") == math.inf

    @pytest.mark.parametrize("dtype", DTYPES)
    @pytest.mark.parametrize("mutant", ["lens-1", "lens+1"])
    def test_off_by_one_caught_by_census(self, mutant, dtype, p_bf16):
        for ctx in ao.CENSUS_CTX:
            c = ao.census_case(ctx, ao.census_rows(ctx), 4, dtype)
            assert decode_ratio(c, p_bf16, ao.CENSUS_SPLITS[ctx],
                                mutant=mutant) > 4, ctx

    @pytest.mark.parametrize("dtype", DTYPES)
    def test_skipped_split_caught_by_census(self, dtype, p_bf16):
        for ctx in (300, 2000):
            c = ao.census_case(ctx, ao.census_rows(ctx), 4, dtype)
            assert decode_ratio(c, p_bf16, ao.CENSUS_SPLITS[ctx],
                                mutant="skip_split") > 4, ctx

    @pytest.mark.parametrize("dtype", DTYPES)
    def test_tile_counted_twice_caught_by_census(self, dtype, p_bf16):
        for ctx in (300, 2000):
            c = ao.census_case(ctx, ao.census_rows(ctx), 4, dtype)
            for splits in (1, ao.CENSUS_SPLITS[ctx]):
                assert decode_ratio(c, p_bf16, splits,
                                    mutant="dup_tile") > 4, (ctx, splits)

    def test_missing_rescale_caught_by_ramp(self, p_bf16):
        """Accumulator not multiplied by corr: the rising ramp is the one
        where corr << 1 on every tile; on the falling ramp corr = 1 and the
        mutant is (correctly) invisible."""
        for S, splits in [(ao.RAMP_UNSPLIT_S, 1), *ao.RAMP_SPLITS.items()]:
            c = ao.ramp_case("up", S)
            assert decode_ratio(c, p_bf16, splits, mutant="no_rescale") > 50
            c = ao.ramp_case("down", S)
            assert decode_ratio(c, p_bf16, splits, mutant="no_rescale") <= 1

    def test_missing_merge_weights_caught_by_ramp(self, p_bf16):
        """Merge without exp(m_w - M)."""
        for S, splits in ao.RAMP_SPLITS.items():
            for direction in ("up", "peak"):
                c = ao.ramp_case(direction, S,
                                 peak_pos=ao.ramp_peak_pos(splits))
                assert decode_ratio(c, p_bf16, splits,
                                    mutant="no_merge_weights") > 50

    def test_reference_without_q_quantisation_rejects_fp8(self, p_bf16):
        """Why decode_ref64 has q_fp8: against a reference that keeps Q in
        bf16, a correct fp8 kernel fails on the format's error alone."""
        c, *ref = ao.cached_ref(ao.grid_case, 256, FP8, 6.0)
        assert decode_ratio(c, p_bf16, 2, ref) <= 1.0
        plain = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale, q_fp8=False)
        assert decode_ratio(c, p_bf16, 2, plain) > 4
        # and the other way round: the emulation without the quantisation
        assert decode_ratio(c, p_bf16, 2, ref, quantize_q=False) > 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_strict_causal_mask_caught_by_prefill_census(dtype):
    """kp < qr instead of kp <= qr: every row loses its own position."""
    for S in (1, 65):
        c = ao.prefill_census_case(2, 8, 2, S, dtype)
        assert prefill_ratio(c, mutant="causal<") > 4
        c = ao.prefill_sentinel_case(2, 8, 2, S, dtype, seed=S)
        assert prefill_ratio(c, mutant="causal<") > 4


def test_randn_and_loose_tolerance_miss_the_dropped_row():
    """The gap this oracle closes: at ctx = 2000 a kernel that drops the
    newest row still passes randn inputs at atol = rtol = 2e-2."""
    g = torch.Generator().manual_seed(11)
    q = torch.randn(1, 4, 128, generator=g).to(BF16)
    k = torch.randn(1, 1, 2008, 128, generator=g).to(BF16)
    v = torch.randn(1, 1, 2008, 128, generator=g).to(BF16)
    c = ao._case(q, k, v, [2000])
    ref, _ = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale)
    out = emulate_decode(c, False, 16, mutant="lens-1").double()
    assert bool(((out - ref).abs() <= 2e-2 + 2e-2 * ref.abs()).all())


# --------------------------------------------------------------------------
# the oracle itself
# --------------------------------------------------------------------------

def test_decode_ref64_agrees_with_ops_reference():
    c = ao.sentinel_case(3, 8, 2, 70, [1, 33, 70], BF16, seed=1,
                         score_gain=1.0)
    ref, absref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale)
    old = ops.gqa_decode_attn_ref(c.q, c.k, c.v, c.lens, c.scale)
    assert (ref - old.double()).abs().max() <= 1e-5 * max(1.0, float(ref.abs().max()))
    assert bool((absref >= ref.abs() - 1e-12).all())


def test_prefill_ref64_agrees_with_naive_loop():
    c = ao.prefill_sentinel_case(2, 4, 2, 9, BF16, seed=2, score_gain=1.0)
    ref, _ = ao.prefill_ref64(c.q, c.k, c.v, c.batch, c.seq, c.scale)
    q = c.q.double().reshape(2, 9, 4, 128)
    for b in range(2):
        for h in range(4):
            for i in range(9):
                kk = c.k[b, h // 2, :i + 1].double()
                p = torch.softmax(kk @ q[b, i, h] * c.scale, dim=0)
                want = p @ c.v[b, h // 2, :i + 1].double()
                assert torch.allclose(ref[b * 9 + i, h], want, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_rows_are_exactly_zero_and_dead_rows_unseen(dtype):
    c = ao.empty_case(64, dtype)
    ref, absref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale,
                                  q_fp8=c.fp8)
    for b in (0, 2):
        assert torch.equal(ref[b], torch.zeros_like(ref[b]))
        assert torch.equal(absref[b], torch.zeros_like(ref[b]))
    for kind in ("nan", "max", "zero"):
        k, v = ao.poison_dead_rows(c.k, c.v, c.lens, kind)
        assert bool(torch.equal(k[3], c.k[3]))          # lens == S: untouched
        if kind == "nan":
            assert bool(k.float()[0].isnan().all())
        again, _ = ao.decode_ref64(c.q, k, v, c.lens, c.scale, q_fp8=c.fp8)
        assert torch.equal(again, ref)


def test_error_ratio_has_no_floor():
    ref = torch.zeros(1, 1, 4, dtype=torch.float64)
    bound = ao.attn_bound(ref, ref, True)
    assert ao.error_ratio(torch.zeros(1, 1, 4), ref, bound)[0] == 0.0
    out = torch.tensor([[[0.0, 0.0, 1e-30, 0.0]]])
    assert ao.error_ratio(out, ref, bound) == (math.inf, (0, 0, 2))
    out[0, 0, 1] = math.nan
    assert ao.error_ratio(out, ref, bound)[0] == math.inf
    with pytest.raises(AssertionError, match=r"\(0, 0, 1\)"):
        ao.assert_within(out, ref, bound)


def test_q_quantisation_matches_the_kernel_recipe():
    q = torch.tensor([[[448.0] + [0.0] * 127, [3.0] + [0.0] * 127]]).to(BF16)
    got = ao.quantize_q_fp8(q, 1)           # one group: scale 1, 3 exact
    assert torch.equal(got, q.float())
    got = ao.quantize_q_fp8(q, 2)           # own groups: both exact
    assert torch.equal(got, q.float())
    q[0, 1, 1] = 0.3                        # 0.3 * 448/3 = 44.8 -> 44 (ulp 4)
    got = ao.quantize_q_fp8(q, 2)
    assert got[0, 1, 1] == pytest.approx(44.0 * 3.0 / 448.0, rel=1e-6)
    assert bool(torch.equal(ao.quantize_q_fp8(torch.zeros(1, 2, 128), 1),
                            torch.zeros(1, 2, 128)))


def test_rope_delta_per_position(capsys):
    """Prints delta(pos), the angle error the GPU test allows, and pins its
    order of magnitude: 0 at position 0, float32 spacing of the angle
    elsewhere."""
    pos = torch.tensor(ao.ROPE_POSITIONS)
    for D in (128, 64):
        delta = ao.rope_delta(pos, D)
        with capsys.disabled():
            print(f"\nrope delta(pos), D={D}: " + ", ".join(
                f"{p}: {float(d):.3g}" for p, d in zip(ao.ROPE_POSITIONS,
                                                       delta)))
        assert float(delta[0]) == 0.0
        for p, d in zip(ao.ROPE_POSITIONS[1:], delta[1:]):
            # a few float32 ulps of the largest angle (= pos, at d = 0)
            assert 0 < float(d) <= 4 * 4 * p * 2.0 ** -24


def test_rope_ref64_agrees_with_ops_reference_at_small_positions():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 2, 128, generator=g).to(BF16)
    pos = torch.tensor([0, 1, 77])
    ref = ao.rope_ref64(x, pos)
    old, _ = ops.rope_ref(x, x, pos, ao.ROPE_THETA)
    assert (ref - old.double()).abs().max() < 1e-4
    assert torch.equal(ref[0], x[0].double())      # cos 0 = 1, sin 0 = 0
    assert bool((ao.rope_bound(x, ref, pos)[0] == 2.0 ** -8 * ref[0].abs()).all())
