"""GPU tests that can see a dropped position, a lost split or a wrong
rotation: decode attention v4/v5 (bf16 and fp8 caches, unsplit and split),
the split merge, prefill attention and RoPE at long positions, against the
float64 oracle and the derived bounds of attn_oracle.py.

test_attn_oracle_cpu.py shows on the CPU that these cases and bounds reject
the corresponding mutants. Every decode test asserts, through
ops.gqa_decode_num_splits, the split count it means to exercise. Each test
prints its worst err/bound ratio (`-s` shows them; docs/testing.md records
them).
"""
import pytest
import torch

import attn_oracle as ao
import paged_cases as pc
from attn_oracle import BF16, FP8
from wva_amd import ops

pytestmark = pytest.mark.gpu

VARIANTS = ["v4", "v5"]
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
SPLIT = [pytest.param(False, id="split"), pytest.param(True, id="unsplit")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(family, variant, dtype, ratio, note=""):
    name = "fp8" if dtype == FP8 else "bf16"
    print(f"\n[attn-edges] family={family} variant={variant} dtype={name} "
          f"ratio={ratio:.3f} {note}")


def decode(c, variant, dev, replicas=1, splits=None, k=None, v=None):
    """Run the decode kernel on case `c`, its batch repeated `replicas`
    times (how a small case gets a grid large enough to stay unsplit).
    Asserts the split count and that every replica is bit-equal to the
    first; returns the first replica's output on the CPU."""
    k = c.k if k is None else k
    v = c.v if v is None else v
    B, Hk, S = k.shape[0], k.shape[1], k.shape[2]
    assert ops.gqa_decode_num_splits(B * replicas, Hk, S) == splits, (
        "the launch heuristic no longer splits this shape as the test "
        "assumes")

    def rep(t):
        # e4m3 tensors are moved as bytes
        raw = t.view(torch.uint8) if t.dtype == FP8 else t
        raw = raw.to(dev).repeat(replicas, *([1] * (t.dim() - 1)))
        return raw.view(t.dtype)

    out = ops.gqa_decode_attn(rep(c.q), rep(k), rep(v), rep(c.lens), c.scale,
                              variant=variant)
    out = out.reshape(replicas, B, *out.shape[1:])
    assert torch.equal(out, out[:1].expand_as(out)), "replicas differ"
    return out[0].cpu()


def check(out, ref, absref, variant, what):
    bound = ao.attn_bound(ref, absref, p_bf16=(variant == "v5"))
    return ao.assert_within(out, ref, bound, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
class TestDecodeEdges:
    @pytest.mark.parametrize("unsplit", SPLIT)
    @pytest.mark.parametrize("gain", ao.GAINS)
    @pytest.mark.parametrize("G", ao.EDGE_GROUPS)
    def test_sentinel_tile_edges(self, dev, G, gain, unsplit, variant, dtype):
        """One row per context length at the tile edges (1 .. 129, S-1, S):
        the newest row must carry its full weight (dim 1), the first dead
        row none at all (dim 2, bound 0)."""
        c, ref, absref = ao.cached_ref(ao.edge_case, G, dtype, gain)
        if unsplit:
            out = decode(c, variant, dev, splits=1,
                         replicas=ao.UNSPLIT_REPLICAS // len(ao.EDGE_LENS))
        else:
            out = decode(c, variant, dev, splits=ao.EDGE_SPLITS)
        r = check(out, ref, absref, variant, f"edges G={G} gain={gain}")
        record("sentinel-edges", variant, dtype, r,
               f"G={G} gain={gain} unsplit={unsplit}")

    @pytest.mark.parametrize("gain", ao.GAINS)
    @pytest.mark.parametrize("S", list(ao.SPLIT_GRID))
    def test_sentinel_split_grid(self, dev, S, gain, variant, dtype):
        """lens = [1, 65, S/2+1, S] at every split count of the grid: from
        ctx << max_seq, where most splits are empty, to the full cache."""
        c, ref, absref = ao.cached_ref(ao.grid_case, S, dtype, gain)
        out = decode(c, variant, dev, splits=ao.SPLIT_GRID[S])
        r = check(out, ref, absref, variant, f"grid S={S} gain={gain}")
        record("sentinel-grid", variant, dtype, r,
               f"S={S} splits={ao.SPLIT_GRID[S]} gain={gain}")

    @pytest.mark.parametrize("S", (640, 2048))
    def test_sentinel_same_shapes_unsplit(self, dev, S, variant, dtype):
        """The same rows as the split grid, in a batch large enough that
        the launch does not split."""
        c, ref, absref = ao.cached_ref(ao.grid_case, S, dtype, 6.0)
        out = decode(c, variant, dev, splits=1,
                     replicas=ao.UNSPLIT_REPLICAS // 4)
        r = check(out, ref, absref, variant, f"grid-unsplit S={S}")
        record("sentinel-grid-unsplit", variant, dtype, r, f"S={S}")

    @pytest.mark.parametrize("unsplit", SPLIT)
    @pytest.mark.parametrize("ctx", ao.CENSUS_CTX)
    def test_census(self, dev, ctx, unsplit, variant, dtype):
        """Uniform softmax over a one-hot V: output dim d counts the live
        positions = d (mod 128). Any position lost, duplicated or
        mis-assigned, in a tile or in the merge, changes a count."""
        S = ao.census_rows(ctx)
        c = ao.census_case(ctx, S, 4, dtype)
        ref, absref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale,
                                      q_fp8=c.fp8)
        if unsplit:
            out = decode(c, variant, dev, splits=1,
                         replicas=ao.UNSPLIT_REPLICAS)
        else:
            out = decode(c, variant, dev, splits=ao.CENSUS_SPLITS[ctx])
        r = check(out, ref, absref, variant, f"census ctx={ctx}")
        record("census", variant, dtype, r, f"ctx={ctx} unsplit={unsplit}")

    @pytest.mark.parametrize("S", (64, 2048))
    def test_empty_sequences(self, dev, S, variant, dtype):
        """lens = [0, 7, 0, S]: empty rows are exactly 0, their neighbours
        within bound, nothing non-finite - unsplit (S = 64) and with 16
        splits, all of them empty for rows 0 and 2."""
        c, ref, absref = ao.cached_ref(ao.empty_case, S, dtype)
        out = decode(c, variant, dev, splits=ao.SPLIT_GRID[S])
        assert bool(torch.isfinite(out.float()).all())
        for b in (0, 2):
            assert torch.equal(out[b], torch.zeros_like(out[b])), b
        r = check(out, ref, absref, variant, f"empty S={S}")
        record("empty", variant, dtype, r, f"S={S}")

    @pytest.mark.parametrize("kind", ("nan", "max"))
    @pytest.mark.parametrize("S", (64, 2048))
    def test_dead_rows_are_never_read(self, dev, S, kind, variant, dtype):
        """Rows >= lens[b] poisoned with NaN or the largest finite value
        give the bit-identical output of zeroed dead rows, which is within
        bound. lens are strictly inside a tile and < S."""
        c, ref, absref = ao.cached_ref(ao.poison_case, S, dtype)
        splits = ao.SPLIT_GRID[S]
        kz, vz = ao.poison_dead_rows(c.k, c.v, c.lens, "zero")
        kp, vp = ao.poison_dead_rows(c.k, c.v, c.lens, kind)
        clean = decode(c, variant, dev, splits=splits, k=kz, v=vz)
        dirty = decode(c, variant, dev, splits=splits, k=kp, v=vp)
        assert bool(torch.isfinite(dirty.float()).all())
        assert torch.equal(clean, dirty)
        r = check(clean, ref, absref, variant, f"poison S={S}")
        record("poison", variant, dtype, r, f"S={S} kind={kind}")

    def test_deterministic(self, dev, variant, dtype):
        """No atomics anywhere in the path: two calls are bit-equal."""
        for S in (64, 2048):
            c = ao.grid_case(S, dtype, 6.0)
            a = decode(c, variant, dev, splits=ao.SPLIT_GRID[S])
            b = decode(c, variant, dev, splits=ao.SPLIT_GRID[S])
            assert torch.equal(a, b), S


@pytest.mark.parametrize("variant", VARIANTS)
class TestDecodeRamp:
    @pytest.mark.parametrize("S", [ao.RAMP_UNSPLIT_S, *ao.RAMP_SPLITS])
    @pytest.mark.parametrize("direction", ao.RAMP_DIRECTIONS)
    def test_ramp(self, dev, direction, S, variant):
        """Scores monotone over ~60 (x 0.5..1.5 per head): the online
        softmax rescale and the merge weights exp(m_w - M) span many orders
        of magnitude."""
        unsplit = S == ao.RAMP_UNSPLIT_S
        splits = 1 if unsplit else ao.RAMP_SPLITS[S]
        c = ao.ramp_case(direction, S, peak_pos=ao.ramp_peak_pos(splits))
        ref, absref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale)
        out = decode(c, variant, dev, splits=splits,
                     replicas=ao.UNSPLIT_REPLICAS if unsplit else 1)
        r = check(out, ref, absref, variant, f"ramp {direction} S={S}")
        record(f"ramp-{direction}", variant, BF16, r, f"S={S}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_dispatch_is_the_named_variant(dev, dtype):
    """`auto` is v5 when G >= 8 or the grid is unsplit, else v4: bit-equal
    to the named kernel on split and unsplit sentinel cases."""
    for c, splits, picked in [
        (ao.grid_case(640, dtype, 6.0), 5, "v4"),           # G = 4, split
        (ao.grid_case(64, dtype, 6.0), 1, "v5"),            # G = 4, unsplit
        (ao.edge_case(8, dtype, 6.0), ao.EDGE_SPLITS, "v5"),  # G = 8, split
    ]:
        forced = decode(c, picked, dev, splits=splits)
        auto = ops.gqa_decode_attn(c.q.to(dev), c.k.to(dev), c.v.to(dev),
                                   c.lens.to(dev), c.scale).cpu()
        assert torch.equal(auto, forced), (splits, picked)
        other = decode(c, "v4" if picked == "v5" else "v5", dev,
                       splits=splits)
        assert not torch.equal(auto, other), "variants indistinguishable"


FORCED_LENS = (130, 65)  # two tiles + two rows; one tile + one row


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", (1, 2, 3))
def test_forced_splits_on_the_contiguous_op(dev, n, variant, dtype):
    """ops.gqa_decode_attn with num_splits and variant forced, B=2, Hq=8,
    Hk=2 over caches of 192 rows. With n = 3 the 65-row sequence has a split
    that meets no tile (the m = -inf merge path). Finite, within the oracle
    bound, bit-equal to ops.paged_decode_attn over the same rows at the same
    n and variant; num_splits=None is the call forced to
    gqa_decode_num_splits."""
    c, ref, absref = ao.cached_ref(ao.sentinel_case, 2, 8, 2, 192,
                                   FORCED_LENS, dtype, 31, 6.0)
    p = pc.scatter_case(c, 16)

    def put(t):  # e4m3 tensors are moved as bytes
        return (t.view(torch.uint8).to(dev).view(FP8) if t.dtype == FP8
                else t.to(dev))

    q, k, v, lens = put(c.q), put(c.k), put(c.v), c.lens.to(dev)
    out = ops.gqa_decode_attn(q, k, v, lens, c.scale, num_splits=n,
                              variant=variant)
    assert bool(torch.isfinite(out.float()).all())
    r = check(out.cpu(), ref, absref, variant, f"forced splits n={n}")
    paged = ops.paged_decode_attn(q, put(p.k_pages), put(p.v_pages),
                                  p.tables.to(dev), lens, c.scale,
                                  num_splits=n, variant=variant)
    assert torch.equal(out, paged)
    auto_n = ops.gqa_decode_num_splits(2, 2, 192)
    assert torch.equal(
        ops.gqa_decode_attn(q, k, v, lens, c.scale, variant=variant),
        ops.gqa_decode_attn(q, k, v, lens, c.scale, num_splits=auto_n,
                            variant=variant))
    record("forced-splits", variant, dtype, r, f"n={n}")


# --------------------------------------------------------------------------
# prefill
# --------------------------------------------------------------------------

def prefill(c, dev, k=None, v=None):
    k = c.k if k is None else k
    v = c.v if v is None else v
    return ops.prefill_attn(c.q.to(dev), k.to(dev), v.to(dev), c.batch,
                            c.seq, c.scale).cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk", ao.PREFILL_HEADS)
@pytest.mark.parametrize("S", ao.PREFILL_S)
class TestPrefillEdges:
    def test_causal_census(self, dev, S, hq, hk, dtype):
        """Query row i counts the positions <= i per residue mod 128."""
        c = ao.prefill_census_case(2, hq, hk, S, dtype)
        ref, absref = ao.prefill_ref64(c.q, c.k, c.v, c.batch, c.seq, c.scale)
        out = prefill(c, dev)
        r = ao.assert_within(out, ref, ao.attn_bound(ref, absref, True),
                             f"prefill census S={S}")
        record("prefill-census", "prefill", dtype, r, f"S={S} {hq}/{hk}")

    def test_sentinel_and_dead_rows(self, dev, S, hq, hk, dtype):
        """Peaked softmax; row i's own key is its newest, cache rows >= S
        must never show (dim 2, bound 0), and NaN in them changes no bit."""
        c = ao.prefill_sentinel_case(2, hq, hk, S, dtype, seed=S)
        ref, absref = ao.prefill_ref64(c.q, c.k, c.v, c.batch, c.seq, c.scale)
        lens = [S] * c.batch
        kz, vz = ao.poison_dead_rows(c.k, c.v, lens, "zero")
        kp, vp = ao.poison_dead_rows(c.k, c.v, lens, "nan")
        out = prefill(c, dev)
        clean = prefill(c, dev, kz, vz)
        dirty = prefill(c, dev, kp, vp)
        assert bool(torch.isfinite(dirty.float()).all())
        assert torch.equal(clean, dirty)
        assert torch.equal(clean, out)
        r = ao.assert_within(out, ref, ao.attn_bound(ref, absref, True),
                             f"prefill sentinel S={S}")
        record("prefill-sentinel", "prefill", dtype, r, f"S={S} {hq}/{hk}")


# --------------------------------------------------------------------------
# RoPE at long positions
# --------------------------------------------------------------------------

def rope_inputs(D, seed):
    g = torch.Generator().manual_seed(seed)
    T = len(ao.ROPE_POSITIONS)
    q = torch.randn(T, 8, D, generator=g).to(BF16)
    k = torch.randn(T, 2, D, generator=g).to(BF16)
    v = torch.randn(T, 2, D, generator=g).to(BF16)
    return q, k, v, torch.tensor(ao.ROPE_POSITIONS, dtype=torch.int32)


def rope_ratios(name, out, x, pos):
    """Worst err/bound per position against rope_ref64; prints all of them,
    returns the list of (position, ratio, index) that exceed 1."""
    ref = ao.rope_ref64(x, pos)
    bound = ao.rope_bound(x, ref, pos)
    bad = []
    for t, p in enumerate(ao.ROPE_POSITIONS):
        r, idx = ao.error_ratio(out[t].cpu(), ref[t], bound[t])
        print(f"\n[attn-edges] family=rope kernel={name} pos={p} "
              f"ratio={r:.3f}")
        if r > 1.0:
            bad.append((p, r, idx))
    return bad


class TestRopeLongPositions:
    @pytest.mark.parametrize("D", (128, 64))
    def test_rope(self, dev, D):
        q, k, _, pos = rope_inputs(D, seed=D)
        qd, kd = q.to(dev), k.to(dev)
        ops.rope(qd, kd, pos.to(dev), ao.ROPE_THETA)
        bad = rope_ratios(f"rope-D{D}-q", qd, q, pos)
        bad += rope_ratios(f"rope-D{D}-k", kd, k, pos)
        assert not bad, f"(position, err/bound, index): {bad}"

    @pytest.mark.parametrize("dtype", DTYPES)
    def test_rope_append_kv(self, dev, dtype):
        """One sequence per position, each appending at its own position of
        a 131072-row cache. q and a bf16 K are held to the rope bound; an
        fp8 K to one e4m3 ulp of the quantised float64 reference; V is a
        copy (exact, or equal to the e4m3 cast)."""
        D, Hq, Hk, S = 128, 8, 2, 131072
        q, k, v, pos = rope_inputs(D, seed=7)
        T = len(pos)
        qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1),
                         v.reshape(T, -1)], dim=1).contiguous()
        raw = torch.uint8 if dtype == FP8 else BF16   # e4m3 handled as bytes
        kc = torch.zeros(T, Hk, S, D, device=dev, dtype=raw).view(dtype)
        vc = torch.zeros(T, Hk, S, D, device=dev, dtype=raw).view(dtype)
        q_out = ops.rope_append_kv(qkv.to(dev), kc, vc, pos.to(dev), Hq, Hk,
                                   ao.ROPE_THETA)
        k_new = torch.stack([kc.view(raw)[t, :, p] for t, p in
                             enumerate(ao.ROPE_POSITIONS)]).cpu().view(dtype)
        v_new = torch.stack([vc.view(raw)[t, :, p] for t, p in
                             enumerate(ao.ROPE_POSITIONS)]).cpu().view(dtype)
        name = "append-fp8" if dtype == FP8 else "append-bf16"
        bad = rope_ratios(f"{name}-q", q_out, q, pos)
        if dtype == FP8:
            assert torch.equal(v_new.view(torch.uint8),
                               v.to(FP8).view(torch.uint8))
            want = ao.rope_ref64(k, pos).float().to(FP8).float().double()
            got = k_new.float().double()
            ulp = ao.e4m3_ulp(torch.maximum(want.abs(), got.abs()))
            for t, p in enumerate(ao.ROPE_POSITIONS):
                r, i = ao.error_ratio(k_new[t].float(), want[t], ulp[t])
                print(f"\n[attn-edges] family=rope kernel={name}-k pos={p} "
                      f"ulps={r:.3f}")
                if r > 1.0:
                    bad.append((p, r, i))
        else:
            assert torch.equal(v_new, v)
            bad += rope_ratios(f"{name}-k", k_new, k, pos)
        assert not bad, f"(position, err/bound, index): {bad}"
