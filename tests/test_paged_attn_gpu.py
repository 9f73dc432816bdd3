"""GPU tests of the paged KV cache: paged decode attention v4/v5 (bf16 and
fp8 pools, block sizes 16/32/64), the paged RoPE append, and
LlamaDecodeModel(kv_layout="paged") eager and under a captured graph.

Two conditions throughout:
  * oracle: within attn_oracle.attn_bound of the cached float64 reference
    of the contiguous case (p_bf16 for v5);
  * bit-equality: torch.equal to ops.gqa_decode_attn on the contiguous case
    with the same pinned variant and the split count of the contiguous
    launch. The paged kernels change addresses only, so no rounding may
    differ; the condition is derived, not tuned.
The pools come from paged_cases.py: shuffled pages, NaN in every unused
page, in every dead row and behind every dead table entry.

No test here feeds a table entry outside [0, num_blocks) or a position past
the reservation: the clamp and skip guards are shown by the CPU reference
tests (test_paged_kv_cpu.py) and by reading the kernels.

Worst err/bound ratios measured on an MI355X (`-s` prints them) are in
docs/testing.md.
"""
import functools

import pytest
import torch

import attn_oracle as ao
import paged_cases as pc
from attn_oracle import BF16, FP8
from wva_amd import ops

pytestmark = pytest.mark.gpu

VARIANTS = ["v4", "v5"]
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(FP8, id="fp8")]
BLOCK_SIZES = (16, 32, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(family, variant, dtype, ratio, note=""):
    name = "fp8" if dtype == FP8 else "bf16"
    print(f"\n[paged-attn] family={family} variant={variant} dtype={name} "
          f"ratio={ratio:.3f} {note}")


def put(t, dev):
    """e4m3 tensors are moved as bytes."""
    if t.dtype == FP8:
        return t.view(torch.uint8).to(dev).view(FP8)
    return t.to(dev)


@functools.lru_cache(maxsize=None)
def pool_of(case_fn, block_size, *args):
    """The scattered pool of a cached attn_oracle case, built once."""
    return pc.scatter_case(case_fn(*args), block_size)


def contiguous(c, variant, dev, splits):
    """The contiguous kernel's output, after asserting its split count."""
    B, Hk, S = c.k.shape[0], c.k.shape[1], c.k.shape[2]
    assert ops.gqa_decode_num_splits(B, Hk, S) == splits, (
        "the launch heuristic no longer splits this shape as the test "
        "assumes")
    return ops.gqa_decode_attn(
        put(c.q, dev), put(c.k, dev), put(c.v, dev), c.lens.to(dev), c.scale,
        variant=variant).cpu()


def paged(c, p, variant, dev, splits):
    return ops.paged_decode_attn(
        put(c.q, dev), put(p.k_pages, dev), put(p.v_pages, dev),
        p.tables.to(dev), c.lens.to(dev), c.scale, splits,
        variant=variant).cpu()


def check(out, ref, absref, variant, what):
    bound = ao.attn_bound(ref, absref, p_bf16=(variant == "v5"))
    return ao.assert_within(out, ref, bound, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
class TestPagedDecode:
    @pytest.mark.parametrize("block_size", BLOCK_SIZES)
    @pytest.mark.parametrize("gain", ao.GAINS)
    @pytest.mark.parametrize("G", ao.EDGE_GROUPS)
    def test_tile_edges(self, dev, G, gain, block_size, variant, dtype):
        """One row per context length at the tile and page edges, 2 splits:
        both conditions; once more unsplit, against the oracle."""
        c, ref, absref = ao.cached_ref(ao.edge_case, G, dtype, gain)
        p = pool_of(ao.edge_case, block_size, G, dtype, gain)
        out = paged(c, p, variant, dev, ao.EDGE_SPLITS)
        what = f"edges G={G} gain={gain} bs={block_size}"
        r = check(out, ref, absref, variant, what)
        assert torch.equal(out, contiguous(c, variant, dev, ao.EDGE_SPLITS))
        one = paged(c, p, variant, dev, 1)
        r1 = check(one, ref, absref, variant, what + " unsplit")
        record("edges", variant, dtype, max(r, r1), what)

    @pytest.mark.parametrize("S", (640, 2048, 20008))
    def test_split_grid(self, dev, S, variant, dtype):
        """lens = [1, 65, S/2+1, S] at the contiguous split counts of the
        grid; S = 20008 ends in a half-filled page."""
        c, ref, absref = ao.cached_ref(ao.grid_case, S, dtype, 6.0)
        p = pool_of(ao.grid_case, 16, S, dtype, 6.0)
        splits = ao.SPLIT_GRID[S]
        out = paged(c, p, variant, dev, splits)
        r = check(out, ref, absref, variant, f"grid S={S}")
        assert torch.equal(out, contiguous(c, variant, dev, splits))
        record("grid", variant, dtype, r, f"S={S} splits={splits}")

    @pytest.mark.parametrize("ctx", (65, 1000))
    def test_census(self, dev, ctx, variant, dtype):
        """Uniform softmax over a one-hot V: a lost, duplicated or
        mis-assigned page changes a count."""
        c = ao.census_case(ctx, ao.census_rows(ctx), 8, dtype)
        ref, absref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale,
                                      q_fp8=c.fp8)
        p = pc.scatter_case(c, 16)
        splits = ao.CENSUS_SPLITS[ctx]
        out = paged(c, p, variant, dev, splits)
        r = check(out, ref, absref, variant, f"census ctx={ctx}")
        assert torch.equal(out, contiguous(c, variant, dev, splits))
        record("census", variant, dtype, r, f"ctx={ctx}")

    @pytest.mark.parametrize("block_size", BLOCK_SIZES)
    def test_poison_and_empty(self, dev, block_size, variant, dtype):
        """NaN in every dead row, unused page and behind every dead table
        entry: outputs finite, dim 2 (the first dead row's sentinel)
        exactly 0, rows with lens == 0 exactly 0."""
        for fn in (ao.poison_case, ao.empty_case):
            c, ref, absref = ao.cached_ref(fn, 200, dtype)
            p = pool_of(fn, block_size, 200, dtype)
            splits = ops.gqa_decode_num_splits(4, 1, 200)
            for n in (splits, 1):
                out = paged(c, p, variant, dev, n)
                assert bool(torch.isfinite(out.float()).all())
                assert bool((out[..., 2] == 0).all())
                for b, ln in enumerate(c.lens.tolist()):
                    if ln == 0:
                        assert torch.equal(out[b], torch.zeros_like(out[b]))
                r = check(out, ref, absref, variant,
                          f"{fn.__name__} bs={block_size} splits={n}")
            assert torch.equal(paged(c, p, variant, dev, splits),
                               contiguous(c, variant, dev, splits))
            record(fn.__name__, variant, dtype, r, f"bs={block_size}")

    def test_shared_prefix(self, dev, variant, dtype):
        """Four sequences whose tables alias the same physical pages for
        the first 3 full blocks and differ after: bit-equal to the
        contiguous kernel on the materialised copies."""
        bs, shared = 16, 3
        lens = [50, 70, 100, 136]
        c = ao.sentinel_case(4, 4, 1, 136, lens, dtype, seed=77,
                             score_gain=6.0)
        for t in (c.k, c.v):
            rows = pc.raw(t)
            rows[1:, :, :shared * bs] = rows[:1, :, :shared * bs]
        p = pc.scatter(c.k, c.v, lens, bs, shared_blocks=shared)
        t = p.tables
        assert bool((t[:, :shared] == t[0, :shared]).all())
        assert len(set(t[:, shared].tolist())) == 4
        splits = ops.gqa_decode_num_splits(4, 1, 136)
        out = paged(c, p, variant, dev, splits)
        assert torch.equal(out, contiguous(c, variant, dev, splits))
        ref, absref = ao.decode_ref64(c.q, c.k, c.v, c.lens, c.scale,
                                      q_fp8=c.fp8)
        r = check(out, ref, absref, variant, "shared prefix")
        record("shared-prefix", variant, dtype, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_is_the_contiguous_rule(dev, dtype):
    """`auto` is v5 when G >= 8 or unsplit, else v4, and num_splits=None
    asks paged_decode_num_splits."""
    c = ao.grid_case(640, dtype, 6.0)                       # G = 4
    p = pool_of(ao.grid_case, 16, 640, dtype, 6.0)
    assert ops.paged_decode_num_splits(4, 1, 40, 16) == ao.SPLIT_GRID[640]
    auto = ops.paged_decode_attn(
        put(c.q, dev), put(p.k_pages, dev), put(p.v_pages, dev),
        p.tables.to(dev), c.lens.to(dev), c.scale).cpu()
    assert torch.equal(auto, paged(c, p, "v4", dev, ao.SPLIT_GRID[640]))
    assert torch.equal(paged(c, p, "auto", dev, 1), paged(c, p, "v5", dev, 1))
    c8 = ao.edge_case(8, dtype, 6.0)
    p8 = pool_of(ao.edge_case, 16, 8, dtype, 6.0)
    assert torch.equal(paged(c8, p8, "auto", dev, 2),
                       paged(c8, p8, "v5", dev, 2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block_size", (16, 64))
def test_append(dev, block_size, dtype):
    """ext.rope_append_kv_paged against ext.rope_append_kv: q bit-equal,
    the written rows gathered back bit-equal, the rest of the pool
    byte-identical to before."""
    ext = ops._require_ext()
    qkv, k, v, pos, lens = pc.append_inputs(dtype, block_size)
    before = pc.scatter(k, v, lens, block_size)
    kc, vc = put(k, dev), put(v, dev)
    q_want = ext.rope_append_kv(qkv.to(dev), kc, vc, pos.to(dev),
                                pc.APPEND_HQ, pc.APPEND_HK, ao.ROPE_THETA)
    kp, vp = put(before.k_pages, dev), put(before.v_pages, dev)
    q_got = ext.rope_append_kv_paged(
        qkv.to(dev), kp, vp, before.tables.to(dev), pos.to(dev),
        pc.APPEND_HQ, pc.APPEND_HK, ao.ROPE_THETA)
    assert torch.equal(q_got.cpu(), q_want.cpu())
    kc, vc, kp, vp = (put(t, "cpu") for t in (kc, vc, kp, vp))
    for got, want, old in ((kp, kc, before.k_pages), (vp, vc, before.v_pages)):
        untouched = torch.ones(pc.raw(got).shape[:3], dtype=torch.bool)
        for b, n in enumerate(pc.APPEND_POSITIONS):
            row = pc.gather_row(got, before.tables, b, n, block_size)
            assert torch.equal(row, pc.raw(want)[b, :, n]), (b, n)
            untouched[int(before.tables[b, n // block_size]), :,
                      n % block_size] = False
        assert torch.equal(pc.raw(got)[untouched], pc.raw(old)[untouched])
    assert not torch.equal(pc.raw(kp), pc.raw(before.k_pages))


class TestPagedModel:
    BATCH, STEPS = 4, 40

    def models(self):
        from wva_amd.calibration.model import TINY, LlamaDecodeModel

        kw = dict(max_batch=self.BATCH, max_seq=256, seed=2)
        return (LlamaDecodeModel(TINY, **kw),
                LlamaDecodeModel(TINY, kv_layout="paged", block_size=16, **kw),
                TINY)

    def tokens(self, cfg, dev):
        g = torch.Generator().manual_seed(5)
        return torch.randint(0, cfg.vocab_size, (self.STEPS, self.BATCH),
                             generator=g).to(dev)

    def test_paged_equals_contiguous_and_graph_equals_eager(self, dev):
        """TINY paged (16) against contiguous from reset(4, 0): the logits
        of 40 steps are equal. The same paged model under a captured graph
        replays the eager paged logits."""
        from wva_amd.calibration.graph import GraphedDecoder

        ref, model, cfg = self.models()
        toks = self.tokens(cfg, dev)
        ref.reset(self.BATCH, 0)
        model.reset(self.BATCH, 0)
        ids = model.block_tables.cpu().reshape(-1).tolist()
        assert sorted(ids) == list(range(len(ids))) and ids != sorted(ids)
        eager = []
        for t in toks:
            a, b = ref.decode_step(t), model.decode_step(t)
            assert torch.equal(a, b)
            eager.append(b.clone())
        assert bool(torch.isfinite(eager[-1].float()).all())
        assert model.context_lens.tolist() == [self.STEPS] * self.BATCH

        gd = GraphedDecoder(model, batch=self.BATCH)
        gd.reset_to(self.BATCH, 0)
        for t, want in zip(toks, eager):
            assert torch.equal(gd.decode_step(t), want)
