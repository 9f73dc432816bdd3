"""The tiled (LDS-staged, 128-row m-tile) grouped MoE GEMMs of csrc/moe.hip
against the float64 oracle of moe_oracle.py. Every kernel case forces
variant="tiled", so the shapes are the smallest around the 128-row tile
rather than prefill-sized; the bounds are the oracle's, with no absolute
floor."""
import functools
from types import SimpleNamespace

import pytest
import torch

import moe_oracle as mo
from moe_oracle import (BF16, SWIGLU_REL, assert_equal, assert_within,
                        down_bound, down_ref64, dyadic_weights, gate_up_bound,
                        gate_up_parts64, integer_rows, routing_from_counts)
from wva_amd import ops

pytestmark = pytest.mark.gpu

# per-expert row counts around the 128-row tile -> top_k
ROUTINGS = {
    "TILE_EDGES": ((0, 1, 127, 128, 129, 255, 256, 2), 2),   # T = 449
    "TIGHT": ((129, 129, 129, 129), 2),                      # T = 258
    "ONE_EACH": ((1,) * 64, 8),                              # T = 8
}
LIVE_AND_GRID = {"TILE_EDGES": (10, 15), "TIGHT": (8, 8), "ONE_EACH": (64, 64)}
GATE_UP_H = {"TILE_EDGES": 384, "TIGHT": 128, "ONE_EACH": 128}
DOWN_SHAPES = ((16, 128), (144, 896))
# a shape the shipped rule sends to the tiled kernels (T, K, E)
RULE_TILED = (258, 2, 4)
MLP_H, MLP_I = 384, 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def routing(name):
    """The namespace the oracle's references expect."""
    counts, K = ROUTINGS[name]
    topk_w, offsets, slots = routing_from_counts(counts, K)
    TK, E = sum(counts), len(counts)
    live, grid = LIVE_AND_GRID[name]
    assert sum(-(-c // 128) for c in counts) == live
    assert min(TK, TK // 128 + E) == grid
    pos_of_slot = torch.empty(TK, dtype=torch.int64)
    pos_of_slot[slots.long()] = torch.arange(TK)
    return SimpleNamespace(
        E=E, K=K, T=TK // K, TK=TK, topk_w=topk_w, offsets=offsets,
        slots=slots, pos_of_slot=pos_of_slot)


def gate_up(dev, r, x, w):
    out = ops.moe_gate_up_swiglu(
        x.to(dev), w.to(dev), r.offsets.to(dev), r.slots.to(dev), r.K,
        variant="tiled")
    assert out.dtype == BF16 and out.shape == (r.TK, w.shape[1] // 2)
    return out.cpu()


def down(dev, r, act, w, topk_w):
    """Stale NaN goes where the allocator will put the workspace, so an
    unwritten workspace row shows."""
    args = [t.to(dev) for t in (act, w, topk_w, r.offsets, r.slots)]
    prime = torch.full((r.TK * w.shape[1],), float("nan"), device=dev)
    del prime
    out = ops.moe_down_combine(*args, variant="tiled")
    assert out.dtype == BF16 and out.shape == (r.T, w.shape[1])
    return out.cpu()


@pytest.mark.parametrize("I", (16, 160))
@pytest.mark.parametrize("name", list(ROUTINGS))
def test_gate_up_integer(dev, name, I):
    r, H = routing(name), GATE_UP_H[name]
    g = torch.Generator().manual_seed(len(name) + 31 * I + H)
    x = integer_rows(r.T, H, seed=I + H + r.T).to(BF16)
    w = torch.randint(-2, 3, (r.E, 2 * I, H), generator=g).to(BF16)
    gg, uu, absg, absu = gate_up_parts64(x, w, r)
    assert float(torch.maximum(absg, absu).max()) <= 64
    ref = mo.silu64(gg) * uu
    ratio = assert_within(gate_up(dev, r, x, w), ref, SWIGLU_REL * ref.abs(),
                          f"tiled gate_up integer {name} H={H} I={I}")
    print(f"\n[moe-tiled] gate_up integer {name} I={I} ratio={ratio:.3f}")


def test_gate_up_bounded(dev):
    r, H, I = routing("TILE_EDGES"), 384, 160
    g = torch.Generator().manual_seed(78)
    x = torch.randn(r.T, H, generator=g).to(BF16)
    w = (torch.randn(r.E, 2 * I, H, generator=g) / H ** 0.5).to(BF16)
    ref, bound = gate_up_bound(x, w, r)
    ratio = assert_within(gate_up(dev, r, x, w), ref, bound,
                          "tiled gate_up bounded")
    print(f"\n[moe-tiled] gate_up bounded ratio={ratio:.3f}")


@pytest.mark.parametrize("H,I", DOWN_SHAPES)
@pytest.mark.parametrize("name", list(ROUTINGS))
def test_down_integer(dev, name, H, I):
    r = routing(name)
    g = torch.Generator().manual_seed(len(name) + H + 3 * I)
    act = integer_rows(r.TK, I, seed=H + I + r.TK).to(BF16)
    w = torch.randint(-2, 3, (r.E, H, I), generator=g).to(BF16)
    topk_w = dyadic_weights(r.T, r.K, seed=H)
    ref, absref = down_ref64(act, w, topk_w, r)
    assert float(absref.max()) <= 64
    assert_equal(down(dev, r, act, w, topk_w), ref.to(BF16),
                 f"tiled down integer {name} H={H} I={I}")


def test_down_bounded_and_deterministic(dev):
    r, (H, I) = routing("TILE_EDGES"), DOWN_SHAPES[1]
    g = torch.Generator().manual_seed(H + I + 12)
    act = torch.randn(r.TK, I, generator=g).to(BF16)
    w = (torch.randn(r.E, H, I, generator=g) / I ** 0.5).to(BF16)
    ref, absref = down_ref64(act, w, r.topk_w, r)
    first = down(dev, r, act, w, r.topk_w)
    second = down(dev, r, act, w, r.topk_w)
    ratio = assert_within(first, ref, down_bound(ref, absref, I, r.K),
                          "tiled down bounded")
    print(f"\n[moe-tiled] down bounded ratio={ratio:.3f}")
    assert torch.equal(first, second)


def graph_logit_sets():
    """Four routings of T = 258 over E = 4, K = 2: seeded pairs, expert 1
    empty, everything to the pair (2, 0), and 129 rows per expert, which
    fill the static tile grid of 8."""
    T, K, E = RULE_TILED
    g = torch.Generator().manual_seed(3)
    no1 = [(0, 2), (2, 3), (3, 0)]
    sets = {
        "balanced": [tuple(torch.randperm(E, generator=g)[:2].tolist())
                     for _ in range(T)],
        "empty": [no1[t % 3] for t in range(T)],
        "pair": [(2, 0)] * T,
        "tight": [(0, 1) if t < 129 else (2, 3) for t in range(T)],
    }
    out = {n: mo.counts_logits(p, E, seed=i)
           for i, (n, p) in enumerate(sets.items())}
    assert ops.moe_route_ref(out["tight"], K)[2].tolist() == [
        0, 129, 258, 387, 516]
    assert ops.moe_route_ref(out["pair"], K)[2].tolist() == [
        0, 258, 258, 516, 516]
    return out


@pytest.fixture(scope="module")
def mlp(dev):
    T, K, E = RULE_TILED
    g = torch.Generator().manual_seed(43)
    x = torch.randn(T, MLP_H, generator=g).to(BF16)
    w_gu = (torch.randn(E, 2 * MLP_I, MLP_H, generator=g)
            / MLP_H ** 0.5).to(BF16)
    w_dn = (torch.randn(E, MLP_H, MLP_I, generator=g) / MLP_I ** 0.5).to(BF16)
    return x.to(dev), w_gu.to(dev), w_dn.to(dev), graph_logit_sets()


def test_rule_and_composition(dev, mlp):
    T, K, E = RULE_TILED
    assert ops.moe_variant(130, 2, 4) == "stream"
    assert ops.moe_variant(256, 2, 8) == "stream"
    assert ops.moe_variant(T, K, E) == "tiled"
    x, w_gu, w_dn, sets = mlp
    with pytest.raises(ValueError):
        ops.moe_mlp(x, sets["tight"].to(dev), w_gu, w_dn, K, variant="lds")
    for name in ("balanced", "tight"):
        lg = sets[name].to(dev)
        whole = ops.moe_mlp(x, lg, w_gu, w_dn, K)
        _, topk_w, offsets, slots = ops.moe_route(lg, K)
        act = ops.moe_gate_up_swiglu(x, w_gu, offsets, slots, K,
                                     variant="tiled")
        parts = ops.moe_down_combine(act, w_dn, topk_w, offsets, slots,
                                     variant="tiled")
        assert torch.equal(whole, parts), name
        # and it is right: the down bound on the kernel's own act
        r = SimpleNamespace(T=T, K=K, E=E, TK=T * K, offsets=offsets.cpu(),
                            slots=slots.cpu(),
                            pos_of_slot=torch.argsort(slots.cpu().long()))
        ref, absref = down_ref64(act.cpu(), w_dn.cpu(), topk_w.cpu(), r)
        assert_within(whole.cpu(), ref, down_bound(ref, absref, MLP_I, K),
                      name)


def test_graph_replays_with_fresh_routing(dev, mlp):
    """Captured on the balanced routing, replayed on three others; the last
    fills the tile grid to its last workgroup."""
    x, w_gu, w_dn, sets = mlp
    K = RULE_TILED[1]
    eager = {n: ops.moe_mlp(x, lg.to(dev), w_gu, w_dn, K,
                            variant="tiled").clone()
             for n, lg in sets.items()}
    assert not torch.equal(eager["balanced"], eager["tight"])
    static_logits = sets["balanced"].to(dev).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.moe_mlp(x, static_logits, w_gu, w_dn, K, variant="tiled")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.moe_mlp(x, static_logits, w_gu, w_dn, K,
                                 variant="tiled")
    for name in ("empty", "pair", "tight", "balanced"):
        static_logits.copy_(sets[name].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager[name]), name


def test_engine_prefill_matches_sparse(dev):
    """B S K = 512 = 128 E: the grouped prefill takes the tiled kernels."""
    from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

    assert ops.moe_variant(
        256, TINY_MOE.top_k, TINY_MOE.num_experts) == "tiled"
    kw = dict(max_batch=2, max_seq=128, seed=13)
    grouped = MixtralDecodeModel(TINY_MOE, moe_impl="grouped", **kw)
    sparse = MixtralDecodeModel(TINY_MOE, moe_impl="sparse", **kw)
    tokens = torch.randint(0, TINY_MOE.vocab_size, (2, 128), device=dev)
    torch.testing.assert_close(grouped.prefill(tokens).float(),
                               sparse.prefill(tokens).float(),
                               atol=0.5, rtol=0.1)
