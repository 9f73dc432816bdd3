"""The routed-MoE kernels (csrc/moe.hip) against the float64 oracle of
moe_oracle.py: bit-exact probe and integer families, derived bounds with no
absolute floor, literal split counts, determinism, composition, graph
replay with fresh routing and the bindings' rejections.
test_moe_oracle_cpu.py proves on an emulation that these cases reject a
subtly wrong kernel.
"""
import pytest
import torch

import moe_oracle as mo
from moe_oracle import BF16
from wva_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(family, ratio, note=""):
    print(f"\n[moe-gpu] family={family} ratio={ratio:.3f} {note}")


def on(dev, *tensors):
    return [t.to(dev) for t in tensors]


def gate_up(dev, r, x, w):
    out = ops.moe_gate_up_swiglu(*on(dev, x, w, r.offsets, r.slots), r.K)
    assert out.dtype == BF16 and out.shape == (r.TK, w.shape[1] // 2)
    return out.cpu()


def down(dev, r, act, w, topk_w, splits):
    """One down + combine call. Asserts the literal split count, and first
    leaves stale NaN (best effort, nothing depends on it) where the
    caching allocator will put the workspace."""
    H, I = w.shape[1], w.shape[2]
    assert ops.moe_down_num_splits(r.T, r.K, r.E, H, I) == splits
    args = on(dev, act, w, topk_w, r.offsets, r.slots)
    prime = torch.full((splits * r.TK * H,), float("nan"), device=dev,
                       dtype=torch.float32)
    del prime
    out = ops.moe_down_combine(*args)
    assert out.dtype == BF16 and out.shape == (r.T, H)
    return out.cpu()


# --------------------------------------------------------------------------
# gate_up + SwiGLU
# --------------------------------------------------------------------------

class TestGateUp:
    @pytest.mark.parametrize("I", mo.PROBE_I)
    @pytest.mark.parametrize("H", mo.PROBE_H)
    def test_probe(self, dev, H, I):
        c = mo.gate_up_probe_case(H, I)
        w = c.w.to(dev)
        for launch in range(c.launches):
            out = gate_up(dev, c.r, mo.gate_up_probe_x(c, launch), w)
            mo.assert_equal(out, mo.gate_up_probe_expected(c, launch),
                            f"gate_up probe H={H} I={I} launch {launch}")

    @pytest.mark.parametrize("I", mo.INT_I)
    @pytest.mark.parametrize("name", mo.MAIN_ROUTINGS)
    def test_integer(self, dev, name, I):
        c = mo.gate_up_integer_case(name, I)
        out = gate_up(dev, c.r, c.x, c.w)
        w = mo.assert_within(out, c.ref, c.bound, f"integer {name} I={I}")
        record(f"gate_up integer {name} I={I}", w)

    def test_saturation(self, dev):
        c = mo.gate_up_saturation_case()
        mo.check_saturation(gate_up(dev, c.r, c.x, c.w), c)

    def test_bounded(self, dev):
        c = mo.gate_up_bounded_case()
        out = gate_up(dev, c.r, c.x, c.w)
        record("gate_up bounded",
               mo.assert_within(out, c.ref, c.bound, "gate_up bounded"))


# --------------------------------------------------------------------------
# down + combine
# --------------------------------------------------------------------------

class TestDown:
    def test_split_table(self, dev):
        """The literals, the binding and the port agree."""
        for (T, K, E, H, I), n in mo.SPLIT_TABLE.items():
            assert ops.moe_down_num_splits(T, K, E, H, I) == n, (T, K, E, H, I)
            assert mo.down_num_splits(T * K, E, H, I) == n
        for table in (mo.DOWN_PROBE, mo.DOWN_INTEGER, mo.DOWN_BOUNDED,
                      mo.DOWN_CANCEL):
            for key, n in table.items():
                assert ops.moe_down_num_splits(*mo.table_key(*key)) == n, key

    @pytest.mark.parametrize("key", list(mo.DOWN_PROBE))
    def test_probe(self, dev, key):
        c = mo.down_probe_case(*key)
        assert c.launches <= 16
        w = c.w.to(dev)
        for launch in range(c.launches):
            act, topk_w = mo.down_probe_inputs(c, launch)
            out = down(dev, c.r, act, w, topk_w, mo.DOWN_PROBE[key])
            mo.assert_equal(out, mo.down_probe_expected(c, launch),
                            f"down probe {key} launch {launch}")

    @pytest.mark.parametrize("key", list(mo.DOWN_INTEGER))
    def test_integer(self, dev, key):
        c = mo.down_integer_case(*key)
        out = down(dev, c.r, c.act, c.w, c.topk_w, mo.DOWN_INTEGER[key])
        mo.assert_equal(out, c.expect, f"down integer {key}")

    @pytest.mark.parametrize("key", list(mo.DOWN_BOUNDED))
    def test_bounded(self, dev, key):
        c = mo.down_bounded_case(*key)
        out = down(dev, c.r, c.act, c.w, c.topk_w, mo.DOWN_BOUNDED[key])
        record(f"down bounded {key}",
               mo.assert_within(out, c.ref, c.bound, f"down bounded {key}"))

    @pytest.mark.parametrize("key", list(mo.DOWN_CANCEL))
    def test_cancel(self, dev, key):
        c = mo.down_cancel_case(*key)
        out = down(dev, c.r, c.act, c.w, c.topk_w, mo.DOWN_CANCEL[key])
        record(f"down cancel {key}",
               mo.assert_within(out, c.ref, c.bound, f"down cancel {key}"))

    @pytest.mark.parametrize("key", mo.DETERMINISM)
    def test_two_calls_are_bit_equal(self, dev, key):
        """At 8 splits, once on EDGE_A and once on the bound-tight grid."""
        name, H, I = key
        c = mo.down_bounded_case(*key)
        w = c.w.to(dev)
        first = down(dev, c.r, c.act, w, c.topk_w, 8)
        second = down(dev, c.r, c.act, w, c.topk_w, 8)
        mo.assert_within(first, c.ref, c.bound, f"determinism {key}")
        assert torch.equal(first, second)


# --------------------------------------------------------------------------
# route
# --------------------------------------------------------------------------

class TestRoute:
    @pytest.mark.parametrize("T,E,K", mo.ROUTE_SHAPES)
    def test_matches_oracle(self, dev, T, E, K):
        worst = 0.0
        for kind in mo.ROUTE_KINDS:
            logits = mo.route_logits(T, E, K, kind)
            if logits is None:
                continue
            out = ops.moe_route(logits.to(dev), K)
            worst = max(worst, mo.check_route(out, logits, K,
                                              f"{kind} {T, E, K}"))
        record(f"route {T, E, K}", worst)

    def test_weights_far_apart(self, dev):
        """Tie-free logits with gaps up to 60: weights down to e^-60 are
        held to the same relative bound (atol = 1e-6 would accept
        anything below it)."""
        g = torch.Generator().manual_seed(9)
        logits = torch.stack([
            (-7.5 * torch.arange(8, dtype=torch.float32))[
                torch.randperm(8, generator=g)] for _ in range(67)])
        logits = logits + torch.randn(67, 8, generator=g)
        out = ops.moe_route(logits.to(dev), 8)
        record("route wide gaps", mo.check_route(out, logits, 8, "wide"))


# --------------------------------------------------------------------------
# composition, graph replay, bindings
# --------------------------------------------------------------------------

GRAPH_T, GRAPH_E, GRAPH_K, GRAPH_H, GRAPH_I = 130, 4, 2, 384, 256


def graph_logit_sets():
    """Four routings of T = 130 over E = 4, K = 2: balanced (seeded pairs),
    expert 1 empty, everything to the pair (2, 0), and per-expert counts
    (65, 65, 65, 65), which fill the static tile grid."""
    g = torch.Generator().manual_seed(3)
    pairs = []
    for _ in range(GRAPH_T):
        a, b = torch.randperm(GRAPH_E, generator=g)[:2].tolist()
        pairs.append((a, b))
    no1 = [(0, 2), (2, 3), (3, 0)]
    sets = {
        "balanced": pairs,
        "empty": [no1[t % 3] for t in range(GRAPH_T)],
        "pair": [(2, 0)] * GRAPH_T,
        "tight": [(0, 1) if t < 65 else (2, 3) for t in range(GRAPH_T)],
    }
    out = {}
    for i, (name, p) in enumerate(sets.items()):
        out[name] = mo.counts_logits(p, GRAPH_E, seed=i)
    _, _, offs, _ = ops.moe_route_ref(out["tight"], GRAPH_K)
    assert offs.tolist() == [0, 65, 130, 195, 260]
    _, _, offs, _ = ops.moe_route_ref(out["empty"], GRAPH_K)
    assert int(offs[1]) == int(offs[2])
    _, _, offs, _ = ops.moe_route_ref(out["pair"], GRAPH_K)
    assert offs.tolist() == [0, 130, 130, 260, 260]
    return out


@pytest.fixture(scope="module")
def mlp(dev):
    g = torch.Generator().manual_seed(41)
    x = torch.randn(GRAPH_T, GRAPH_H, generator=g).to(BF16)
    w_gu = (torch.randn(GRAPH_E, 2 * GRAPH_I, GRAPH_H, generator=g)
            / GRAPH_H ** 0.5).to(BF16)
    w_dn = (torch.randn(GRAPH_E, GRAPH_H, GRAPH_I, generator=g)
            / GRAPH_I ** 0.5).to(BF16)
    return x.to(dev), w_gu.to(dev), w_dn.to(dev), graph_logit_sets()


def staged(x, logits, w_gu, w_dn, K):
    route = ops.moe_route(logits, K)
    _, topk_w, offsets, slots = route
    act = ops.moe_gate_up_swiglu(x, w_gu, offsets, slots, K)
    return ops.moe_down_combine(act, w_dn, topk_w, offsets, slots), route


def test_mlp_is_the_three_staged_ops(dev, mlp):
    x, w_gu, w_dn, sets = mlp
    for name, logits in sets.items():
        lg = logits.to(dev)
        whole = ops.moe_mlp(x, lg, w_gu, w_dn, GRAPH_K)
        parts, route = staged(x, lg, w_gu, w_dn, GRAPH_K)
        assert torch.equal(whole, parts), name
        mo.check_route(route, logits, GRAPH_K, name)
        # and the staged result is right: the down bound on the kernel's act
        _, topk_w, offsets, slots = [t.cpu() for t in route]
        r = mo.SimpleNamespace(
            T=GRAPH_T, K=GRAPH_K, E=GRAPH_E, TK=GRAPH_T * GRAPH_K,
            offsets=offsets, slots=slots,
            expert_of_pos=torch.repeat_interleave(
                torch.arange(GRAPH_E), (offsets[1:] - offsets[:-1]).long()),
            pos_of_slot=torch.argsort(slots.long()))
        act = ops.moe_gate_up_swiglu(x, w_gu, route[2], route[3], GRAPH_K)
        ref, absref = mo.down_ref64(act.cpu(), w_dn.cpu(), topk_w, r)
        mo.assert_within(whole.cpu(), ref,
                         mo.down_bound(ref, absref, GRAPH_I, GRAPH_K), name)


def test_graph_replays_with_fresh_routing(dev, mlp):
    """moe.hip's header: routing lives in device tensors the kernels read
    at execution time, so a captured step replays with fresh routing.
    Capture on the balanced routing, then replay on all four; the last
    fills the tile grid, which the captured routing did not."""
    x, w_gu, w_dn, sets = mlp
    eager = {}
    for name, logits in sets.items():
        lg = logits.to(dev)
        eager[name] = ops.moe_mlp(x, lg, w_gu, w_dn, GRAPH_K).clone()
        mo.check_route(ops.moe_route(lg, GRAPH_K), logits, GRAPH_K, name)
    assert not torch.equal(eager["balanced"], eager["tight"])
    static_x = x.clone()
    static_logits = sets["balanced"].to(dev).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.moe_mlp(static_x, static_logits, w_gu, w_dn, GRAPH_K)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.moe_mlp(static_x, static_logits, w_gu, w_dn, GRAPH_K)
    for name in ("balanced", "empty", "pair", "tight", "balanced"):
        static_logits.copy_(sets[name].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager[name]), name


def test_bindings_reject_and_a_correct_call_still_works(dev):
    c = mo.down_integer_case("NSUB1_TILES", 16, 896)
    r = c.r
    g = mo.gate_up_integer_case("EDGE_A", 16)
    bf = dict(device=dev, dtype=BF16)
    offs, slots = r.offsets.to(dev), r.slots.to(dev)
    act, w, topk_w = on(dev, c.act, c.w, c.topk_w)
    bad_calls = [
        lambda: ops.moe_route(torch.zeros(0, 8, device=dev), 2),     # T = 0
        lambda: ops.moe_route(torch.zeros(4, 65, device=dev), 2),    # E = 65
        lambda: ops.moe_route(torch.zeros(4, 3, device=dev), 4),     # K > E
        lambda: ops.moe_gate_up_swiglu(                              # H % 128
            torch.zeros(r.T, 192, **bf), torch.zeros(r.E, 32, 192, **bf),
            offs, slots, r.K),
        lambda: ops.moe_gate_up_swiglu(                              # I % 16
            torch.zeros(r.T, 128, **bf), torch.zeros(r.E, 48, 128, **bf),
            offs, slots, r.K),
        lambda: ops.moe_down_combine(                                # H % 16
            act, torch.zeros(r.E, 24, 896, **bf), topk_w, offs, slots),
        lambda: ops.moe_down_combine(act, w, topk_w, offs[:-1].contiguous(),
                                     slots),             # offsets of length E
        lambda: ops.moe_down_combine(act, w, topk_w, offs, slots.long()),
        lambda: ops.moe_gate_up_swiglu(
            torch.zeros(r.T, 128, **bf), torch.zeros(r.E, 32, 128, **bf),
            offs, slots.long(), r.K),                           # int64 slots
    ]
    for call in bad_calls:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    mo.assert_equal(down(dev, r, c.act, c.w, c.topk_w, 1), c.expect,
                    "down after the rejections")
    mo.assert_within(gate_up(dev, g.r, g.x, g.w), g.ref, g.bound,
                     "gate_up after the rejections")
