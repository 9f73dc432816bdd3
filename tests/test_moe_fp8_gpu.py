"""The streaming routed-MoE kernels with weight-only fp8 (e4m3) expert weights
(csrc/moe.hip, moe_*_fp8_kernel) against exact and float64 references, on the
routings, shapes and bounds of moe_oracle.py.
"""
import pytest
import torch

import moe_oracle as mo
from moe_oracle import BF16
from wva_amd import ops

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(family, ratio):
    print(f"\n[moe-fp8-gpu] family={family} ratio={ratio:.3f}")


def on(dev, *tensors):
    return [t.to(dev) for t in tensors]


def seeded_quant(shape, seed):
    """e4m3 weights [E, N, K], fp32 row scales in [0.5, 1.5) (no powers of 2)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g).to(FP8),
            0.5 + torch.rand(shape[:2], generator=g))


def pow2_quant(w):
    """(q, scale, q scale): e4m3 weights under the smallest power-of-two row
    scale that brings the row's amax to 448 or below, and their dequantised
    form, which is exact in float32."""
    scale = 2.0 ** torch.ceil(torch.log2(w.float().abs().amax(-1) / 448))
    q = (w.float() / scale[..., None]).to(FP8)
    return q, scale, q.float() * scale[..., None]


def gate_up(dev, r, x, q, scale):
    out = ops.moe_gate_up_swiglu(*on(dev, x, q, r.offsets, r.slots), r.K,
                                 w_scale=scale.to(dev))
    assert out.dtype == BF16 and out.shape == (r.TK, q.shape[1] // 2)
    return out.cpu()


def down(dev, r, act, q, scale, topk_w, splits):
    H, I = q.shape[1], q.shape[2]
    assert ops.moe_down_num_splits(r.T, r.K, r.E, H, I) == splits
    out = ops.moe_down_combine(*on(dev, act, q, topk_w, r.offsets, r.slots),
                               w_scale=scale.to(dev))
    assert out.dtype == BF16 and out.shape == (r.T, H)
    return out.cpu()


@pytest.mark.parametrize("I", mo.PROBE_I)
@pytest.mark.parametrize("H", mo.PROBE_H)
def test_gate_up_probe(dev, H, I):
    """One-hot x: act[p, n] = bf16(g fl32(s_u q_u)) at the one k of p's
    token, g = s_g q_g. Gate values {32, 64, 128} times gate scales {1, 2, 4}
    by row, not {0.5, 1, 2}: at g = 16, expf(-16) = 1.13e-7 is above half an
    ulp of 1 (2^-24 = 5.96e-8) and 1 + expf(-g) = 1 + 2^-23; at the smallest
    g here, 32, expf(-32) = 1.27e-14 < 2^-24, so 1 + expf(-g) == 1 and
    silu(g) = g in float32. g is a power of two: g u is exact."""
    c = mo.gate_up_probe_case(H, I)
    r = c.r
    g = torch.Generator().manual_seed(H + 3 * I)
    q_up, s_up = seeded_quant((r.E, I, H), seed=H * 5 + I)
    q_gate = torch.tensor([32.0, 64.0, 128.0])[
        torch.randint(0, 3, (r.E, I, H), generator=g)].to(FP8)
    s_gate = torch.tensor([1.0, 2.0, 4.0])[torch.arange(r.E * I) % 3]
    q = torch.cat([q_gate, q_up], dim=1).contiguous()
    scale = torch.cat([s_gate.reshape(r.E, I), s_up], dim=1).contiguous()
    tok = torch.div(r.slots.long(), r.K, rounding_mode="floor")
    for launch in range(c.launches):
        out = gate_up(dev, r, mo.gate_up_probe_x(c, launch), q, scale)
        k = (launch * r.T + tok) % H
        col = q.float()[r.expert_of_pos, :, k] * scale[r.expert_of_pos]
        mo.assert_equal(out, (col[:, :I] * col[:, I:]).to(BF16),
                        f"fp8 gate_up probe H={H} I={I} launch {launch}")


DOWN_PROBE = {**mo.DOWN_PROBE, ("NSUB1_TILES", 16, 896): 1}


def check_down_probe(dev, c, q, scale, launch, splits, what):
    """One-hot act and topk_w: out[t] = bf16(fl32(s[e, n] q[e, n, k]))."""
    r = c.r
    act, topk_w = mo.down_probe_inputs(c, launch)
    out = down(dev, r, act, q, scale, topk_w, splits)
    p = r.pos_of_slot[torch.arange(r.T) * r.K + launch % r.K]
    e = r.expert_of_pos[p]
    expect = q.float()[e, :, (launch * r.TK + p) % c.I] * scale[e]
    mo.assert_equal(out, expect.to(BF16), f"{what} launch {launch}")


@pytest.mark.parametrize("key", list(DOWN_PROBE))
def test_down_probe(dev, key):
    c = mo.down_probe_case(*key)
    q, scale = seeded_quant((c.r.E, c.H, c.I), seed=c.H + c.I)
    for launch in range(c.launches):
        check_down_probe(dev, c, q, scale, launch, DOWN_PROBE[key],
                         f"fp8 down probe {key}")


def test_gate_up_bounded(dev):
    c = mo.gate_up_bounded_case()
    q, scale, w = pow2_quant(c.w)
    ref, bound = mo.gate_up_bound(c.x, w, c.r)
    record("gate_up bounded", mo.assert_within(
        gate_up(dev, c.r, c.x, q, scale), ref, bound, "fp8 gate_up bounded"))


@pytest.mark.parametrize("key", list(mo.DOWN_BOUNDED))
def test_down_bounded(dev, key):
    c = mo.down_bounded_case(*key)
    q, scale, w = pow2_quant(c.w)
    ref, absref = mo.down_ref64(c.act, w, c.topk_w, c.r)
    out = down(dev, c.r, c.act, q, scale, c.topk_w, mo.DOWN_BOUNDED[key])
    record(f"down bounded {key}", mo.assert_within(
        out, ref, mo.down_bound(ref, absref, c.I, c.r.K),
        f"fp8 down bounded {key}"))


def test_mlp_is_the_staged_ops_and_replays_in_a_graph(dev):
    T, E, K, H, I = 8, 4, 2, 256, 256
    g = torch.Generator().manual_seed(6)
    x = torch.randn(T, H, generator=g).to(BF16).to(dev)
    q_gu, s_gu = on(dev, *seeded_quant((E, 2 * I, H), seed=7))
    q_dn, s_dn = on(dev, *seeded_quant((E, H, I), seed=8))
    s_gu, s_dn = s_gu / (448 * H ** 0.5), s_dn / (448 * I ** 0.5)
    logit_sets = [torch.randn(T, E, generator=g).to(dev) for _ in range(3)]

    def mlp(logits):
        return ops.moe_mlp(x, logits, q_gu, q_dn, K, w_gate_up_scale=s_gu,
                           w_down_scale=s_dn)

    eager = [mlp(lg).clone() for lg in logit_sets]
    assert not torch.equal(eager[0], eager[1])
    assert bool(torch.isfinite(eager[0].float()).all())
    _, topk_w, offsets, slots = ops.moe_route(logit_sets[0], K)
    act = ops.moe_gate_up_swiglu(x, q_gu, offsets, slots, K, w_scale=s_gu)
    assert torch.equal(eager[0], ops.moe_down_combine(
        act, q_dn, topk_w, offsets, slots, w_scale=s_dn))
    assert torch.equal(eager[0], mlp(logit_sets[0]))
    static_logits = logit_sets[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            mlp(static_logits)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = mlp(static_logits)
    for i in (0, 1, 2, 0):
        static_logits.copy_(logit_sets[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager[i]), i


def test_bindings_reject_and_a_correct_call_still_works(dev):
    c = mo.down_probe_case("NSUB1_TILES", 16, 896)
    r = c.r
    q, scale = seeded_quant((r.E, c.H, c.I), seed=9)
    act, topk_w = mo.down_probe_inputs(c, 0)
    ad, qd, sd, tw, offs, slots = on(dev, act, q, scale, topk_w, r.offsets,
                                     r.slots)
    x = torch.zeros(r.T, 128, device=dev, dtype=BF16)
    q_gu, s_gu = on(dev, *seeded_quant((r.E, 32, 128), seed=10))

    def gu(w, s):
        return ops.moe_gate_up_swiglu(x, w, offs, slots, r.K, w_scale=s)

    def dn(w, s):
        return ops.moe_down_combine(ad, w, tw, offs, slots, w_scale=s)

    for call in (
        lambda: gu(q_gu, None), lambda: dn(qd, None),     # fp8, no scale
        lambda: gu(q_gu.to(BF16), s_gu), lambda: dn(qd.to(BF16), sd),
        lambda: gu(q_gu, s_gu[:, :16].contiguous()),      # [E, I]
        lambda: dn(qd, sd.t().contiguous()),              # [H, E]
        lambda: gu(q_gu, s_gu.to(BF16)), lambda: dn(qd, sd.double()),
    ):
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    check_down_probe(dev, c, q, scale, 0, 1, "down after the rejections")
