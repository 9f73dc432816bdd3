"""Weight-only fp8 (e4m3) expert weights of the routed MoE, the parts that
need no GPU: the quantiser, the scaled references behind the public ops, the
refusal of the tiled kernels and the fp8-weight Mixtral engine.
"""
import pytest
import torch

from moe_oracle import BF16
from wva_amd import ops
from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

FP8 = torch.float8_e4m3fn


def test_quantize_moe_weights():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(3, 5, 64, generator=g).to(BF16)
    w[1, 2] = 0                                  # an all-zero row
    w[2, 4, 7] = 1e9                             # far past e4m3's 448
    q, scale = ops.quantize_moe_weights(w)
    assert q.dtype == FP8 and q.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (3, 5)
    qf = q.float()
    assert bool(torch.isfinite(qf).all())
    top = w.float().abs().argmax(-1, keepdim=True)   # the row amax -> +-448
    assert torch.equal(qf.gather(-1, top), 448 * w.float().gather(-1, top).sign())
    assert not qf[1, 2].any() and scale[1, 2] == 1
    # q0 · 2^e with amax(|q0|) = 448 in every row comes back exactly
    q0 = torch.randn(2, 4, 32, generator=g).to(FP8).float()
    q0[:, :, 0] = 448
    w0 = q0 * 2.0 ** torch.arange(-9, -1).reshape(2, 4, 1)
    q, scale = ops.quantize_moe_weights(w0)
    assert torch.equal(q.float() * scale[:, :, None], w0)


def test_public_ops_on_cpu_are_the_refs_on_dequantised_weights():
    T, E, K, H, I = 8, 4, 2, 256, 256
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, H, generator=g).to(BF16)
    logits = torch.randn(T, E, generator=g)
    q_gu, s_gu = ops.quantize_moe_weights(
        torch.randn(E, 2 * I, H, generator=g) / H ** 0.5)
    q_dn, s_dn = ops.quantize_moe_weights(
        torch.randn(E, H, I, generator=g) / I ** 0.5)
    w_gu, w_dn = q_gu.float() * s_gu[:, :, None], q_dn.float() * s_dn[:, :, None]
    _, topk_w, offs, slots = ops.moe_route(logits, K)
    act = ops.moe_gate_up_swiglu(x, q_gu, offs, slots, K, w_scale=s_gu)
    assert torch.equal(
        act, ops.moe_gate_up_swiglu_ref(x, w_gu, offs, slots, K).to(BF16))
    out = ops.moe_down_combine(act, q_dn, topk_w, offs, slots, w_scale=s_dn)
    assert torch.equal(out, ops.moe_down_combine_ref(
        act, w_dn, topk_w, offs, slots).to(BF16))
    whole = ops.moe_mlp(x, logits, q_gu, q_dn, K, w_gate_up_scale=s_gu,
                        w_down_scale=s_dn)
    assert torch.equal(whole, out)
    assert torch.equal(whole, ops.moe_mlp_ref(x, logits, w_gu, w_dn, K).to(BF16))
    for call in (      # variant="tiled" with a scale
        lambda: ops.moe_gate_up_swiglu(x, q_gu, offs, slots, K, "tiled", s_gu),
        lambda: ops.moe_down_combine(act, q_dn, topk_w, offs, slots, "tiled",
                                     s_dn),
        lambda: ops.moe_mlp(x, logits, q_gu, w_dn.to(BF16), K, "tiled", s_gu),
    ):
        with pytest.raises(ValueError):
            call()


def test_engine_with_fp8_expert_weights():
    cfg = TINY_MOE
    E, H, I = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
    m = MixtralDecodeModel(cfg, max_batch=4, max_seq=16, device="cpu",
                           moe_impl="grouped", weights_dtype="fp8")
    layer = m.layers[1]
    for w, s, shape in (
            (layer.w_gate_up_stacked, layer.w_gate_up_scale, (E, 2 * I, H)),
            (layer.w_down_stacked, layer.w_down_scale, (E, H, I))):
        assert w.dtype == FP8 and w.shape == shape
        assert s.dtype == torch.float32 and s.shape == shape[:2]
    for name in ("w_gate_up_flat", "w_down_t", "w_gate_up", "w_down"):
        assert not hasattr(layer, name), name     # no bf16 expert copies
    h2 = torch.randn(5, H, generator=torch.Generator().manual_seed(3)).to(BF16)
    w_gu = layer.w_gate_up_stacked.float() * layer.w_gate_up_scale[:, :, None]
    w_dn = layer.w_down_stacked.float() * layer.w_down_scale[:, :, None]
    logits = h2.float() @ layer.w_router.t().float()
    want = ops.moe_mlp_ref(h2, logits, w_gu, w_dn, cfg.top_k).to(BF16)
    assert torch.equal(m._moe_mlp(layer, h2), want)
    m.reset(3, 4)
    out = m.decode_step(torch.tensor([1, 2, 3]))
    assert out.shape == (3, cfg.vocab_size)
    assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("kwargs", [
    dict(moe_impl="auto", weights_dtype="fp8"),
    dict(moe_impl="dense", weights_dtype="fp8"),
    dict(moe_impl="sparse", weights_dtype="fp8"),
    dict(moe_impl="grouped", weights_dtype="fp16"),
])
def test_engine_refuses(kwargs):
    with pytest.raises(ValueError):
        MixtralDecodeModel(TINY_MOE, max_batch=1, max_seq=8, device="cpu",
                           **kwargs)
