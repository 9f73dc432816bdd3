"""`variant` of the MoE ops on CPU tensors: validated, otherwise ignored
(the references have no variants)."""
import pytest
import torch

from wva_amd import ops


def test_variant_is_validated_and_ignored_on_cpu():
    g = torch.Generator().manual_seed(0)
    T, E, K, H, I = 6, 4, 2, 128, 128
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, generator=g)
    w_gu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).bfloat16()
    w_dn = (torch.randn(E, H, I, generator=g) / I ** 0.5).bfloat16()
    _, topk_w, offsets, slots = ops.moe_route(logits, K)
    act_ref = ops.moe_gate_up_swiglu_ref(x, w_gu, offsets, slots, K).bfloat16()
    out_ref = ops.moe_down_combine_ref(
        act_ref, w_dn, topk_w, offsets, slots).bfloat16()
    for variant in (None, "stream", "tiled"):
        act = ops.moe_gate_up_swiglu(x, w_gu, offsets, slots, K,
                                     variant=variant)
        assert torch.equal(act, act_ref)
        out = ops.moe_down_combine(act, w_dn, topk_w, offsets, slots,
                                   variant=variant)
        assert torch.equal(out, out_ref)
        assert torch.equal(
            ops.moe_mlp(x, logits, w_gu, w_dn, K, variant=variant), out_ref)
    for call in (
        lambda: ops.moe_gate_up_swiglu(x, w_gu, offsets, slots, K, "auto"),
        lambda: ops.moe_down_combine(act_ref, w_dn, topk_w, offsets, slots,
                                     variant="lds"),
        lambda: ops.moe_mlp(x, logits, w_gu, w_dn, K, variant=1),
    ):
        with pytest.raises(ValueError):
            call()
