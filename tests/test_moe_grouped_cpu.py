"""Routed-MoE (grouped expert MLP) references and engine plumbing on CPU.

The fp32 references in wva_amd.ops are the numerics oracles for the HIP
kernels (tests/test_moe_grouped_gpu.py); here they are pinned against
plain torch and against the engine's existing sparse path.
"""
import pytest
import torch

from wva_amd import ops
from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel


def tie_free_logits(T, E, seed=0, device="cpu"):
    """Each row a random permutation of 0.37·arange(E) plus a per-row
    constant: every pairwise gap is ≥ 0.37, so top-k has no ties."""
    g = torch.Generator().manual_seed(seed)
    base = 0.37 * torch.arange(E, dtype=torch.float32)
    rows = torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)])
    rows = rows + torch.randn(T, 1, generator=g)
    return rows.to(device)


def torch_route(logits, K):
    """topk + softmax + stable sort, the plain-torch statement of routing."""
    E = logits.shape[1]
    vals, idx = torch.topk(logits, K, dim=-1)
    w = torch.softmax(vals, dim=-1)
    flat = idx.reshape(-1)
    order = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=E)
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    return idx, w, offsets, order


class TestRouteRef:
    @pytest.mark.parametrize("T", [1, 67])
    def test_matches_topk_softmax_stable_sort(self, T):
        E, K = 8, 2
        logits = tie_free_logits(T, E, seed=T)
        idx, w, offsets, slots = ops.moe_route_ref(logits, K)
        r_idx, r_w, r_off, r_slots = torch_route(logits, K)
        assert idx.dtype == torch.int32 and slots.dtype == torch.int32
        assert offsets.dtype == torch.int32 and w.dtype == torch.float32
        assert torch.equal(idx.long(), r_idx)
        assert torch.equal(offsets.long(), r_off)
        assert torch.equal(slots.long(), r_slots)
        torch.testing.assert_close(w, r_w, atol=1e-6, rtol=0)
        # CPU dispatch is the reference
        d_idx, _, d_off, d_slots = ops.moe_route(logits, K)
        assert torch.equal(d_idx, idx) and torch.equal(d_slots, slots)
        assert torch.equal(d_off, offsets)

    def test_empty_expert_group(self):
        T, E, K, dead = 67, 8, 2, 3
        logits = tie_free_logits(T, E, seed=5)
        logits[:, dead] = -1e4
        idx, w, offsets, slots = ops.moe_route_ref(logits, K)
        r_idx, r_w, r_off, r_slots = torch_route(logits, K)
        assert int(offsets[dead]) == int(offsets[dead + 1])
        assert int(offsets[0]) == 0 and int(offsets[E]) == T * K
        assert torch.equal(idx.long(), r_idx)
        assert torch.equal(offsets.long(), r_off)
        assert torch.equal(slots.long(), r_slots)

    def test_exact_tie_takes_lowest_index(self):
        logits = torch.zeros(3, 8)
        idx, w, _, _ = ops.moe_route_ref(logits, 2)
        assert idx.tolist() == [[0, 1]] * 3
        torch.testing.assert_close(w, torch.full((3, 2), 0.5))


class TestMlpRef:
    def test_matches_engine_sparse_path(self):
        torch.manual_seed(0)
        m = MixtralDecodeModel(TINY_MOE, max_batch=8, max_seq=32, device="cpu")
        h2 = torch.randn(8, TINY_MOE.hidden_size, dtype=torch.bfloat16)
        layer = m.layers[0]
        logits = h2.float() @ layer.w_router.t().float()
        w, sel = torch.topk(logits, TINY_MOE.top_k, dim=-1)
        w = torch.softmax(w, dim=-1).to(h2.dtype)
        sparse = m._moe_mlp_sparse(layer, h2, w, sel)
        ref = ops.moe_mlp_ref(
            h2, logits, layer.w_gate_up_stacked, layer.w_down_stacked,
            TINY_MOE.top_k,
        )
        assert ref.dtype == torch.float32
        # same tolerance as tests/test_emulator.py dense-vs-sparse
        torch.testing.assert_close(ref, sparse.float(), atol=3e-2, rtol=3e-2)
        # the composite op on CPU is the reference rounded to bf16
        out = ops.moe_mlp(
            h2, logits, layer.w_gate_up_stacked, layer.w_down_stacked,
            TINY_MOE.top_k,
        )
        assert out.dtype == torch.bfloat16
        assert torch.equal(out, ref.to(torch.bfloat16))


class TestEngineMoeImpl:
    def test_grouped_matches_auto(self):
        kw = dict(max_batch=2, max_seq=32, device="cpu", seed=11)
        auto = MixtralDecodeModel(TINY_MOE, **kw)
        grouped = MixtralDecodeModel(TINY_MOE, moe_impl="grouped", **kw)
        assert auto.moe_impl == "auto" and grouped.moe_impl == "grouped"
        torch.manual_seed(1)
        auto.reset(2, 8)
        for lg, la in zip(grouped.layers, auto.layers):
            assert torch.equal(lg.w_down_stacked, la.w_down_stacked)
        for li in range(TINY_MOE.num_layers):
            grouped.k_cache[li].copy_(auto.k_cache[li])
            grouped.v_cache[li].copy_(auto.v_cache[li])
        grouped.context_lens.copy_(auto.context_lens)
        tokens = torch.randint(0, TINY_MOE.vocab_size, (2,))
        la = auto.decode_step(tokens)
        lg = grouped.decode_step(tokens)
        # the two paths differ only in where bf16 rounding happens inside
        # the MLP (dense rounds the routing weights and each expert's y to
        # bf16, grouped keeps both fp32): a few bf16 ulps on O(1) values —
        # the file-wide bf16 tolerance of tests/test_ops_gpu.py
        torch.testing.assert_close(lg.float(), la.float(), atol=2e-2, rtol=2e-2)

    def test_bogus_impl_raises(self):
        with pytest.raises(ValueError):
            MixtralDecodeModel(
                TINY_MOE, max_batch=2, max_seq=16, device="cpu",
                moe_impl="bogus",
            )

    @pytest.mark.parametrize("B,expected", [(2, "dense"), (70, "sparse")])
    def test_auto_keeps_batch_threshold(self, monkeypatch, B, expected):
        m = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=16, device="cpu")
        calls = []

        def fake(name):
            def run(layer, h2, weights, selected):
                calls.append(name)
                return torch.zeros_like(h2)
            return run

        monkeypatch.setattr(m, "_moe_mlp_dense", fake("dense"))
        monkeypatch.setattr(m, "_moe_mlp_sparse", fake("sparse"))
        h2 = torch.randn(B, TINY_MOE.hidden_size, dtype=torch.bfloat16)
        m._moe_mlp(m.layers[0], h2)
        assert calls == [expected]

    @pytest.mark.parametrize("impl", ["dense", "sparse"])
    def test_forced_impl_ignores_batch(self, monkeypatch, impl):
        m = MixtralDecodeModel(
            TINY_MOE, max_batch=2, max_seq=16, device="cpu", moe_impl=impl
        )
        calls = []
        for name in ("dense", "sparse"):
            monkeypatch.setattr(
                m, f"_moe_mlp_{name}",
                lambda layer, h2, w, s, name=name: (
                    calls.append(name), torch.zeros_like(h2))[1],
            )
        for B in (2, 70):
            h2 = torch.randn(B, TINY_MOE.hidden_size, dtype=torch.bfloat16)
            m._moe_mlp(m.layers[0], h2)
        assert calls == [impl, impl]
