"""GPU numerics tests for the routed-MoE kernels (csrc/moe.hip): routing,
grouped gate_up+SwiGLU, grouped down+combine, and the `grouped` engine
path (decode, hipGraph capture, prefill) against the fp32 references.
"""
import pytest
import torch

from wva_amd import ops

pytestmark = pytest.mark.gpu

# The GEMM outputs are rounded to bf16 exactly once from an fp32
# accumulator: rtol = 2^-7 is twice the bf16 round-to-nearest half-ulp,
# atol covers fp32 summation-order differences on O(1) outputs.
GEMM_TOL = dict(rtol=2.0 ** -7, atol=1e-3)

T_SET = [1, 17, 67, 130]   # rows per expert cross 16, 64 and the m-tile
ROUTINGS = ["balanced", "empty", "pair"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    # The GPU path must use the in-tree HIP extension — no fallback.
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def tie_free_logits(T, E, seed=0):
    """Rows are random permutations of 0.37·arange(E) plus a per-row
    constant: every pairwise gap is ≥ 0.37, so top-k has no ties."""
    g = torch.Generator().manual_seed(seed)
    base = 0.37 * torch.arange(E, dtype=torch.float32)
    rows = torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)])
    return rows + torch.randn(T, 1, generator=g)


def routed_logits(T, E, routing, seed=0):
    logits = tie_free_logits(T, E, seed)
    if routing == "empty":          # expert 1 never selected
        logits[:, 1] = -1e4
    elif routing == "pair":         # every token → experts (2, 0)
        logits[:, 2] += 100.0
        logits[:, 0] += 50.0
    return logits


def ref_routing(T, E, K, routing, dev, seed=0):
    """Routing from the reference, so the GEMM tests do not depend on the
    route kernel."""
    logits = routed_logits(T, E, routing, seed)
    _, w, offsets, slots = ops.moe_route_ref(logits, K)
    if routing == "empty":
        assert int(offsets[1]) == int(offsets[2])
    if routing == "pair":
        assert int(offsets[1]) == T and int(offsets[3]) == 2 * T
    return w.to(dev), offsets.to(dev), slots.to(dev)


class TestRouteKernel:
    def _check(self, logits, K, dev):
        ref = ops.moe_route_ref(logits, K)
        out = ops.moe_route(logits.to(dev), K)
        torch.cuda.synchronize()
        for name, o, r in zip(("topk_idx", "topk_w", "offsets", "slots"),
                              out, ref):
            assert o.dtype == r.dtype and o.shape == r.shape, name
            if r.dtype == torch.int32:
                assert torch.equal(o.cpu(), r), name
            else:
                torch.testing.assert_close(o.cpu(), r, atol=1e-6, rtol=0)
        return out

    @pytest.mark.parametrize("T,E,K", [
        (1, 8, 2), (67, 8, 2), (300, 4, 2), (130, 64, 8),
    ])
    def test_matches_reference(self, dev, T, E, K):
        self._check(tie_free_logits(T, E, seed=T + E), K, dev)

    def test_empty_expert(self, dev):
        logits = routed_logits(130, 8, "empty", seed=3)
        _, _, offsets, _ = self._check(logits, 2, dev)
        assert int(offsets[1]) == int(offsets[2])

    def test_all_tokens_one_pair(self, dev):
        logits = routed_logits(130, 8, "pair", seed=4)
        idx, _, offsets, _ = self._check(logits, 2, dev)
        assert idx.cpu().tolist() == [[2, 0]] * 130
        assert offsets.cpu().tolist() == [0, 130, 130, 260, 260, 260, 260,
                                          260, 260]

    def test_exact_tie_lowest_index_wins(self, dev):
        idx, w, _, _ = self._check(torch.zeros(5, 8), 2, dev)
        assert idx.cpu().tolist() == [[0, 1]] * 5

    def test_rejects_unsupported_shapes(self, dev):
        with pytest.raises(RuntimeError):
            ops.moe_route(torch.zeros(4, 65, device=dev), 2)
        with pytest.raises(RuntimeError):
            ops.moe_route(torch.zeros(4, 16, device=dev), 9)


class TestGateUpSwiglu:
    H, I, E, K = 256, 160, 4, 2   # I is not a multiple of the 64-wide N-tile

    @pytest.fixture(scope="class")
    def weights(self, dev):
        g = torch.Generator().manual_seed(21)
        w = torch.randn(self.E, 2 * self.I, self.H, generator=g) / self.H ** 0.5
        return w.to(torch.bfloat16).to(dev)

    @pytest.mark.parametrize("routing", ROUTINGS)
    @pytest.mark.parametrize("T", T_SET)
    def test_matches_reference(self, dev, weights, T, routing):
        g = torch.Generator().manual_seed(100 + T)
        x = torch.randn(T, self.H, generator=g).to(torch.bfloat16).to(dev)
        _, offsets, slots = ref_routing(T, self.E, self.K, routing, dev, T)
        out = ops.moe_gate_up_swiglu(x, weights, offsets, slots, self.K)
        assert out.dtype == torch.bfloat16
        assert out.shape == (T * self.K, self.I)
        ref = ops.moe_gate_up_swiglu_ref(
            x.cpu(), weights.cpu(), offsets.cpu(), slots.cpu(), self.K
        )
        torch.testing.assert_close(out.float().cpu(), ref, **GEMM_TOL)

    def test_rejects_bad_shapes(self, dev, weights):
        _, offsets, slots = ref_routing(4, self.E, self.K, "balanced", dev)
        x = torch.zeros(4, 192, device=dev, dtype=torch.bfloat16)
        w = torch.zeros(self.E, 2 * self.I, 192, device=dev,
                        dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):   # K-dim not a multiple of 128
            ops.moe_gate_up_swiglu(x, w, offsets, slots, self.K)


class TestDownCombine:
    H, E, K = 160, 4, 2

    @pytest.fixture(scope="class")
    def weights(self, dev):
        g = torch.Generator().manual_seed(22)
        return {
            inter: (torch.randn(self.E, self.H, inter, generator=g)
                    / inter ** 0.5).to(torch.bfloat16).to(dev)
            for inter in (256, 2048)
        }

    def _check(self, dev, w_down, T, routing):
        inter = w_down.shape[2]
        g = torch.Generator().manual_seed(200 + T)
        act = torch.randn(T * self.K, inter, generator=g).to(
            torch.bfloat16).to(dev)
        topk_w, offsets, slots = ref_routing(
            T, self.E, self.K, routing, dev, T
        )
        out = ops.moe_down_combine(act, w_down, topk_w, offsets, slots)
        again = ops.moe_down_combine(act, w_down, topk_w, offsets, slots)
        assert out.dtype == torch.bfloat16 and out.shape == (T, self.H)
        ref = ops.moe_down_combine_ref(
            act.cpu(), w_down.cpu(), topk_w.cpu(), offsets.cpu(), slots.cpu()
        )
        torch.testing.assert_close(out.float().cpu(), ref, **GEMM_TOL)
        assert torch.equal(out, again)   # fixed summation order

    @pytest.mark.parametrize("routing", ROUTINGS)
    @pytest.mark.parametrize("T", T_SET)
    def test_matches_reference(self, dev, weights, T, routing):
        self._check(dev, weights[256], T, routing)

    def test_split_k(self, dev, weights):
        assert ops.moe_down_num_splits(1, self.K, self.E, self.H, 2048) > 1
        self._check(dev, weights[2048], 1, "balanced")


def _copy_weights_to_cpu(cpu, gpu):
    cpu.embed = gpu.embed.cpu()
    cpu.lm_head = gpu.lm_head.cpu()
    cpu.final_norm = gpu.final_norm.cpu()
    for lc, lg in zip(cpu.layers, gpu.layers):
        for attr in ("input_norm", "post_attn_norm", "wqkv", "wo",
                     "w_router"):
            setattr(lc, attr, getattr(lg, attr).cpu())
        lc.set_expert_weights(
            lg.w_gate_up_stacked.cpu(), lg.w_down_stacked.cpu()
        )


class TestGroupedEngine:
    @pytest.mark.parametrize("B", [70, 3])
    def test_layer_matches_sparse(self, dev, B):
        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

        torch.manual_seed(B)
        m = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=16, seed=5)
        layer = m.layers[0]
        h2 = torch.randn(B, TINY_MOE.hidden_size, device=dev,
                         dtype=torch.bfloat16)
        logits = h2.float() @ layer.w_router.t().float()
        w, sel = torch.topk(logits, TINY_MOE.top_k, dim=-1)
        w = torch.softmax(w, dim=-1).to(h2.dtype)
        sparse = m._moe_mlp_sparse(layer, h2, w, sel)
        grouped = ops.moe_mlp(
            h2, logits, layer.w_gate_up_stacked, layer.w_down_stacked,
            TINY_MOE.top_k,
        )
        torch.testing.assert_close(
            grouped.float(), sparse.float(), atol=2e-2, rtol=2e-2
        )

    def test_decode_matches_cpu_reference(self, dev):
        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

        gpu = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=32, seed=7,
                                 moe_impl="grouped")
        cpu = MixtralDecodeModel(
            TINY_MOE, max_batch=2, max_seq=32, device="cpu", seed=7
        )
        _copy_weights_to_cpu(cpu, gpu)
        gpu.context_lens[:2] = 0
        cpu.context_lens[:2] = 0
        tokens = torch.randint(0, TINY_MOE.vocab_size, (2,))
        lg = gpu.decode_step(tokens.to(dev))
        lc = cpu.decode_step(tokens)
        torch.testing.assert_close(
            lg.float().cpu(), lc.float(), atol=0.5, rtol=0.1
        )

    def test_graph_capture_above_sparse_threshold(self, dev):
        """B=70 is past the dense path's limit; the sparse path syncs with
        the host per expert and cannot be captured — grouped can."""
        from wva_amd.calibration.graph import GraphedDecoder
        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

        B = 70
        model = MixtralDecodeModel(TINY_MOE, max_batch=B, max_seq=64, seed=3,
                                   moe_impl="grouped")
        tokens = torch.randint(0, TINY_MOE.vocab_size, (B,), device=dev)
        torch.manual_seed(0)
        model.reset(B, 8)
        eager = model.decode_step(tokens).clone()
        torch.manual_seed(0)
        dec = GraphedDecoder(model, batch=B, warmup_steps=2)
        dec.reset_to(B, 8)
        graphed = dec.decode_step(tokens).clone()
        torch.testing.assert_close(graphed.float(), eager.float(),
                                   atol=1e-2, rtol=1e-2)
        g2 = dec.decode_step(tokens).clone()
        assert not torch.equal(graphed, g2)  # position advanced
        assert torch.isfinite(g2.float()).all()

    def test_prefill_matches_sparse(self, dev):
        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

        kw = dict(max_batch=2, max_seq=32, seed=13)
        grouped = MixtralDecodeModel(TINY_MOE, moe_impl="grouped", **kw)
        sparse = MixtralDecodeModel(TINY_MOE, moe_impl="sparse", **kw)
        assert torch.equal(grouped.layers[1].w_down_stacked,
                           sparse.layers[1].w_down_stacked)
        tokens = torch.randint(0, TINY_MOE.vocab_size, (2, 24), device=dev)
        lg = grouped.prefill(tokens)
        ls = sparse.prefill(tokens)
        torch.testing.assert_close(lg.float(), ls.float(), atol=0.5, rtol=0.1)
