"""CPU tests of the fp32 reference ops (shape/semantics sanity: these are
the ground truth that the GPU kernels are compared against)."""
import math

import torch

from wva_amd import ops


class TestReferenceOps:
    def test_rmsnorm_unit_weight_norms(self):
        x = torch.randn(4, 64)
        w = torch.ones(64)
        out, _ = ops.rmsnorm_ref(x, w, None, 0.0)
        rms = out.pow(2).mean(dim=-1)
        torch.testing.assert_close(rms, torch.ones(4), atol=1e-5, rtol=1e-5)

    def test_rmsnorm_residual_fold(self):
        x = torch.randn(2, 8)
        r = torch.randn(2, 8)
        _, folded = ops.rmsnorm_ref(x, torch.ones(8), r)
        torch.testing.assert_close(folded, x + r)

    def test_rope_preserves_norm(self):
        q = torch.randn(3, 2, 128)
        k = torch.randn(3, 1, 128)
        pos = torch.tensor([0, 5, 100])
        qr, kr = ops.rope_ref(q, k, pos)
        # rotation preserves the norm of each (x1, x2) pair
        torch.testing.assert_close(
            qr.norm(dim=-1), q.float().norm(dim=-1), atol=1e-4, rtol=1e-4
        )

    def test_silu_mul(self):
        g = torch.tensor([[0.0, 1.0]])
        u = torch.tensor([[3.0, 2.0]])
        out = ops.silu_mul_ref(g, u)
        assert out[0, 0] == 0.0
        expected = 1.0 / (1.0 + math.exp(-1.0)) * 2.0
        assert abs(out[0, 1].item() - expected) < 1e-6

    def test_attention_uniform_v(self):
        # all V rows identical → output equals that row regardless of scores
        B, S, Hk, Hq, D = 1, 16, 2, 4, 128
        q = torch.randn(B, Hq, D)
        k = torch.randn(B, Hk, S, D)
        v = torch.ones(B, Hk, S, D) * 0.5
        lens = torch.tensor([10], dtype=torch.int32)
        out = ops.gqa_decode_attn_ref(q, k, v, lens, 1.0 / math.sqrt(D))
        torch.testing.assert_close(
            out, torch.full((B, Hq, D), 0.5), atol=1e-5, rtol=1e-5
        )

    def test_attention_respects_context_len(self):
        B, S, Hk, Hq, D = 1, 8, 1, 1, 128
        q = torch.zeros(B, Hq, D)
        q[0, 0, 0] = 10.0
        k = torch.zeros(B, Hk, S, D)
        v = torch.zeros(B, Hk, S, D)
        # position 5 (beyond ctx=4) has huge value — must not leak
        k[0, 0, 5, 0] = 100.0
        v[0, 0, 5, :] = 999.0
        lens = torch.tensor([4], dtype=torch.int32)
        out = ops.gqa_decode_attn_ref(q, k, v, lens, 1.0)
        assert out.abs().max() < 1.0

    def test_cpu_dispatch_uses_reference(self):
        x = torch.randn(2, 64, dtype=torch.bfloat16)
        w = torch.ones(64, dtype=torch.bfloat16)
        out = ops.rmsnorm(x, w)
        assert out.dtype == torch.bfloat16

    def test_skinny_linear_cpu_is_the_float32_matmul(self):
        """bf16 and weight-only fp8 (w_scale): the float32 matmul, rounded
        once to x's dtype."""
        torch.manual_seed(4)
        x = torch.randn(5, 256, dtype=torch.bfloat16)
        w = (torch.randn(48, 256) * 0.05).to(torch.bfloat16)
        y = ops.skinny_linear(x, w)
        assert y.dtype == torch.bfloat16 and y.shape == (5, 48)
        assert torch.equal(y, (x.float() @ w.float().t()).to(torch.bfloat16))

        scale = (w.float().abs().amax(dim=1) / 448.0).clamp_min(1e-12)
        w8 = (w.float() / scale[:, None]).to(torch.float8_e4m3fn)
        y8 = ops.skinny_linear(x, w8, scale)
        ref8 = x.float() @ (w8.float() * scale[:, None]).t()
        assert torch.equal(y8, ref8.to(torch.bfloat16))

    def test_fit_itl_curve(self):
        from wva_amd.calibration.itl_benchmark import fit_itl_curve

        # perfect linear data
        alpha, beta, r2 = fit_itl_curve([1, 2, 4, 8], [10.5, 11.0, 12.0, 14.0])
        assert abs(alpha - 10.0) < 1e-9
        assert abs(beta - 0.5) < 1e-9
        assert r2 > 0.999

    def test_kv_capacity_288gb(self):
        from wva_amd.calibration.itl_benchmark import derive_kv_capacity
        from wva_amd.calibration.model import LLAMA_3_8B

        hbm = 288 * 1024**3
        blocks, tokens = derive_kv_capacity(LLAMA_3_8B, hbm_bytes=hbm)
        # 8B bf16 weights ≈ 16 GB + embeddings; KV/token = 2*32*1024*2 = 128 KiB
        # → ≈ (0.9*288GB − ~18GB) / 128KiB ≈ 1.9M tokens
        assert 1_500_000 < tokens < 2_200_000
        assert blocks == tokens // 16


class TestMoEReference:
    def test_router_top2_weights_normalized(self):
        import torch
        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

        m = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=16, device="cpu")
        h2 = torch.randn(2, TINY_MOE.hidden_size, dtype=torch.bfloat16)
        out = m._moe_mlp(m.layers[0], h2)
        assert out.shape == h2.shape
        assert torch.isfinite(out.float()).all()

    def test_weight_bytes_mixtral_fits_mi355x(self):
        from wva_amd.calibration.moe_model import MIXTRAL_8X7B

        gb = MIXTRAL_8X7B.weight_bytes() / 2**30
        # Mixtral-8x7B ≈ 47B params ≈ 87-94 GiB bf16: resident on 288 GB
        # MI355X, NOT on 192 GB MI300X together with a useful KV budget
        assert 80 < gb < 100


class TestPrefill:
    def test_prefill_matches_stepwise_decode(self):
        """prefill(S tokens) must equal decoding the same tokens one by
        one from an empty cache — same math, different schedule."""
        import torch

        from wva_amd.calibration.model import TINY, LlamaDecodeModel

        torch.manual_seed(3)
        m1 = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                              seed=9)
        m2 = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                              seed=9)
        S = 7
        tokens = torch.randint(0, TINY.vocab_size, (2, S))

        logits_pre = m1.prefill(tokens)

        m2.context_lens.zero_()
        for s in range(S):
            logits_step = m2.decode_step(tokens[:, s])

        torch.testing.assert_close(
            logits_pre.float(), logits_step.float(), atol=5e-2, rtol=5e-2
        )
        assert int(m1.context_lens[0]) == S
        # KV caches agree too
        torch.testing.assert_close(
            m1.k_cache[0][:2, :, :S].float(),
            m2.k_cache[0][:2, :, :S].float(), atol=5e-2, rtol=5e-2,
        )

    def test_prefill_then_decode_continues(self):
        import torch

        from wva_amd.calibration.model import TINY, LlamaDecodeModel

        m = LlamaDecodeModel(TINY, max_batch=1, max_seq=32, device="cpu")
        tokens = torch.randint(0, TINY.vocab_size, (1, 5))
        m.prefill(tokens)
        nxt = torch.randint(0, TINY.vocab_size, (1,))
        logits = m.decode_step(nxt)
        assert logits.shape == (1, TINY.vocab_size)
        assert int(m.context_lens[0]) == 6
        assert torch.isfinite(logits.float()).all()


class TestMoEPrefill:
    def test_moe_prefill_matches_stepwise(self):
        import torch

        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel

        torch.manual_seed(4)
        m1 = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=32,
                                device="cpu", seed=5)
        m2 = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=32,
                                device="cpu", seed=5)
        S = 6
        tokens = torch.randint(0, TINY_MOE.vocab_size, (2, S))
        logits_pre = m1.prefill(tokens)
        m2.context_lens.zero_()
        for s in range(S):
            logits_step = m2.decode_step(tokens[:, s])
        torch.testing.assert_close(
            logits_pre.float(), logits_step.float(), atol=6e-2, rtol=6e-2
        )


class TestFp8KvCpu:
    def test_fp8_cache_decode_close_to_bf16(self):
        import torch

        from wva_amd.calibration.model import TINY, LlamaDecodeModel

        torch.manual_seed(0)
        m_bf = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                                seed=7)
        torch.manual_seed(0)
        m_f8 = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                                seed=7, kv_dtype="fp8")
        assert m_f8.k_cache[0].dtype == torch.float8_e4m3fn
        m_bf.context_lens.zero_()
        m_f8.context_lens.zero_()
        t = torch.randint(0, TINY.vocab_size, (2,))
        for _ in range(4):
            lb = m_bf.decode_step(t)
            lf = m_f8.decode_step(t)
        rel = (lb.float() - lf.float()).abs().max() / lb.float().abs().max()
        assert float(rel) < 0.15  # e4m3 quantization noise only

    def test_fp8_capacity_doubles(self):
        from wva_amd.calibration.itl_benchmark import derive_kv_capacity
        from wva_amd.calibration.model import LLAMA_3_8B

        hbm = 288 * 2 ** 30
        _, bf16_tokens = derive_kv_capacity(LLAMA_3_8B, hbm_bytes=hbm)
        _, fp8_tokens = derive_kv_capacity(
            LLAMA_3_8B, hbm_bytes=hbm, kv_dtype_bytes=1
        )
        assert abs(fp8_tokens - 2 * bf16_tokens) < 32

    def test_fp8_prefill_raises(self):
        import pytest as _pytest
        import torch

        from wva_amd.calibration.model import TINY, LlamaDecodeModel

        m = LlamaDecodeModel(TINY, max_batch=1, max_seq=32, device="cpu",
                             kv_dtype="fp8")
        # CPU prefill uses the matmul path and works (float upcast);
        # the GPU guard is exercised in the gpu suite
        t = torch.randint(0, TINY.vocab_size, (1, 4))
        logits = m.prefill(t)
        assert torch.isfinite(logits.float()).all()

    def test_fp8_moe_and_tp_engines(self):
        import torch

        from wva_amd.calibration.moe_model import TINY_MOE, MixtralDecodeModel
        from wva_amd.calibration.tp_model import TPLlamaDecodeModel
        from wva_amd.calibration.model import TINY

        moe = MixtralDecodeModel(TINY_MOE, max_batch=2, max_seq=32,
                                 device="cpu", kv_dtype="fp8")
        assert moe.k_cache[0].dtype == torch.float8_e4m3fn
        moe.reset(2, 8)
        out = moe.decode_step(torch.randint(0, TINY_MOE.vocab_size, (2,)))
        assert torch.isfinite(out.float()).all()

        tp = TPLlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                                kv_dtype="fp8")
        assert tp.k_cache[0].dtype == torch.float8_e4m3fn
        tp.reset(2, 8)
        out = tp.decode_step(torch.randint(0, TINY.vocab_size, (2,)))
        assert torch.isfinite(out.float()).all()

    def test_fp8_weights_decode_close_to_bf16(self):
        import torch

        from wva_amd.calibration.model import TINY, LlamaDecodeModel

        torch.manual_seed(0)
        m_bf = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                                seed=7)
        torch.manual_seed(0)
        m_q = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                               seed=7, weights_dtype="fp8")
        assert m_q.lm_head is None and m_q.lm_head_q[0].dtype == \
            torch.float8_e4m3fn
        m_bf.context_lens.zero_()
        m_q.context_lens.zero_()
        t = torch.randint(0, TINY.vocab_size, (2,))
        for _ in range(3):
            lb = m_bf.decode_step(t)
            lq = m_q.decode_step(t)
        rel = (lb.float() - lq.float()).abs().max() / lb.float().abs().max()
        assert float(rel) < 0.25  # W8A8 per-tensor quantization noise
