"""GPU tests of the skinny GEMM (bf16 and e4m3 weights), RMSNorm and SwiGLU
kernels against the float64 oracles, derived bounds and adversarial cases of
dense_oracle.py: bit-exact probe and integer families, bounded randn
families with no absolute floor, and the binding's empty and rejected
inputs.

test_dense_ops_cpu.py shows on the CPU that these cases and bounds reject
the corresponding mutants. Every GEMM test asserts, through
ops.skinny_linear_num_splits, the literal split count it means to exercise.
Each bounded test prints its worst err/bound ratio (`-s` shows them;
docs/testing.md records them).
"""
import pytest
import torch

import dense_oracle as do
from dense_oracle import BF16, FP8
from wva_amd import ops

pytestmark = pytest.mark.gpu

FP8_MODES = [pytest.param(False, id="bf16"), pytest.param(True, id="fp8")]
FUSED = [pytest.param(False, id="flat"), pytest.param(True, id="fused")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_available(), "HIP extension _wva_ops not loaded"
    return torch.device("cuda:0")


def record(family, ratio, note=""):
    print(f"\n[dense-ops] family={family} ratio={ratio:.3f} {note}")


def to_dev(t, dev):
    """e4m3 tensors are moved as bytes."""
    if t is None:
        return None
    if t.dtype == FP8:
        return t.view(torch.uint8).to(dev).view(FP8)
    return t.to(dev)


def assert_splits(M, N, K, splits):
    assert ops.skinny_linear_num_splits(M, N, K) == splits, (
        f"the launch heuristic no longer splits ({M}, {N}, {K}) as the "
        "test assumes")


def gemm(c, dev, splits):
    """Run the skinny GEMM on case `c` after asserting its split count."""
    assert c.splits == splits
    assert_splits(c.M, c.N, c.K, splits)
    return ops.skinny_linear(to_dev(c.x, dev), to_dev(c.w, dev),
                             to_dev(c.scale, dev))


# --------------------------------------------------------------------------
# skinny GEMM
# --------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", FP8_MODES)
class TestSkinnyGemm:
    @pytest.mark.parametrize("K", list(do.PROBE_K))
    @pytest.mark.parametrize("M", do.PROBE_M)
    def test_probe_every_k(self, dev, M, K, fp8):
        """K / M launches, x row m one-hot at k = r M + m: y[m, n] must be
        w[n, k] (times its scale, rounded once) bit for bit, for every k of
        the shape and all 254 finite e4m3 codes."""
        c = do.probe_case(M, K, fp8)
        assert_splits(M, do.PROBE_N, K, do.PROBE_K[K])
        w, scale = to_dev(c.w, dev), to_dev(c.scale, dev)
        expect = c.expect.to(dev)
        x = torch.zeros(M, K, device=dev, dtype=BF16)
        rows = torch.arange(M, device=dev)
        bad = torch.zeros(c.launches, device=dev, dtype=torch.int64)
        for r in range(c.launches):
            cols = r * M + rows
            x[rows, cols] = 1
            y = ops.skinny_linear(x, w, scale)
            bad[r] = (y != expect[:, r * M:(r + 1) * M].t()).sum()
            x[rows, cols] = 0
        bad = bad.cpu()
        assert int(bad.sum()) == 0, (
            f"{int(bad.sum())} wrong elements in {int((bad > 0).sum())} of "
            f"{c.launches} launches, first launch {int(bad.nonzero()[0])}")

    @pytest.mark.parametrize("M", do.GEMM_M)
    def test_integer_edge_grid(self, dev, M, fp8):
        """Exact integer products over the whole M x N edge grid at K =
        1536 (4 splits): every tile edge of both instantiations, and for
        fp8 a per-row power-of-two scale that differs 16 rows on."""
        for N in do.GEMM_N:
            c = do.integer_case(M, N, do.EDGE_K, fp8)
            do.assert_equal(gemm(c, dev, do.EDGE_SPLITS), c.expect,
                            f"integer ({M}, {N}, {do.EDGE_K})")

    @pytest.mark.parametrize("M", do.SPLIT_M)
    def test_integer_split_table(self, dev, M, fp8):
        """Exact integer products at every split count: nonzeros at the
        first and last k of every split's range."""
        for K, splits in do.SPLIT_TABLE.items():
            c = do.integer_case(M, do.SPLIT_N, K, fp8)
            do.assert_equal(gemm(c, dev, splits), c.expect,
                            f"integer ({M}, {do.SPLIT_N}, {K})")
        c = do.integer_case(M, do.WIDE_N, do.WIDE_K, fp8)
        do.assert_equal(gemm(c, dev, do.WIDE_SPLITS[M]), c.expect,
                        f"integer ({M}, {do.WIDE_N}, {do.WIDE_K})")

    @pytest.mark.parametrize("shape", list(do.BOUNDED_SHAPES))
    def test_bounded_randn(self, dev, shape, fp8):
        c = do.bounded_case(*shape, fp8)
        out = gemm(c, dev, do.BOUNDED_SHAPES[shape])
        r = do.assert_within(out, c.ref, c.bound, f"bounded {shape}")
        record("gemm-bounded", r, f"shape={shape} fp8={fp8}")

    @pytest.mark.parametrize("shape", list(do.CANCEL_SHAPES))
    def test_bounded_cancelling(self, dev, shape, fp8):
        """Halves of K that nearly cancel: the partials are ~16x the
        result, so a partial or workspace kept in bf16 is several times the
        bound here."""
        c = do.cancel_case(*shape, fp8)
        out = gemm(c, dev, do.CANCEL_SHAPES[shape])
        r = do.assert_within(out, c.ref, c.bound, f"cancel {shape}")
        record("gemm-cancel", r, f"shape={shape} fp8={fp8}")

    def test_deterministic(self, dev, fp8):
        c = do.bounded_case(*do.DETERMINISM_SHAPE, fp8)
        a = gemm(c, dev, 16)
        b = gemm(c, dev, 16)
        assert torch.equal(a, b)


class TestSkinnyGemmBinding:
    def test_split_table_literals(self, dev):
        for K, n in {128: 1, 896: 1, 768: 2, 1536: 4, 3072: 8, 2048: 16,
                     2816: 2, 14336: 16}.items():
            for M in (1, 16, 17, 64):
                assert ops.skinny_linear_num_splits(M, 128, K) == n, (M, K)
        assert ops.skinny_linear_num_splits(16, 7232, 2048) == 8
        assert ops.skinny_linear_num_splits(17, 7232, 2048) == 16

    def test_rejections(self, dev):
        def t(*shape, dtype=BF16):
            return torch.zeros(*shape, device=dev, dtype=dtype)

        w8 = t(8, 128).to(FP8)
        with pytest.raises(RuntimeError, match="multiple of 128"):
            ops.skinny_linear(t(4, 130), t(8, 130))
        with pytest.raises(RuntimeError, match="M <= 64"):
            ops.skinny_linear(t(65, 128), t(8, 128))
        with pytest.raises(RuntimeError, match="K mismatch"):
            ops.skinny_linear(t(4, 128), t(8, 256))
        with pytest.raises(RuntimeError, match="w_scale"):
            ops.skinny_linear(t(4, 128), w8, t(7, dtype=torch.float32))
        with pytest.raises(RuntimeError, match="w_scale"):
            ops.skinny_linear(t(4, 128), w8, t(8))
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.skinny_linear(t(128, 4).t(), t(8, 128))
        with pytest.raises(RuntimeError):
            ops.skinny_linear_num_splits(65, 128, 128)
        with pytest.raises(RuntimeError):
            ops.skinny_linear_num_splits(4, 128, 130)
        torch.cuda.synchronize()

    def test_empty_inputs(self, dev):
        """M = 0 (a zero-sized merge grid under split-K), N = 0 and zero
        RMSNorm rows return empty outputs without a launch, and the next
        op works."""
        def t(*shape, dtype=BF16):
            return torch.zeros(*shape, device=dev, dtype=dtype)

        assert ops.skinny_linear_num_splits(0, 128, 2048) == 16
        f32 = torch.float32
        assert ops.skinny_linear(t(0, 2048), t(128, 2048)).shape == (0, 128)
        assert ops.skinny_linear(t(0, 128), t(128, 128)).shape == (0, 128)
        assert ops.skinny_linear(t(4, 2048), t(0, 2048)).shape == (4, 0)
        assert ops.skinny_linear(t(17, 2048), t(0, 2048)).shape == (17, 0)
        assert ops.skinny_linear(
            t(0, 2048), t(128, 2048).to(FP8), t(128, dtype=f32)
        ).shape == (0, 128)
        assert ops.skinny_linear(
            t(4, 2048), t(0, 2048).to(FP8), t(0, dtype=f32)
        ).shape == (4, 0)
        w = do.rms_weight(2048).to(dev)
        assert ops.rmsnorm(t(0, 2048), w).shape == (0, 2048)
        res = t(0, 2048)
        assert ops.rmsnorm(t(0, 2048), w, res).shape == (0, 2048)
        assert ops.rmsnorm(t(2, 0, 2048), w).shape == (2, 0, 2048)
        assert ops.silu_mul(t(0, 8), t(0, 8)).shape == (0, 8)
        assert ops.silu_mul_fused(t(0, 8)).shape == (0, 4)
        torch.cuda.synchronize()
        c = do.integer_case(16, 17, 768, False)
        do.assert_equal(gemm(c, dev, 2), c.expect, "GEMM after empties")
        cs = do.rms_sign_case(3, 16)
        out = ops.rmsnorm(cs.x.to(dev), cs.w.to(dev), None, cs.eps)
        ref, _ = do.rmsnorm_ref64(cs.x, cs.w, None, cs.eps)
        do.assert_within(out, ref, do.rel_bound(ref), "rmsnorm after empties")


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------

def run_rmsnorm(c, dev):
    """The kernel on case `c`, held to the bound. Fused: the stored
    residual must be the float32 sum rounded once, and the input and weight
    must come back bit for bit."""
    x, w = c.x.to(dev), c.w.to(dev)
    res = None if c.res is None else c.res.to(dev)
    out = ops.rmsnorm(x, w, res, c.eps)
    ref, stored = do.rmsnorm_ref64(c.x, c.w, c.res, c.eps)
    assert torch.equal(x.cpu(), c.x) and torch.equal(w.cpu(), c.w)
    if stored is not None:
        do.assert_equal(res, stored, "stored residual")
    return do.assert_within(out, ref, do.rel_bound(ref),
                            f"rmsnorm {tuple(c.x.shape)}")


@pytest.mark.parametrize("hidden", do.RMS_HIDDEN)
class TestRmsnorm:
    def test_spike_and_sign_census(self, dev, hidden):
        """One nonzero per row at the vector edges (every other output
        exactly 0), and +-2^(r mod 3) rows with an exact sum of squares."""
        for rows in do.RMS_ROWS:
            r = run_rmsnorm(do.rms_spike_case(rows, hidden), dev)
            record("rmsnorm-spike", r, f"rows={rows} hidden={hidden}")
            r = run_rmsnorm(do.rms_sign_case(rows, hidden), dev)
            record("rmsnorm-sign", r, f"rows={rows} hidden={hidden}")

    @pytest.mark.parametrize("eps", do.RMS_EPS)
    def test_eps(self, dev, hidden, eps):
        """Rows at 2^-30 (the output is x rsqrt(eps) w) and at 2^30."""
        for rows in do.RMS_ROWS:
            for e in (-30, 30):
                r = run_rmsnorm(do.rms_eps_case(rows, hidden, e, eps), dev)
                record("rmsnorm-eps", r,
                       f"rows={rows} hidden={hidden} 2^{e} eps={eps}")

    @pytest.mark.parametrize("kind", do.FUSED_KINDS)
    def test_fused_residual(self, dev, hidden, kind):
        for rows in do.RMS_ROWS:
            r = run_rmsnorm(do.rms_fused_case(kind, rows, hidden), dev)
            record("rmsnorm-fused-" + kind, r, f"rows={rows} hidden={hidden}")


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------

def run_silu(c, fused, dev):
    if fused:
        out = ops.silu_mul_fused(do.fuse(c).to(dev))
    else:
        out = ops.silu_mul(c.gate.to(dev), c.up.to(dev))
    assert out.shape == c.gate.shape
    return out.cpu()


@pytest.mark.parametrize("fused", FUSED)
class TestSilu:
    def test_gate_sweep(self, dev, fused):
        c = do.gate_sweep_case()
        ref = do.silu_ref64(c.gate, c.up)
        r = do.assert_within(run_silu(c, fused, dev), ref, do.rel_bound(ref),
                             "gate sweep")
        record("silu-sweep", r, f"fused={fused}")

    def test_saturation(self, dev, fused):
        """e^-g overflows (g = -100, -1000, -3.38e38) or underflows (g =
        1000): finite, below 2^-126 in the first three rows, exactly 1000
        in the last."""
        c = do.saturation_case()
        out = run_silu(c, fused, dev).float()
        assert not bool(torch.isnan(out).any())
        assert bool(torch.isfinite(out).all())
        assert float(out[:3].abs().max()) < 2.0 ** -126
        assert torch.equal(out[3], torch.full_like(out[3], 1000.0))

    def test_position_code(self, dev, fused):
        """g = 1, u hashed from (row, col): the small shapes, and one above
        the 2 097 152 pairs of the first grid pass."""
        big = do.POSITION_FUSED if fused else do.POSITION_FLAT
        for shape in do.POSITION_SHAPES + (big,):
            c = do.position_case(*shape)
            ref = do.silu_ref64(c.gate, c.up)
            r = do.assert_within(run_silu(c, fused, dev), ref,
                                 do.rel_bound(ref), f"position {shape}")
            record("silu-position", r, f"shape={shape} fused={fused}")


# --------------------------------------------------------------------------
# engine
# --------------------------------------------------------------------------

def test_fp8_weights_decode_matches_cpu_reference(dev):
    """TINY with fp8 weights: the GPU engine (every linear on
    skinny_gemm_kernel<*, true>) against the CPU engine holding the same
    weights and quantised pairs, from an empty cache at batch 2."""
    from wva_amd.calibration.model import TINY, LlamaDecodeModel

    # the down projection of the issue's table, as the engine launches it
    assert_splits(2, TINY.hidden_size, TINY.intermediate_size, 2)
    gpu = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, seed=3,
                           weights_dtype="fp8")
    cpu = LlamaDecodeModel(TINY, max_batch=2, max_seq=32, device="cpu",
                           seed=3, weights_dtype="fp8")

    def pair(q):
        w8, scale = q
        return w8.view(torch.uint8).cpu().view(FP8), scale.cpu()

    cpu.embed = gpu.embed.cpu()
    cpu.final_norm = gpu.final_norm.cpu()
    cpu.lm_head_q = pair(gpu.lm_head_q)
    for lc, lg in zip(cpu.layers, gpu.layers):
        for attr in ("input_norm", "post_attn_norm"):
            setattr(lc, attr, getattr(lg, attr).cpu())
        for attr in ("wqkv_q", "wo_q", "w_gate_up_q", "w_down_q"):
            setattr(lc, attr, pair(getattr(lg, attr)))
    gpu.context_lens[:2] = 0
    cpu.context_lens[:2] = 0
    tokens = torch.randint(0, TINY.vocab_size, (2,),
                           generator=torch.Generator().manual_seed(5))
    lg = gpu.decode_step(tokens.to(dev))
    lc = cpu.decode_step(tokens)
    assert lg.shape == (2, TINY.vocab_size)
    torch.testing.assert_close(lg.float().cpu(), lc.float(),
                               atol=8e-2, rtol=8e-2)
