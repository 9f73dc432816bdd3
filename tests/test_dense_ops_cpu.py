"""CPU proof that the dense-op oracle (dense_oracle.py) has teeth.

Float32 emulations of the three kernels' algorithms - the skinny GEMM's
128-wide chunks, lane -> k windows, split ranges, fp32 workspace and merge,
64/128-row workgroup tiles and scale at the store; RMSNorm's two passes over
8-wide vectors strided by 256; SwiGLU's strided loop over pairs under the
grid cap - must pass every family at every shape the GPU tests use, and each
mutant of them must be rejected by the family named in its test.
"""
import math

import pytest
import torch

import dense_oracle as do
from dense_oracle import BF16

FP8_MODES = [pytest.param(False, id="bf16"), pytest.param(True, id="fp8")]


def record(family, ratio, note=""):
    print(f"\n[dense-emu] family={family} ratio={ratio:.3f} {note}")


# --------------------------------------------------------------------------
# float32 emulations of the kernels, with mutants
# --------------------------------------------------------------------------

def emulate_gemm(x, w, scale, splits, mutant=None):
    """skinny_gemm_kernel + skinny_gemm_merge_kernel in float32. One MFMA
    of k-subtile kk sums, for lane group g = 0..3 and element i = 0..7, the
    products at k = k0 + 32 g + 8 kk + i (k = k0 + 4 col0 + 8 kk with col0 =
    8 g), for both operands."""
    M, K = x.shape
    N = w.shape[0]
    nsub = 2 if M > 16 else 1
    wg_rows = 64 * nsub
    n_pad = -(-N // wg_rows) * wg_rows
    m_pad = -(-M // 16) * 16
    a = torch.zeros(m_pad, K)                # dead rows are zero fragments
    a[:M] = x.float()
    b = torch.zeros(n_pad, K)
    b[:N] = w.float()
    scl = torch.ones(n_pad)
    if scale is not None:
        scl[:N] = scale
        if mutant == "scale_subtile0" and nsub == 2:
            n = torch.arange(n_pad)
            scl = scl[n - 16 * (n % 32 >= 16).long()]
    per = (K // do.KT) // splits
    g = torch.arange(4)[:, None]
    i = torch.arange(8)[None, :]
    parts = []
    for s in range(splits):
        acc = torch.zeros(m_pad, n_pad)
        n_chunks = per - 1 if mutant == "drop_odd_chunk" and per % 2 else per
        for c in range(s * per, s * per + n_chunks):
            k0 = c * do.KT
            for kk in range(3 if mutant == "drop_kk" else 4):
                if mutant == "drop_one_kk" and (c, kk) == (0, 3):
                    continue
                ka = (k0 + 32 * g + 8 * kk + i).reshape(-1)
                kb = ka
                if mutant == "ab_maps":      # B on the natural 32-run map
                    kb = (k0 + 32 * kk + 8 * g + i).reshape(-1)
                acc = acc + a[:, ka] @ b[:, kb].t()
        part = acc * scl[None, :]            # the scale folds in at the store
        if splits == 1:
            return part[:M, :N].to(BF16)
        if mutant == "ws_bf16":
            part = part.to(BF16).float()
        parts.append(part)
    if mutant == "merge_drop_last":
        parts = parts[:-1]
    out = torch.zeros(m_pad, n_pad)
    for part in parts:
        out = out + part
    return out[:M, :N].to(BF16)


def run_gemm(c, x=None, **kw):
    return emulate_gemm(c.x if x is None else x, c.w, c.scale, c.splits, **kw)


def emulate_rmsnorm(c, mutant=None):
    """rmsnorm_kernel in float32: thread t owns the 8-wide vectors t, t +
    256, ... of a row in both passes. Returns (out, stored residual)."""
    rows, hidden = c.x.shape
    vec_n = hidden // 8
    s = c.x.float()
    stored = None
    if c.res is not None:
        s = s + c.res.float()
        stored = s.to(BF16)
    sq_src = c.x.float() if mutant == "ss_without_residual" else s
    n1 = vec_n - 1 if mutant == "pass1_skips_tail" else vec_n
    passes = -(-vec_n // 256)
    v = torch.zeros(rows, passes * 256, 8)
    v[:, :n1] = sq_src.reshape(rows, vec_n, 8)[:, :n1]
    per_thread = (v * v).reshape(rows, passes, 256, 8).sum(dim=(1, 3))
    ss = per_thread.sum(dim=1, keepdim=True)
    eps = torch.tensor(c.eps, dtype=torch.float32)
    if mutant == "no_eps":
        inv = torch.rsqrt(ss / hidden)
    elif mutant == "eps_before_division":
        inv = torch.rsqrt((ss + eps) / hidden)
    else:
        inv = torch.rsqrt(ss / hidden + eps)
    xo = s if stored is None else stored.float()
    if mutant == "out_from_unfolded_x":
        xo = c.x.float()
    w = c.w.float()
    if mutant == "weight_shifted":
        w = torch.roll(w, -8)
    out = (xo * inv * w[None, :]).to(BF16)
    if mutant == "pass2_skips_tail":
        out[:, 8 * (vec_n - 1):] = 0
    return out, stored


def silu32(g, u):
    g, u = g.float(), u.float()
    return ((g / (1.0 + torch.exp(-g))) * u).to(BF16)


def emulate_silu(c, fused, mutant=None):
    """silu_mul_kernel / silu_mul_fused_kernel: pairs in a grid-stride loop
    under the 8192-workgroup cap; the fused kernel finds pair i of row r at
    r * 2 * inter2 + col of the gate_up buffer, its up at + inter2."""
    rows, cols = c.gate.shape
    inter2 = cols // 2               # fused only: the flat kernel has no rows
    n2 = rows * cols // 2
    if fused:
        gu = do.fuse(c).reshape(-1, 2)
    else:
        gate, up = c.gate.reshape(-1, 2), c.up.reshape(-1, 2)
    out = torch.zeros(n2, 2, dtype=BF16)
    grid = min(do.SILU_GRID_CAP, max(1, -(-n2 // do.SILU_BLOCK)))
    stride = grid * do.SILU_BLOCK
    for start in range(0, n2, stride):
        i = torch.arange(start, min(start + stride, n2))
        if fused:
            row_stride = inter2 if mutant == "row_stride_inter" else 2 * inter2
            base = (i // inter2) * row_stride + i % inter2
            g, u = gu[base], gu[base + inter2]
        else:
            g, u = gate[i], up[i]
        if mutant == "swap_gate_up":
            g, u = u, g
        out[i] = silu32(g, u)
        if mutant == "single_pass":
            break
    return out.reshape(rows, cols)


def ratio(out, ref, bound):
    return do.error_ratio(out, ref, bound)[0]


# --------------------------------------------------------------------------
# GEMM: the unmutated emulation passes every family at every GPU shape
# --------------------------------------------------------------------------

def test_split_literals_match_heuristic_mirror():
    for K, n in do.SPLIT_TABLE.items():
        for M in do.SPLIT_M:
            assert do.heuristic_splits(M, do.SPLIT_N, K) == n, (M, K)
    for M, n in do.WIDE_SPLITS.items():
        assert do.heuristic_splits(M, do.WIDE_N, do.WIDE_K) == n
    for M in do.GEMM_M:
        for N in do.GEMM_N:
            assert do.heuristic_splits(M, N, do.EDGE_K) == do.EDGE_SPLITS
    for M in do.PROBE_M:
        for K, n in do.PROBE_K.items():
            assert do.heuristic_splits(M, do.PROBE_N, K) == n
    for (M, N, K), n in {**do.BOUNDED_SHAPES, **do.CANCEL_SHAPES}.items():
        assert do.heuristic_splits(M, N, K) == n


def probe_mismatches(c, launches, **kw):
    bad = 0
    for r in launches:
        out = run_gemm(c, do.probe_x(c, r), **kw)
        bad += int((out != do.probe_expected(c, r)).sum())
    return bad


@pytest.mark.parametrize("fp8", FP8_MODES)
class TestGemmEmulationPasses:
    @pytest.mark.parametrize("K", list(do.PROBE_K))
    @pytest.mark.parametrize("M", do.PROBE_M)
    def test_probe(self, M, K, fp8):
        c = do.probe_case(M, K, fp8)
        assert c.splits == do.PROBE_K[K]
        launches = do.probe_launches_cpu(c)
        assert launches[0] == 0 and launches[-1] == c.launches - 1
        for r in launches:
            do.assert_equal(run_gemm(c, do.probe_x(c, r)),
                            do.probe_expected(c, r), f"probe launch {r}")

    def test_probe_hits_every_k_once(self, fp8):
        c = do.probe_case(64, 896, fp8)
        hits = sum(do.probe_x(c, r).float() for r in range(c.launches))
        assert torch.equal(hits.sum(dim=0), torch.ones(c.K))
        if fp8:
            codes = torch.unique(c.w.view(torch.uint8))
            assert torch.equal(codes, do.E4M3_FINITE)

    @pytest.mark.parametrize("M", do.GEMM_M)
    def test_integer_edge_grid(self, M, fp8):
        for N in do.GEMM_N:
            c = do.integer_case(M, N, do.EDGE_K, fp8)
            do.assert_equal(run_gemm(c), c.expect, f"integer {M}x{N}")

    @pytest.mark.parametrize("M", do.SPLIT_M)
    def test_integer_split_table(self, M, fp8):
        shapes = [(do.SPLIT_N, K) for K in do.SPLIT_TABLE]
        shapes.append((do.WIDE_N, do.WIDE_K))
        for N, K in shapes:
            c = do.integer_case(M, N, K, fp8)
            do.assert_equal(run_gemm(c), c.expect, f"integer {M}x{N}x{K}")

    @pytest.mark.parametrize("shape", list(do.BOUNDED_SHAPES))
    def test_bounded(self, shape, fp8):
        c = do.bounded_case(*shape, fp8)
        r = do.assert_within(run_gemm(c), c.ref, c.bound, f"bounded {shape}")
        record("gemm-bounded", r, f"shape={shape} fp8={fp8}")

    @pytest.mark.parametrize("shape", list(do.CANCEL_SHAPES))
    def test_bounded_cancelling(self, shape, fp8):
        c = do.cancel_case(*shape, fp8)
        r = do.assert_within(run_gemm(c), c.ref, c.bound, f"cancel {shape}")
        record("gemm-cancel", r, f"shape={shape} fp8={fp8}")


# --------------------------------------------------------------------------
# GEMM: every mutant is rejected, by the family its test names
# --------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", FP8_MODES)
class TestGemmMutantsRejected:
    def test_dropped_kk_subtile_fails_probe_and_integer(self, fp8):
        c = do.probe_case(64, 896, fp8)
        # the k of subtile 3 are 24..31 of every 32-run: a quarter is lost
        bad = probe_mismatches(c, range(c.launches), mutant="drop_kk")
        assert bad >= 0.2 * c.K * c.N
        for M in (1, 16, 17, 64):
            ci = do.integer_case(M, 129, do.EDGE_K, fp8)
            assert not torch.equal(run_gemm(ci, mutant="drop_kk"), ci.expect)
        # one subtile of one chunk is enough for the probe
        assert probe_mismatches(c, range(c.launches), mutant="drop_one_kk")

    def test_different_lane_maps_fail_probe(self, fp8):
        for M, K in ((64, 896), (16, 2048)):
            c = do.probe_case(M, K, fp8)
            bad = probe_mismatches(c, do.probe_launches_cpu(c)[:8],
                                   mutant="ab_maps")
            assert bad > 0

    def test_merge_dropping_last_split_fails_integer(self, fp8):
        for K, n in do.SPLIT_TABLE.items():
            if n == 1:
                continue
            for M in do.SPLIT_M:
                c = do.integer_case(M, do.SPLIT_N, K, fp8)
                out = run_gemm(c, mutant="merge_drop_last")
                # the last k of the last split is nonzero in every x row
                assert not torch.equal(out, c.expect), (M, K)

    def test_dropped_odd_last_chunk_fails_integer_and_probe(self, fp8):
        for K in (896, 2816, 14336):         # 7, 11 and 7 chunks per split
            for M in do.SPLIT_M:
                c = do.integer_case(M, do.SPLIT_N, K, fp8)
                out = run_gemm(c, mutant="drop_odd_chunk")
                assert not torch.equal(out, c.expect), (M, K)
        c = do.probe_case(64, 896, fp8)
        assert probe_mismatches(c, [c.launches - 1], mutant="drop_odd_chunk")

    def test_workspace_in_bf16_fails_bounded(self, fp8):
        """The bound's (K + 16) 2^-23 absref term is a worst case that grows
        with K while a bf16 partial costs 2^-8 of a partial whatever K is:
        the family rejects the mutant at (16, 200, 1536) (1.25x / 1.57x the
        bound), is level with it at (33, 7232, 2048) (0.99x) and no longer
        sees it at K = 3072 (0.63x) and 14336 (0.09x)."""
        seen = {}
        for shape, n in do.BOUNDED_SHAPES.items():
            if n == 1:
                continue
            c = do.bounded_case(*shape, fp8)
            seen[shape] = ratio(run_gemm(c, mutant="ws_bf16"), c.ref, c.bound)
            record("gemm-ws-bf16-mutant", seen[shape], f"shape={shape}")
        assert seen[(16, 200, 1536)] > 1.0, seen
        # the cancelling cases, same bound, see it at every shape
        for shape in do.CANCEL_SHAPES:
            c = do.cancel_case(*shape, fp8)
            r = ratio(run_gemm(c, mutant="ws_bf16"), c.ref, c.bound)
            record("gemm-ws-bf16-mutant", r, f"cancel shape={shape}")
            assert r > 1.5, (shape, r)
        # ... and the integer family cannot see it: its partials are exact
        ci = do.integer_case(64, 128, 2048, fp8)
        assert torch.equal(run_gemm(ci, mutant="ws_bf16"), ci.expect)


def test_scale_of_wrong_subtile_fails_integer_fp8():
    for M in (17, 33, 64):
        for N in (17, 63, 129, 200):
            c = do.integer_case(M, N, do.EDGE_K, True)
            out = run_gemm(c, mutant="scale_subtile0")
            assert not torch.equal(out, c.expect), (M, N)
    # M <= 16 has one subtile per wave: the mutant is the kernel
    c = do.integer_case(16, 200, do.EDGE_K, True)
    assert torch.equal(run_gemm(c, mutant="scale_subtile0"), c.expect)


def test_randn_and_loose_tolerance_miss_the_gemm_mutants():
    """Pins the gap of the fp8 randn case of test_ops_gpu.py (randn * 0.05
    weights, amax / 448 scales, atol = 0.5, rtol = 2e-2; here M = 33, K =
    4096 at N = 512), as measured rather than as estimated per element:

    * a workspace rounded to bf16 passes it outright, everywhere;
    * the scale of the wrong 16-row subtile and one dropped k-subtile of
      one chunk move a typical element by less than the tolerance (0.07 |y|
      at the median, sigma 0.28), so more than 90 % of the elements pass -
      the loose check sees these two only through the tail of 17 000
      elements (4.5 % and 5.9 % outside), with nothing that says which
      elements must be wrong or why.

    The integer and probe families reject the last two on every affected
    element, and the bounded family rejects the first (tests above)."""
    torch.manual_seed(2)
    M, N, K = 33, 512, 4096
    x = torch.randn(M, K).to(BF16)
    w = (torch.randn(N, K) * 0.05).to(BF16)
    w8, scale = do.quantize_fp8(w)
    ref = x.float() @ (w8.float() * scale[:, None]).t()
    splits = do.heuristic_splits(M, N, K)
    assert splits == 16
    good = emulate_gemm(x, w8, scale, splits)

    def outside(out):
        err = (out.float() - ref).abs()
        return float((err > 0.5 + 2e-2 * ref.abs()).float().mean())

    assert outside(good) == 0.0
    out = emulate_gemm(x, w8, scale, splits, mutant="ws_bf16")
    assert not torch.equal(out, good)
    torch.testing.assert_close(out.float(), ref, atol=0.5, rtol=2e-2)
    for mutant in ("scale_subtile0", "drop_one_kk"):
        out = emulate_gemm(x, w8, scale, splits, mutant=mutant)
        changed = float((out != good).float().mean())
        frac = outside(out)
        record("gemm-loose-randn", frac, f"mutant={mutant} changed={changed}")
        assert changed > 0.45 and 0.0 < frac < 0.10, (mutant, changed, frac)


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------

def rms_cases(rows, hidden):
    """(name, case) of every RMSNorm family at one shape."""
    yield "spike", do.rms_spike_case(rows, hidden)
    yield "sign", do.rms_sign_case(rows, hidden)
    for eps in do.RMS_EPS:
        for e in (-30, 30):
            yield f"eps{e}", do.rms_eps_case(rows, hidden, e, eps)
    for kind in do.FUSED_KINDS:
        yield kind, do.rms_fused_case(kind, rows, hidden)


def rms_ratio(c, mutant=None):
    ref, stored = do.rmsnorm_ref64(c.x, c.w, c.res, c.eps)
    out, got = emulate_rmsnorm(c, mutant)
    if stored is not None:
        assert torch.equal(got, stored)
    return ratio(out, ref, do.rel_bound(ref))


@pytest.mark.parametrize("hidden", do.RMS_HIDDEN)
def test_rmsnorm_emulation_within_bound(hidden):
    worst = {}
    for rows in do.RMS_ROWS:
        for name, c in rms_cases(rows, hidden):
            r = rms_ratio(c)
            assert r <= 1.0, (name, rows, hidden, r)
            worst[name] = max(worst.get(name, 0.0), r)
    for name, r in worst.items():
        record("rmsnorm-" + name, r, f"hidden={hidden}")


def test_rmsnorm_spike_is_exact_elsewhere():
    for hidden in do.RMS_HIDDEN:
        c = do.rms_spike_case(257, hidden)
        ref, _ = do.rmsnorm_ref64(c.x, c.w, None, c.eps)
        assert int((ref != 0).sum()) == 257
        assert set(do.spike_positions(hidden)) >= {0, hidden - 1}


class TestRmsnormMutantsRejected:
    def test_no_eps_fails_the_small_rows(self):
        for hidden in do.RMS_HIDDEN:
            for eps in do.RMS_EPS:
                c = do.rms_eps_case(3, hidden, -30, eps)
                assert rms_ratio(c, "no_eps") > 100, (hidden, eps)
            # unit-scale rows cannot tell: eps is 1e-5 of the mean square
            c = do.rms_fused_case("randn", 3, hidden)
            assert rms_ratio(c, "no_eps") <= 1.0

    def test_eps_before_division_fails_the_small_rows(self):
        for hidden in do.RMS_HIDDEN:
            for eps in do.RMS_EPS:
                c = do.rms_eps_case(3, hidden, -30, eps)
                assert rms_ratio(c, "eps_before_division") > 100, (hidden, eps)

    def test_pass1_tail_skipped_fails_spike(self):
        for hidden in do.RMS_HIDDEN:
            c = do.rms_spike_case(257, hidden)
            assert rms_ratio(c, "pass1_skips_tail") > 100, hidden

    def test_pass2_tail_skipped_fails_spike_and_sign(self):
        for hidden in do.RMS_HIDDEN:
            for c in (do.rms_spike_case(257, hidden),
                      do.rms_sign_case(3, hidden)):
                assert rms_ratio(c, "pass2_skips_tail") > 100, hidden

    def test_weight_shifted_by_a_vector_fails_sign(self):
        for hidden in do.RMS_HIDDEN[1:]:     # at 8 the shift wraps to itself
            c = do.rms_sign_case(3, hidden)
            assert rms_ratio(c, "weight_shifted") > 5, hidden

    def test_residual_missing_from_ss_fails_fused(self):
        for hidden in do.RMS_HIDDEN:
            for kind in ("randn", "cancel"):
                c = do.rms_fused_case(kind, 3, hidden)
                assert rms_ratio(c, "ss_without_residual") > 10, (hidden, kind)

    def test_output_from_unfolded_x_fails_fused(self):
        for hidden in do.RMS_HIDDEN:
            for kind in ("randn", "cancel"):
                c = do.rms_fused_case(kind, 3, hidden)
                assert rms_ratio(c, "out_from_unfolded_x") > 10, (hidden, kind)


def test_rmsnorm_round_case_needs_rounding():
    c = do.rms_fused_case("round", 3, 2048)
    s32 = c.x.float() + c.res.float()
    assert bool((s32.to(BF16).float() != s32).all())


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------

def silu_ratio(c, fused, mutant=None):
    ref = do.silu_ref64(c.gate, c.up)
    return ratio(emulate_silu(c, fused, mutant), ref, do.rel_bound(ref))


FUSED = [pytest.param(False, id="flat"), pytest.param(True, id="fused")]


def position_shapes(fused):
    big = do.POSITION_FUSED if fused else do.POSITION_FLAT
    return do.POSITION_SHAPES + (big,)


@pytest.mark.parametrize("fused", FUSED)
class TestSiluEmulationPasses:
    def test_gate_sweep(self, fused):
        c = do.gate_sweep_case()
        assert float(c.gate.float().abs().max()) == 80.0
        r = silu_ratio(c, fused)
        assert r <= 1.0
        record("silu-sweep", r, f"fused={fused}")

    def test_saturation(self, fused):
        c = do.saturation_case()
        out = emulate_silu(c, fused).float()
        assert bool(torch.isfinite(out).all())
        assert float(out[:3].abs().max()) < 2.0 ** -126
        assert torch.equal(out[3], torch.full_like(out[3], 1000.0))

    def test_position_code(self, fused):
        for shape in position_shapes(fused):
            c = do.position_case(*shape)
            r = silu_ratio(c, fused)
            assert r <= 1.0, shape
            record("silu-position", r, f"shape={shape} fused={fused}")


def test_position_shapes_cross_the_first_grid_pass():
    for rows, cols in (do.POSITION_FLAT, do.POSITION_FUSED):
        assert rows * cols // 2 > do.SILU_FIRST_PASS
    for rows, cols in do.POSITION_SHAPES:
        assert rows * cols // 2 < do.SILU_FIRST_PASS


class TestSiluMutantsRejected:
    @pytest.mark.parametrize("fused", FUSED)
    def test_single_stride_pass_fails_position(self, fused):
        c = do.position_case(*position_shapes(fused)[-1])
        assert silu_ratio(c, fused, "single_pass") > 100
        # below the cap there is no second pass to lose
        c = do.position_case(5, 2816)
        assert silu_ratio(c, fused, "single_pass") <= 1.0

    def test_row_stride_inter_fails_position(self):
        for shape in position_shapes(True):
            c = do.position_case(*shape)
            assert silu_ratio(c, True, "row_stride_inter") > 100, shape

    @pytest.mark.parametrize("fused", FUSED)
    def test_swapped_gate_and_up_fails_position(self, fused):
        for shape in do.POSITION_SHAPES:
            c = do.position_case(*shape)
            assert silu_ratio(c, fused, "swap_gate_up") > 10, shape


def test_silu_bound_is_tight_where_it_should_be():
    """The bound is one output rounding plus 2^-12: silu(1) * 3 in bf16 must
    sit inside it, and a 1 % error outside."""
    g = torch.ones(1, 2, dtype=BF16)
    u = torch.full((1, 2), 3.0, dtype=BF16)
    ref = do.silu_ref64(g, u)
    assert math.isclose(float(ref[0, 0]), 3 / (1 + math.exp(-1)))
    assert ratio(ref.to(BF16), ref, do.rel_bound(ref)) <= 1.0
    assert ratio((ref * 1.01).to(BF16), ref, do.rel_bound(ref)) > 1.0
