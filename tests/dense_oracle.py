"""Float64 oracles, derived error bounds and adversarial case builders for
the dense decode ops: the skinny GEMM (bf16 and e4m3 weights), RMSNorm (plain
and fused with the residual add) and SwiGLU (flat and fused gate_up).

Plain helper module: torch on CPU only, no GPU calls. The GPU tests in
test_dense_ops_gpu.py run the kernels on these cases; the CPU tests in
test_dense_ops_cpu.py prove, with mutants of float32 emulations of the
kernels' algorithms, that the cases plus the bounds reject a subtly wrong
kernel.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from attn_oracle import BF16, FP8, error_ratio, f64  # noqa: F401

# --------------------------------------------------------------------------
# skinny GEMM: shapes shared by the CPU and GPU tests
# --------------------------------------------------------------------------

KT = 128                    # k elements per chunk
MAX_WGS = 1792              # workgroups the split heuristic fills
GEMM_M = (1, 15, 16, 17, 33, 48, 49, 64)
GEMM_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
EDGE_K = 1536
EDGE_SPLITS = 4
# K -> split count at N = 128 (any M): 896 is 7 chunks unsplit (odd trip
# count), 2816 is TINY's down projection (11 chunks per split), 14336 has 7
# chunks per split
SPLIT_N = 128
SPLIT_TABLE = {128: 1, 896: 1, 768: 2, 1536: 4, 3072: 8, 2048: 16, 2816: 2,
               14336: 16}
SPLIT_M = (16, 17, 64)
# 113 workgroups of 64 rows (113 * 16 > 1792) against 57 of 128 rows
WIDE_N, WIDE_K = 7232, 2048
WIDE_SPLITS = {16: 8, 17: 16, 64: 16}
PROBE_M = (64, 16)
PROBE_N = 129
PROBE_K = {896: 1, 2048: 16, 14336: 16}
BOUNDED_SHAPES = {(1, 128, 896): 1, (16, 200, 1536): 4, (17, 129, 3072): 8,
                  (33, 7232, 2048): 16, (64, 128, 14336): 16}
CANCEL_SHAPES = {(16, 128, 768): 2, (33, 200, 768): 2, (16, 200, 1536): 4}
DETERMINISM_SHAPE = (64, 128, 14336)


def tile_n(M: int) -> int:
    """Workgroup N-tile: 64 rows (one 16-row subtile per wave) up to M = 16,
    128 rows (two subtiles per wave) above."""
    return 128 if M > 16 else 64


def heuristic_splits(M: int, N: int, K: int) -> int:
    """Mirror of skinny_gemm_num_splits. Only the CPU emulation and the
    case builders split by it; the GPU tests assert literal counts against
    the extension's own answer."""
    nt = tile_n(M)
    n_wgs = (N + nt - 1) // nt
    chunks = K // KT
    sk = 1
    while sk < 16 and n_wgs * sk * 2 <= MAX_WGS and chunks % (sk * 2) == 0:
        sk *= 2
    return sk


def _gemm_case(x, w, scale, splits, **extra):
    return SimpleNamespace(x=x.contiguous(), w=w.contiguous(),
                           scale=None if scale is None else scale.contiguous(),
                           fp8=w.dtype == FP8, splits=splits,
                           M=x.shape[0], N=w.shape[0], K=x.shape[1], **extra)


def w_eff64(w, scale):
    """The weights the kernel multiplies by, in float64."""
    wd = f64(w)
    return wd if scale is None else wd * scale.double()[:, None]


def gemm_ref64(c):
    """(ref, absref) = (x . w_eff^T, |x| . |w_eff|^T), float64 [M, N]."""
    xd, wd = f64(c.x), w_eff64(c.w, c.scale)
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def gemm_bound(ref, absref, K):
    """2^-8 |ref| + (K + 16) 2^-23 absref per element.

    Products of bf16 values (e4m3 values are bf16 values) are exact in
    float32. Summing them in any order, plus at most 16 merge additions,
    is K + 16 float32 additions, each off by at most 2^-23 (rounded or
    truncated) of a running sum whose magnitude absref bounds; the scale
    multiply of the fp8 path is one more such step (the 16 is never all
    used: there are at most 15 merge additions). The bf16 output rounding
    gets 2^-8 |ref| and no margin, and there is no absolute floor. A
    partial sum or workspace kept in bf16 adds 2^-8 of a partial per
    split, far outside this."""
    return 2.0 ** -8 * ref.abs() + (K + 16) * 2.0 ** -23 * absref


# all 254 finite e4m3fn codes: 0x7f and 0xff are NaN
E4M3_FINITE = torch.tensor(
    [b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)


def probe_weights(N, K, fp8, seed=0):
    """Random weights of the probe family. bf16: randn. fp8: bytes drawn
    from all 254 finite e4m3 codes, every code present, with random
    positive float32 scales that are no power of two. Returns (w, scale,
    expect [N, K] bf16) where expect is what a one-hot x row at k must
    give: w itself, or bf16(float32(w8) * scale) - the kernel's only
    operations on the value are one float32 multiply and one rounding."""
    g = torch.Generator().manual_seed(seed)
    if not fp8:
        w = torch.randn(N, K, generator=g).to(BF16)
        return w, None, w.clone()
    assert N * K >= 2 * len(E4M3_FINITE)
    extra = torch.randint(0, len(E4M3_FINITE), (N * K - len(E4M3_FINITE),),
                          generator=g)
    codes = torch.cat([E4M3_FINITE, E4M3_FINITE[extra]])
    codes = codes[torch.randperm(N * K, generator=g)].reshape(N, K)
    assert len(torch.unique(codes)) == len(E4M3_FINITE)
    w = codes.contiguous().view(FP8)
    scale = ((0.75 + torch.rand(N, generator=g))
             * torch.exp2(torch.randint(-4, 5, (N,), generator=g).float()))
    mant, _ = torch.frexp(scale)
    assert bool((mant != 0.5).all()) and bool((scale > 0).all())
    expect = (w.float() * scale[:, None]).to(BF16)
    return w, scale, expect


@functools.lru_cache(maxsize=None)
def probe_case(M, K, fp8):
    """The probe family at N = PROBE_N: launch r has x[m, :] one-hot (value
    1) at k = r * M + m, r = 0 .. K / M - 1, so every k of the shape is hit
    exactly once, each by a different row. Every other product is 0, so
    y[m, n] must equal expect[n, r * M + m] bit for bit: a k lost,
    duplicated or paired with another k of the other operand, an (m, n)
    mis-assignment and an e4m3 conversion error each change it."""
    assert K % M == 0
    w, scale, expect = probe_weights(PROBE_N, K, fp8, seed=K + M)
    return _gemm_case(torch.zeros(M, K, dtype=BF16), w, scale,
                      heuristic_splits(M, PROBE_N, K), expect=expect,
                      launches=K // M)


def probe_x(c, r):
    x = torch.zeros(c.M, c.K, dtype=BF16)
    x[torch.arange(c.M), r * c.M + torch.arange(c.M)] = 1
    return x


def probe_expected(c, r):
    """[M, N] bf16: row m is column r * M + m of expect."""
    return c.expect[:, r * c.M: (r + 1) * c.M].t().contiguous()


def probe_launches_cpu(c):
    """The launches the CPU emulation runs: all of them at small K, else the
    first, the last and one middle launch of every split's k range."""
    if c.launches <= 64:
        return list(range(c.launches))
    span = c.K // c.splits
    picks = set()
    for s in range(c.splits):
        lo, hi = s * span // c.M, ((s + 1) * span - 1) // c.M
        picks.update((lo, (lo + hi) // 2, hi))
    return sorted(picks)


def integer_case(M, N, K, fp8, seed=0):
    """Dense w in {-2 .. 2} (exact in bf16 and e4m3); every x row has at
    most 64 nonzeros in {+-1, +-2}: at k = 0 and K - 1, at the first and
    last k of every split's range, and at seeded positions for the rest.
    fp8 scales are 2^((n mod 7) - 3), so the row 16 further on has another
    scale by a factor of 4 or more. sum |x| |w| <= 256 (asserted), so every
    partial sum and the bf16 output are exact integers times a power of
    two: the output must torch.equal the float64 reference cast to bf16.
    Catches lost chunks and splits, the merge, the M and N tile edges of
    both instantiations and a scale read from the wrong row."""
    g = torch.Generator().manual_seed(seed + 7 * M + 131 * N + K)
    sk = heuristic_splits(M, N, K)
    span = K // sk
    fixed = sorted({0, K - 1} | {s * span for s in range(sk)}
                   | {(s + 1) * span - 1 for s in range(sk)})
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    x = torch.zeros(M, K)
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])
    for m in range(M):
        free = torch.randperm(K, generator=g)[: 64 - len(fixed)].tolist()
        pos = torch.tensor(sorted(set(fixed) | set(free)))
        assert len(pos) <= 64
        x[m, pos] = vals[torch.randint(0, 4, (len(pos),), generator=g)]
    assert float((x.abs() @ w.abs().t()).max()) <= 256
    scale = None
    if fp8:
        scale = torch.exp2(((torch.arange(N) % 7) - 3).float())
    c = _gemm_case(x.to(BF16), w.to(FP8 if fp8 else BF16), scale, sk)
    ref, _ = gemm_ref64(c)
    c.expect = ref.to(BF16)
    assert torch.equal(f64(c.expect), ref)       # exact in bf16
    return c


def quantize_fp8(w):
    """calibration.model._quantize_fp8: per-row amax / 448 scales."""
    scale = (w.abs().amax(dim=1).float() / 448.0).clamp_min(1e-12)
    w8 = (w.float() / scale[:, None]).clamp(-448.0, 448.0).to(FP8)
    return w8.contiguous(), scale.contiguous()


@functools.lru_cache(maxsize=None)
def bounded_case(M, N, K, fp8):
    """randn activations against randn * 0.05 weights (quantised as the
    engine does for fp8), with (ref, absref, bound). This is the family
    that sees a partial or a workspace kept in bf16."""
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
    scale = None
    if fp8:
        w, scale = quantize_fp8(w)
    c = _gemm_case(x, w, scale, heuristic_splits(M, N, K))
    c.ref, c.absref = gemm_ref64(c)
    c.bound = gemm_bound(c.ref, c.absref, K)
    return c


@functools.lru_cache(maxsize=None)
def cancel_case(M, N, K, fp8):
    """A bounded case whose two halves of K nearly cancel: x = [x1, -x1], w
    = [w1, w1 + 2^-4 noise]. The split partials are ~16x the result, so
    2^-8 |ref| is small and the bound is its float32 term, which at K <=
    1536 is 2^-12.4 absref or less: a partial rounded to bf16 (up to 2^-8
    of a partial each) is several times that, where the plain randn case
    sees it at 1.25x. Same bound as bounded_case, no term added."""
    g = torch.Generator().manual_seed(M * 1000 + N + K + 1)
    h = K // 2
    x1 = torch.randn(M, h, generator=g)
    w1 = torch.randn(N, h, generator=g) * 0.05
    w2 = w1 + 2.0 ** -4 * 0.05 * torch.randn(N, h, generator=g)
    x = torch.cat([x1, -x1], dim=1).to(BF16)
    w = torch.cat([w1, w2], dim=1).to(BF16)
    scale = None
    if fp8:
        w, scale = quantize_fp8(w)
    c = _gemm_case(x, w, scale, heuristic_splits(M, N, K))
    c.ref, c.absref = gemm_ref64(c)
    c.bound = gemm_bound(c.ref, c.absref, K)
    return c


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------

RMS_HIDDEN = (8, 16, 2040, 2048, 2056, 4096, 5120)   # vec_n 1 .. 640
RMS_ROWS = (1, 3, 257)
RMS_EPS = (1e-5, 1e-6)
SPIKE = 128.0
REL_BOUND = 2.0 ** -8 + 2.0 ** -12


def rms_weight(hidden):
    """w[i] = 1 + (i mod 128) / 128: exact in bf16, different at every
    index of a 128-run, so a shifted weight index shows."""
    return (1 + (torch.arange(hidden) % 128).float() / 128).to(BF16)


def rmsnorm_ref64(x, w, residual=None, eps=1e-5):
    """Float64 mirror of the kernel's contract. eps is the float32 value
    the launch receives. Fused: the stored residual is bf16(fp32(x) +
    fp32(res)); the sum of squares comes from the unrounded float32 sums,
    the output from the stored bf16 residual. Returns (ref, stored)."""
    eps32 = float(np.float32(eps))
    if residual is None:
        stored, s, xo = None, f64(x), f64(x)
    else:
        s32 = x.float() + residual.float()
        stored = s32.to(BF16)
        s, xo = s32.double(), f64(stored)
    hidden = x.shape[-1]
    ms = (s * s).sum(dim=-1, keepdim=True) / hidden
    ref = xo / torch.sqrt(ms + eps32) * f64(w)
    return ref, stored


def rel_bound(ref):
    """(2^-8 + 2^-12) |ref|: one bf16 output rounding with no margin, and
    2^-12 for the float32 order of the sum, rsqrtf / __expf and the two
    float32 multiplies - the float32 term of the v4 attention bound. Where
    ref is 0 the output must be 0."""
    return REL_BOUND * ref.abs()


def spike_positions(hidden):
    js = (0, 7, 8, 2039, 2040, 2047, hidden - 8, hidden - 1)
    return sorted({j for j in js if 0 <= j < hidden})


def rms_spike_case(rows, hidden):
    """Row r is 0 except SPIKE at one of the vector-edge indices (cycled
    over the rows). Every other output must be exactly 0; an element
    dropped from the sum of squares gives 128 rsqrt(eps) ~ 40000 in place
    of sqrt(hidden)."""
    js = spike_positions(hidden)
    x = torch.zeros(rows, hidden, dtype=BF16)
    for r in range(rows):
        x[r, js[r % len(js)]] = SPIKE
    return SimpleNamespace(x=x, w=rms_weight(hidden), res=None, eps=1e-5)


def rms_sign_case(rows, hidden, seed=0):
    """x[r, i] = +-2^(r mod 3) with seeded signs per row: the sum of squares
    is exact, and the sign pattern and the weight ramp show a shifted x,
    weight or row index."""
    g = torch.Generator().manual_seed(seed + rows + hidden)
    sign = torch.randint(0, 2, (rows, hidden), generator=g).float() * 2 - 1
    mag = torch.exp2((torch.arange(rows) % 3).float())[:, None]
    return SimpleNamespace(x=(sign * mag).to(BF16), w=rms_weight(hidden),
                           res=None, eps=1e-5)


def rms_eps_case(rows, hidden, exponent, eps, seed=0):
    """randn rows scaled by 2^exponent. At -30 the mean square is far below
    eps and the output is x rsqrt(eps) w; at +30 eps must vanish. A missing
    or misplaced eps is a large error in the first."""
    g = torch.Generator().manual_seed(seed + rows + hidden)
    x = (torch.randn(rows, hidden, generator=g) * 2.0 ** exponent).to(BF16)
    return SimpleNamespace(x=x, w=rms_weight(hidden), res=None, eps=eps)


FUSED_KINDS = ("randn", "cancel", "round")


def rms_fused_case(kind, rows, hidden, seed=0):
    """x and a residual: "randn" both random; "cancel" res = -x + 2^-6
    randn, so the sum is 100x smaller than either operand; "round" x = +-1,
    res = +-{1, 3} 2^-9, sums that need rounding to bf16 (1 + 2^-9 is a tie,
    1 + 3 2^-9 rounds up)."""
    g = torch.Generator().manual_seed(seed + rows + hidden)
    if kind == "randn":
        x = torch.randn(rows, hidden, generator=g).to(BF16)
        res = torch.randn(rows, hidden, generator=g).to(BF16)
    elif kind == "cancel":
        x = torch.randn(rows, hidden, generator=g).to(BF16)
        res = (-x.float()
               + 2.0 ** -6 * torch.randn(rows, hidden, generator=g)).to(BF16)
    else:
        sign = torch.randint(0, 2, (rows, hidden), generator=g).float() * 2 - 1
        c = torch.randint(0, 2, (rows, hidden), generator=g).float() * 2 + 1
        x = sign.to(BF16)
        res = (sign * c * 2.0 ** -9).to(BF16)
    return SimpleNamespace(x=x, w=rms_weight(hidden), res=res, eps=1e-5)


# --------------------------------------------------------------------------
# SwiGLU
# --------------------------------------------------------------------------

SILU_BLOCK = 256
SILU_GRID_CAP = 8192
SILU_FIRST_PASS = SILU_GRID_CAP * SILU_BLOCK        # pairs of one grid pass
SAT_GATES = (-100.0, -1000.0, -3.38e38)
POSITION_SHAPES = ((3, 2), (3, 6), (5, 2816))       # flat and fused
POSITION_FLAT = (2, SILU_FIRST_PASS + 3)            # 3 pairs past one pass
POSITION_FUSED = (293, 14336)                       # 2 100 224 pairs


def silu_ref64(g, u):
    gd = f64(g)
    return gd / (1 + torch.exp(-gd)) * f64(u)


def gate_sweep_case(seed=0):
    """Gates 0, +-2^-20, +-1, every integer in +-[2, 80] and a randn * 8
    block (|g| <= 80), one row per u in {1, -1, 3, -3, randn}. __expf is
    good to ~2^-17 at |g| = 80 and 1 + e^-g does not cancel, so
    rel_bound holds over the whole sweep."""
    g = torch.Generator().manual_seed(seed)
    ints = torch.arange(2, 81).float()
    gates = torch.cat([
        torch.tensor([0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0]), ints, -ints,
        (torch.randn(93, generator=g) * 8).clamp(-80, 80)])
    n = len(gates)
    assert n % 2 == 0
    up = torch.stack([torch.ones(n), -torch.ones(n), 3 * torch.ones(n),
                      -3 * torch.ones(n), torch.randn(n, generator=g)])
    gate = gates[None, :].expand(5, n).contiguous()
    return SimpleNamespace(gate=gate.to(BF16), up=up.to(BF16))


def saturation_case(seed=0):
    """Outside the bound's range: gates of SAT_GATES (e^-g overflows) and
    1000 (e^-g underflows), against u in {+-1, +-3, randn}; the last row
    pairs g = 1000 with u = 1, which must give exactly 1000."""
    g = torch.Generator().manual_seed(seed)
    n = 8
    us = torch.cat([torch.tensor([1.0, -1.0, 3.0, -3.0]),
                    torch.randn(n - 4, generator=g)])
    gate = torch.tensor(SAT_GATES + (1000.0,))[:, None].expand(4, n)
    up = us[None, :].expand(4, n).clone()
    up[3] = 1.0
    return SimpleNamespace(gate=gate.contiguous().to(BF16), up=up.to(BF16))


def position_case(rows, cols):
    """g = 1 everywhere; u is a small integer hashed from (row, col) into
    -125 .. 125, different between neighbours in either direction. The
    expected output is silu(1) * u: a missing second grid pass leaves
    elements unwritten, a wrong row stride, swapped gate and up or swapped
    lo and hi change which u an element sees."""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    up = ((r * 131 + c * 7 + 3) % 251 - 125).to(BF16)
    gate = torch.ones(rows, cols, dtype=BF16)
    return SimpleNamespace(gate=gate, up=up)


def fuse(c):
    """The [rows, 2 * inter] gate_up buffer of a case."""
    return torch.cat([c.gate, c.up], dim=1).contiguous()


# --------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------

def assert_within(out, ref, bound, what=""):
    """Fail with the worst err/bound ratio and its index; return the
    ratio. A zero bound demands an exact zero."""
    out = out.detach().cpu()
    worst, idx = error_ratio(out, ref, bound)
    assert worst <= 1.0, (
        f"{what}: worst err/bound = {worst:.3g} at {idx}: "
        f"out {float(out[idx]):.6g}, ref {float(ref[idx]):.6g}, "
        f"bound {float(bound[idx]):.3g}")
    return worst


def assert_equal(out, expect, what=""):
    """torch.equal with the first differing index in the message."""
    out = out.detach().cpu()
    if torch.equal(out, expect):
        return
    assert out.shape == expect.shape, (what, out.shape, expect.shape)
    bad = (out != expect) | torch.isnan(out.float())
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first "
        f"at {idx}: out {float(out[idx]):.6g}, expected "
        f"{float(expect[idx]):.6g}")
