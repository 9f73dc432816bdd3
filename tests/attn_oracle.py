"""Float64 oracle, derived error bound and adversarial case builders for the
attention path (decode v4/v5, split merge, prefill) and RoPE.

Plain helper module: torch on CPU only, no GPU calls. The GPU tests in
test_attention_edges_gpu.py run the kernels on these cases; the CPU tests in
test_attn_oracle_cpu.py prove, with mutants of a float32 emulation of the
kernels' algorithm, that the cases plus the bound reject a subtly wrong kernel.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

D = 128
TILE = 64
FP8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
SCALE = D ** -0.5

# Shapes shared by the GPU tests and the CPU proof that the emulation passes
# at exactly those shapes.
SPLIT_GRID = {64: 1, 256: 2, 640: 5, 2048: 16, 12288: 24, 20008: 39}
EDGE_S = 136                       # cache rows of the tile-edge sentinel batch
EDGE_LENS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, EDGE_S - 1, EDGE_S)
EDGE_GROUPS = (1, 4, 8)
GAINS = (1.0, 6.0)
CENSUS_CTX = (65, 300, 1000, 2000)
RAMP_DIRECTIONS = ("up", "down", "peak")
RAMP_SPLIT_S = (640, 2048)
RAMP_UNSPLIT_S = 300
# batch·kv-head count from which the launch heuristic stops splitting
UNSPLIT_REPLICAS = 900
PREFILL_S = (1, 63, 64, 65, 129, 200)
PREFILL_HEADS = ((4, 4), (8, 2), (8, 1))
ROPE_POSITIONS = (0, 1, 1608, 1609, 2047, 8191, 32767, 131071)
ROPE_THETA = 500000.0


EDGE_SPLITS = 2
CENSUS_SPLITS = {65: 2, 300: 3, 1000: 8, 2000: 16}
RAMP_SPLITS = {640: 5, 2048: 16}


def heuristic_splits(base: int, max_seq: int, min_tiles: int = 8) -> int:
    """Mirror of the launch heuristic (gqa_decode_attn_num_splits) for
    base = batch·kv-heads. Only the CPU emulation splits by it; the GPU
    tests assert literal counts against the extension's own answer."""
    if base >= 1792:
        return 1
    splits = min(1792 // base, max(16, max_seq // (min_tiles * TILE)))
    return max(1, min(splits, (max_seq + 2 * TILE - 1) // (2 * TILE)))


def census_rows(ctx: int) -> int:
    """Cache rows of the split census case: a few dead rows past ctx, and
    more than two tiles so that the launch splits."""
    return max(ctx + 8, 200)


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------

def quantize_q_fp8(q: torch.Tensor, num_kv_heads: int) -> torch.Tensor:
    """Q as the fp8-KV decode kernels see it (load_q_frags): one scale per
    (b, kv-head) group, s = max(amax over the group's G heads x 128 dims /
    448, 1e-12), q <- e4m3(q / s) * s, round-to-nearest. The kernel forms
    q * (1 / s) in float32, so this does too: the same products round the
    same way. Returns float32 [B, Hq, D]."""
    B, Hq, d = q.shape
    G = Hq // num_kv_heads
    qf = q.float().reshape(B, num_kv_heads, G * d)
    amax = qf.abs().amax(dim=-1, keepdim=True)
    s = torch.clamp(amax / 448.0, min=1e-12)
    inv = 1.0 / s
    q8 = (qf * inv).clamp(-448.0, 448.0).to(FP8).float()
    return (q8 * s).reshape(B, Hq, d)


def _masked_softmax_pv(scores, v, mask):
    """scores [..., n] float64, v [..., n, D] (broadcastable), mask [..., n].
    Returns (P.V, P.|V|); rows with an empty mask give exactly 0."""
    neg = torch.full_like(scores, -math.inf)
    sc = torch.where(mask, scores, neg)
    m = sc.amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.where(mask, torch.exp(sc - m), torch.zeros_like(sc))
    s = p.sum(dim=-1, keepdim=True)
    p = torch.where(s > 0, p / torch.where(s > 0, s, torch.ones_like(s)),
                    torch.zeros_like(p))
    return p @ v, p @ v.abs()


def decode_ref64(q, k_cache, v_cache, lens, scale, q_fp8=False):
    """Float64 decode attention over a head-major cache [B, Hk, S, D].
    Returns (ref, absref) = (P.V, P.|V|), both [B, Hq, D] float64, with P the
    softmax over positions < lens[b]. Rows at or past lens[b] are never
    looked at (they may hold NaN)."""
    B, Hq, d = q.shape
    _, Hk, S, _ = k_cache.shape
    G = Hq // Hk
    qd = quantize_q_fp8(q, Hk).double() if q_fp8 else f64(q)
    qd = qd.reshape(B, Hk, G, d)
    live = torch.arange(S)[None, :] < lens.long().reshape(B, 1)   # [B, S]
    rows = live[:, None, :, None]
    k = torch.where(rows, f64(k_cache), torch.zeros((), dtype=torch.float64))
    v = torch.where(rows, f64(v_cache), torch.zeros((), dtype=torch.float64))
    scores = torch.einsum("bhgd,bhsd->bhgs", qd, k) * scale
    ref, absref = _masked_softmax_pv(scores, v, live[:, None, None, :])
    return ref.reshape(B, Hq, d), absref.reshape(B, Hq, d)


def prefill_ref64(q, k_cache, v_cache, batch, seq, scale):
    """Float64 causal attention. q [B*S, Hq, D], caches [B, Hk, S_max, D];
    key kp is visible to query row qr iff kp <= qr and kp < S. Returns
    (ref, absref), both [B*S, Hq, D] float64."""
    T, Hq, d = q.shape
    _, Hk, S_max, _ = k_cache.shape
    G = Hq // Hk
    qd = f64(q).reshape(batch, seq, Hk, G, d)
    pos = torch.arange(S_max)
    rows = (pos < seq)[None, None, :, None]
    k = torch.where(rows, f64(k_cache), torch.zeros((), dtype=torch.float64))
    v = torch.where(rows, f64(v_cache), torch.zeros((), dtype=torch.float64))
    scores = torch.einsum("bqhgd,bhsd->bhgqs", qd, k) * scale
    mask = (pos[None, :] <= torch.arange(seq)[:, None]) & (pos < seq)[None, :]
    ref, absref = _masked_softmax_pv(scores, v[:, :, None],
                                     mask[None, None, None])
    # [B, Hk, G, S, D] -> [B*S, Hq, D]
    shape = (T, Hq, d)
    return (ref.permute(0, 3, 1, 2, 4).reshape(shape),
            absref.permute(0, 3, 1, 2, 4).reshape(shape))


def rope_ref64(x, positions, theta=ROPE_THETA):
    """NeoX half-rotation RoPE on x [T, H, D]; inv_freq and the angles are
    float64."""
    _, _, d = x.shape
    half = d // 2
    inv_freq = theta ** (-2.0 * torch.arange(half, dtype=torch.float64) / d)
    angle = positions.double()[:, None] * inv_freq[None, :]
    cos, sin = angle.cos()[:, None, :], angle.sin()[:, None, :]
    xd = f64(x)
    x1, x2 = xd[..., :half], xd[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def rope_delta(positions, head_dim, theta=ROPE_THETA):
    """Per position: 4 x max_d |angle_fp32 - angle_fp64|, the float32 angle
    being the project's own formula (ops.rope_ref). The factor 4 is the
    margin for a different, still float32, order of evaluation."""
    half = head_dim // 2
    inv32 = theta ** (
        -2.0 * torch.arange(half, dtype=torch.float32) / head_dim)
    a32 = positions.float()[:, None] * inv32[None, :]
    inv64 = theta ** (
        -2.0 * torch.arange(half, dtype=torch.float64) / head_dim)
    a64 = positions.double()[:, None] * inv64[None, :]
    return 4.0 * (a32.double() - a64).abs().amax(dim=1)


def rope_bound(x, ref, positions, theta=ROPE_THETA):
    """2^-8 |ref| + delta(pos) (|x1| + |x2|) per element of x [T, H, D]:
    one bf16 rounding of the result (at most 2^-8 of it) plus the rotation
    by an angle that is off by delta."""
    d = x.shape[-1]
    half = d // 2
    xd = f64(x).abs()
    mag = xd[..., :half] + xd[..., half:]
    mag = torch.cat([mag, mag], dim=-1)
    delta = rope_delta(positions, d, theta)[:, None, None]
    return 2.0 ** -8 * ref.abs() + delta * mag


def e4m3_ulp(x):
    """Spacing of e4m3 at |x| (float64): 2^(e-3) for normals, 2^-9 below
    2^-6."""
    a = x.abs().clamp(min=2.0 ** -6)
    return torch.exp2(torch.floor(torch.log2(a)) - 3)


# --------------------------------------------------------------------------
# bound and comparison
# --------------------------------------------------------------------------

def attn_bound(ref, absref, p_bf16: bool):
    """Element-wise error bound of an attention output against the float64
    reference, derived rather than tuned.

    The inputs are exact bf16 / e4m3 values and the kernels keep scores,
    softmax sums and accumulators in float32, so only two roundings are
    coarser than float32. bf16 keeps 8 significant bits, so one
    round-to-nearest is off by at most 2^-8 of the value (half a spacing of
    2^-7, relative to the bottom of the binade):
      * the bf16 output:            <= 2^-8 |ref|
      * v5 and prefill only, P cast to bf16 for the PV MFMA:
                                    <= 2^-8 sum_t p_t |v_t| = 2^-8 absref
    Everything else is float32: accumulation order, the normaliser, and
    __expf, whose argument (up to ~90 in magnitude) carries a relative
    2^-24, i.e. ~2^-17 on p. The bounds are
      v4 (float32 P):       2^-8 |ref| + 2^-12 absref
      v5, prefill (bf16 P): 2^-8 |ref| + 2^-8  absref
    so the output rounding gets no margin at all and the float32 effects
    get 2^-12 absref (v4), or the slack between the worst case of the P
    roundings, all in one direction, and what they really sum to (v5).
    Measured on an MI355X, the worst ratio of a correct kernel is 0.94: one
    output rounding at its worst, 2^-8 / (2^-8 + 2^-12).
    The prefill kernel stages P to LDS in float32 but builds its PV A
    fragments with f2bf_bits, so its P does go through bf16: it takes the
    p_bf16=True bound. There is no absolute floor: where ref and absref are
    0 the output must be 0."""
    return 2.0 ** -8 * ref.abs() + (2.0 ** -8 if p_bf16 else 2.0 ** -12) * absref


def error_ratio(out, ref, bound):
    """Worst err / bound over all elements and its index. 0/0 counts as 0,
    anything non-finite or non-zero over a zero bound as inf."""
    err = (f64(out) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(f64(out)), ratio,
                        torch.full_like(ratio, math.inf))
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat),
                                                    ratio.shape))
    return float(ratio.reshape(-1)[flat]), idx


def assert_within(out, ref, bound, what=""):
    """Fail with the worst err/bound ratio and its (b, h, d) index; return
    that ratio."""
    out = out.detach().cpu()
    worst, idx = error_ratio(out, ref, bound)
    assert worst <= 1.0, (
        f"{what}: worst err/bound = {worst:.3g} at (b, h, d) = {idx}: "
        f"out {float(out[idx]):.6g}, ref {float(ref[idx]):.6g}, "
        f"bound {float(bound[idx]):.3g}"
    )
    return worst


# --------------------------------------------------------------------------
# case builders
# --------------------------------------------------------------------------

def _case(q, k, v, lens, **extra):
    return SimpleNamespace(
        q=q.contiguous(), k=k.contiguous(), v=v.contiguous(),
        lens=torch.as_tensor(lens, dtype=torch.int32), scale=SCALE,
        fp8=k.dtype == FP8, **extra)


def sentinel_case(B, Hq, Hk, S, lens, dtype, seed, score_gain):
    """Random q, k, v with q scaled by `score_gain` (score std ~ gain: 1 is
    a nearly uniform softmax, 6 a peaked one whose running max moves by tens
    between tiles). V dims 0..2 are reserved, zero except
      dim 0 = 256 at row 0,
      dim 1 = 256 at row lens[b]-1 (the newest row),
      dim 2 = 256 at row lens[b]   (the first dead row, if it exists).
    256 is exact in bf16 and e4m3. A dropped newest row zeroes dim 1 (100 %
    error); one dead row read lights dim 2, whose bound is exactly 0."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Hq, D, generator=g) * score_gain).to(BF16)
    k = torch.randn(B, Hk, S, D, generator=g).to(BF16)
    v = torch.randn(B, Hk, S, D, generator=g).to(BF16)
    v[..., :3] = 0
    for b, n in enumerate(int(x) for x in lens):
        if n > 0:
            v[b, :, 0, 0] = 256
            v[b, :, n - 1, 1] = 256
        if n < S:
            v[b, :, n, 2] = 256
    return _case(q, k.to(dtype), v.to(dtype), lens)


def census_case(ctx, S, G, dtype, seed=0):
    """K = 0, so every score is 0 and p = 1/ctx exactly. V[t, t % 128] is a
    power of two c and 0 elsewhere (dead rows included), so output dim d is
    c/ctx times the number of live positions = d (mod 128): one position
    lost, duplicated or mis-assigned anywhere changes one count by 1 in
    ceil(ctx/128) - 6 % at ctx = 2000, about 8x the bound. c =
    2^ceil(log2 ctx), capped at 256 for e4m3 caches (448 is that format's
    largest value); the bound is relative, so the cap costs nothing."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, G, D, generator=g).to(BF16)
    k = torch.zeros(1, 1, S, D, dtype=BF16)
    c = 2.0 ** math.ceil(math.log2(ctx))
    if dtype == FP8:
        c = min(c, 256.0)
    v = torch.zeros(1, 1, S, D, dtype=BF16)
    t = torch.arange(S)
    v[0, 0, t, t % D] = c
    return _case(q, k.to(dtype), v.to(dtype), [ctx])


def prefill_census_case(B, Hq, Hk, S, dtype, seed=0):
    """Causal census: query row i must count the positions <= i per residue.
    Rows >= S of the cache carry the same pattern, so a read past S shows."""
    g = torch.Generator().manual_seed(seed)
    S_max = S + 8
    q = torch.randn(B * S, Hq, D, generator=g).to(BF16)
    k = torch.zeros(B, Hk, S_max, D, dtype=BF16)
    v = torch.zeros(B, Hk, S_max, D, dtype=BF16)
    t = torch.arange(S_max)
    v[:, :, t, t % D] = 256.0
    return SimpleNamespace(q=q, k=k.to(dtype), v=v.to(dtype), batch=B, seq=S,
                           scale=SCALE, fp8=dtype == FP8)


def prefill_sentinel_case(B, Hq, Hk, S, dtype, seed, score_gain=6.0):
    """Random causal case with a peaked softmax. V dim 0 is 256 on the rows
    at even positions and dim 1 on those at odd ones (0 otherwise). Query
    row i's newest key is row i itself, so out[i, i % 2] carries
    p_ii * 256 and loses it under a strict mask; row i+1 has the other
    parity and must add nothing there (for row 0, dim 1 has bound 0). Dim 2
    is 256 on the cache rows >= S only: its bound is 0 everywhere."""
    g = torch.Generator().manual_seed(seed)
    S_max = S + 8
    q = (torch.randn(B * S, Hq, D, generator=g) * score_gain).to(BF16)
    k = torch.randn(B, Hk, S_max, D, generator=g).to(BF16)
    v = torch.randn(B, Hk, S_max, D, generator=g).to(BF16)
    v[..., :3] = 0
    t = torch.arange(S_max)
    v[:, :, t, t % 2] = 256.0
    v[:, :, S:, 2] = 256.0        # dead rows light dim 2, whose bound is 0
    return SimpleNamespace(q=q, k=k.to(dtype), v=v.to(dtype), batch=B, seq=S,
                           scale=SCALE, fp8=dtype == FP8)


def ramp_peak_pos(num_splits: int) -> int:
    """A position inside a middle tile that a middle split owns (tiles are
    interleaved: tile j belongs to split j % num_splits)."""
    tile = num_splits + num_splits // 2 if num_splits > 1 else 2
    return tile * TILE + 20


def ramp_case(direction, S, G=4, seed=0, peak_pos=None, span=60.0):
    """All q heads of the group share one unit direction u, with per-head
    gains 0.5 .. 1.5; K[t] = r(t) u + small noise, so head h's scaled score
    is gain_h r(t): monotone over `span` (x gain).
      "up":   r rises with position - corr = exp(m - m_new) << 1 on every
              tile, and for the larger gains the earliest tiles' share
              underflows to 0;
      "down": r falls - corr = 1 always, p underflows instead;
      "peak": r peaks at `peak_pos`, in a middle tile of a middle split.
    A kernel that rescales the accumulator wrongly across tiles, or merges
    splits without exp(m_w - M), is off by orders of magnitude here. bf16
    caches only; ctx = S - 3 leaves a partial last tile and dead rows."""
    g = torch.Generator().manual_seed(seed)
    ctx = S - 3
    u = torch.randn(D, generator=g)
    u = u / u.norm()
    gains = torch.linspace(0.5, 1.5, G) if G > 1 else torch.ones(1)
    q = (gains[:, None] * math.sqrt(D) * u[None, :]).reshape(1, G, D).to(BF16)
    t = torch.arange(S, dtype=torch.float32)
    if direction == "up":
        r = span * t / (ctx - 1)
    elif direction == "down":
        r = span * (1 - t / (ctx - 1))
    else:
        far = max(peak_pos, ctx - 1 - peak_pos)
        r = span * (1 - (t - peak_pos).abs() / far)
    k = r[:, None] * u[None, :] + 0.05 * torch.randn(S, D, generator=g)
    v = torch.randn(1, 1, S, D, generator=g).to(BF16)
    return _case(q, k.reshape(1, 1, S, D).to(BF16), v, [ctx])


def poison_dead_rows(k, v, lens, kind):
    """Copies of the caches with every row >= lens[b] overwritten: "nan"
    (bf16 NaN / the e4m3fn byte 0x7f), "max" (largest finite value) or
    "zero"."""
    S = k.shape[2]
    dead = (torch.arange(S)[None, :]
            >= torch.as_tensor(lens).long().reshape(-1, 1))      # [B, S]
    dead = dead[:, None, :, None].expand(k.shape)
    out = []
    for t in (k, v):
        t = t.clone()
        if t.dtype == FP8:
            byte = {"nan": 0x7F, "max": 0x7E, "zero": 0x00}[kind]
            t.view(torch.uint8)[dead] = byte
        else:
            val = {"nan": math.nan, "max": torch.finfo(t.dtype).max,
                   "zero": 0.0}[kind]
            t[dead] = val
        out.append(t)
    return out


# --------------------------------------------------------------------------
# the case lists of the GPU tests (cached: built once per process)
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_case(G, dtype, gain):
    """Tile-edge sentinel batch: one row per length in EDGE_LENS."""
    return sentinel_case(len(EDGE_LENS), G, 1, EDGE_S, EDGE_LENS, dtype,
                         seed=100 + G, score_gain=gain)


def grid_lens(S):
    return [1, min(65, S), S // 2 + 1, S]


@functools.lru_cache(maxsize=None)
def grid_case(S, dtype, gain, G=4):
    """Split-grid sentinel batch: ctx << max_seq (most splits empty) up to
    the full cache."""
    return sentinel_case(4, G, 1, S, grid_lens(S), dtype, seed=S,
                         score_gain=gain)


@functools.lru_cache(maxsize=None)
def empty_case(S, dtype):
    return sentinel_case(4, 4, 1, S, [0, 7, 0, S], dtype, seed=7 + S,
                         score_gain=6.0)


@functools.lru_cache(maxsize=None)
def poison_case(S, dtype):
    """lens strictly inside a tile and < S."""
    lens = [5, min(S - 30, 100), S - 30, S - 1]
    return sentinel_case(4, 4, 1, S, lens, dtype, seed=31 + S,
                         score_gain=6.0)


@functools.lru_cache(maxsize=None)
def cached_ref(case_fn, *args):
    """(case, ref, absref) of a cached case builder, computed once."""
    c = case_fn(*args)
    ref, absref = decode_ref64(c.q, c.k, c.v, c.lens, c.scale, q_fp8=c.fp8)
    return c, ref, absref
