"""Float64 oracles, derived error bounds and adversarial case builders for
the routed-MoE kernels (csrc/moe.hip): the route (top-k + counting sort),
the grouped gate_up + SwiGLU GEMM and the grouped split-K down GEMM with its
combine.

Plain helper module: torch on CPU only, no GPU calls, everything seeded. The
GPU tests in test_moe_edges_gpu.py run the kernels on these cases; the CPU
tests in test_moe_oracle_cpu.py prove, with mutants of a float32 emulation
of the kernels' structure, that the cases plus the bounds reject a subtly
wrong kernel.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch

from attn_oracle import BF16, error_ratio, f64  # noqa: F401
from dense_oracle import assert_equal, assert_within  # noqa: F401

# --------------------------------------------------------------------------
# launch heuristics: Python ports of the extern "C" helpers of moe.hip
# --------------------------------------------------------------------------

KT = 128                    # k elements per unrolled block
BM = 64                     # sorted rows per m-tile
NT = 64                     # W rows per workgroup per n-subtile
MAX_WGS = 1792              # workgroups the split heuristic fills


def num_m_tiles(TK: int, E: int) -> int:
    """moe_num_m_tiles: static bound on the non-empty m-tiles."""
    return min(TK, TK // BM + E)


def down_nsub(TK: int) -> int:
    """moe_down_nsub: n-subtiles per wave of the down GEMM."""
    return 2 if TK > 16 else 1


def down_num_splits(TK: int, E: int, H: int, I: int) -> int:
    """moe_down_num_splits. Only the CPU emulation and the case builders
    split by it; the GPU tests assert literal counts against the
    extension's own answer."""
    nt = NT * down_nsub(TK)
    wgs = -(-H // nt) * num_m_tiles(TK, E)
    chunks = I // KT
    sk = 1
    while sk < 16 and wgs * sk * 2 <= MAX_WGS and chunks % (sk * 2) == 0:
        sk *= 2
    return sk


def live_tiles(counts) -> int:
    """m-tiles that a routing with these per-expert row counts fills."""
    return sum(-(-c // BM) for c in counts)


# --------------------------------------------------------------------------
# routings
# --------------------------------------------------------------------------

EDGE_A = (0, 1, 15, 16, 17, 63, 64, 64)          # E = 8, K = 2, T = 120
EDGE_B = (65, 127, 128, 129, 0, 0, 1, 2)         # E = 8, K = 2, T = 226
BOUND_TIGHT = (65, 65, 65, 65)                   # E = 4, K = 2, T = 130
ONE_EACH = (1,) * 64                             # E = 64, K = 8, T = 8
LAST_ONLY = (0,) * 63 + (72,)                    # E = 64, K = 8, T = 9
ONE_TOKEN = (0, 1, 0, 1)                         # E = 4, K = 2, T = 1
NSUB1_TILES = (1, 5, 3, 7)                       # E = 4, K = 2, T = 8

# name -> (per-expert row counts, top_k)
ROUTINGS = {
    "EDGE_A": (EDGE_A, 2), "EDGE_B": (EDGE_B, 2),
    "BOUND_TIGHT": (BOUND_TIGHT, 2), "ONE_EACH": (ONE_EACH, 8),
    "LAST_ONLY": (LAST_ONLY, 8), "ONE_TOKEN": (ONE_TOKEN, 2),
    "NSUB1_TILES": (NSUB1_TILES, 2),
}
MAIN_ROUTINGS = ("EDGE_A", "EDGE_B", "BOUND_TIGHT", "ONE_EACH", "LAST_ONLY")

# (T, K, E, H, I) -> split count of the down GEMM, evaluated by hand from
# the heuristic; the port above and the binding are both held to it.
SPLIT_TABLE = {
    (120, 2, 8, 144, 896): 1,      # 7 blocks per split
    (120, 2, 8, 144, 1792): 2,     # 7
    (120, 2, 8, 144, 3072): 8,     # 3
    (120, 2, 8, 144, 2048): 16,    # 1
    (1, 2, 4, 160, 2048): 16,
    (8, 2, 4, 16, 896): 1,         # NSUB = 1, four tiles
}


def routing_from_counts(counts, top_k, seed=0):
    """(topk_w [T, K] fp32, expert_offsets [E + 1] i32, sorted_slots [T K]
    i32) for arbitrary per-expert row counts: a seeded permutation deals the
    T K slots out to the experts, and the slots of one expert ascend (the
    contract of the sort). topk_w is a seeded softmax. The GEMM kernels
    never look at which experts a token's slots went to, so two slots of one
    token may share an expert here, which no real top-k produces."""
    counts = [int(c) for c in counts]
    TK = sum(counts)
    assert TK % top_k == 0 and TK > 0
    g = torch.Generator().manual_seed(seed + 1000 * len(counts) + TK)
    perm = torch.randperm(TK, generator=g)
    offsets = torch.zeros(len(counts) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor(counts), 0)
    slots = torch.empty(TK, dtype=torch.int64)
    for e in range(len(counts)):
        lo, hi = int(offsets[e]), int(offsets[e + 1])
        slots[lo:hi] = torch.sort(perm[lo:hi]).values
    assert torch.equal(torch.sort(slots).values, torch.arange(TK))
    topk_w = torch.softmax(
        torch.randn(TK // top_k, top_k, generator=g), dim=-1)
    return (topk_w.contiguous(), offsets.to(torch.int32),
            slots.to(torch.int32))


@functools.lru_cache(maxsize=None)
def routing(name, seed=0):
    """The named routing as a namespace: counts, E, K, T, TK, topk_w,
    offsets, slots, expert_of_pos [TK], pos_of_slot [TK]. BOUND_TIGHT
    asserts that it fills the static tile grid to the last tile."""
    counts, K = ROUTINGS[name]
    topk_w, offsets, slots = routing_from_counts(counts, K, seed)
    TK = sum(counts)
    E = len(counts)
    expert_of_pos = torch.repeat_interleave(
        torch.arange(E), torch.tensor(counts))
    pos_of_slot = torch.empty(TK, dtype=torch.int64)
    pos_of_slot[slots.long()] = torch.arange(TK)
    assert live_tiles(counts) <= num_m_tiles(TK, E)
    if name in ("BOUND_TIGHT", "ONE_EACH"):
        assert live_tiles(counts) == num_m_tiles(TK, E)
    return SimpleNamespace(
        name=name, counts=counts, E=E, K=K, T=TK // K, TK=TK, topk_w=topk_w,
        offsets=offsets, slots=slots, expert_of_pos=expert_of_pos,
        pos_of_slot=pos_of_slot)


def dyadic_weights(T, K, seed=0):
    """topk_w whose products and sums with integers are exact: K = 2 rows
    cycle through (1/2, 1/2), (3/4, 1/4), (1, 0); K = 8 rows are seeded
    eighths that sum to 1 (some of them 0); any other K is 1/K-free: one-hot
    rows cycling over the k-slots."""
    g = torch.Generator().manual_seed(seed + T + K)
    if K == 2:
        pats = torch.tensor([[0.5, 0.5], [0.75, 0.25], [1.0, 0.0]])
        return pats[torch.arange(T) % 3].contiguous()
    if K == 8:
        w = torch.zeros(T, K)
        for t in range(T):
            cuts = torch.randint(0, K, (8,), generator=g)
            w[t] = torch.bincount(cuts, minlength=K).float() / 8
        return w
    w = torch.zeros(T, K)
    w[torch.arange(T), torch.arange(T) % K] = 1.0
    return w


# --------------------------------------------------------------------------
# float64 references and bounds of the two GEMMs
# --------------------------------------------------------------------------

def gate_up_parts64(x, w, r):
    """(g, u, absg, absu), float64 [TK, I] in sorted order: the two dot
    products of every routed row and their sums of magnitudes."""
    I = w.shape[1] // 2
    tokens = torch.div(r.slots.long(), r.K, rounding_mode="floor")
    xs = f64(x)[tokens]                                    # [TK, H]
    gu = torch.zeros(r.TK, 2 * I, dtype=torch.float64)
    ab = torch.zeros(r.TK, 2 * I, dtype=torch.float64)
    offs = r.offsets.tolist()
    for e in range(r.E):
        lo, hi = offs[e], offs[e + 1]
        if hi > lo:
            we = f64(w[e])
            gu[lo:hi] = xs[lo:hi] @ we.t()
            ab[lo:hi] = xs[lo:hi].abs() @ we.abs().t()
    return gu[:, :I], gu[:, I:], ab[:, :I], ab[:, I:]


def silu64(g):
    return g / (1 + torch.exp(-g))


def gate_up_ref64(x, w, r):
    g, u, _, _ = gate_up_parts64(x, w, r)
    return silu64(g) * u


SWIGLU_REL = 2.0 ** -8 + 2.0 ** -12


def gate_up_bound(x, w, r):
    """(ref, bound) of the bounded gate_up family.

    Products of bf16 values are exact in float32; g and u are each H
    accumulations in some order (the MFMA's internal adds included, hence
    the + 16 of the skinny-GEMM bound), each off by at most 2^-23 of a
    running sum that absg / absu bound: dg = (H + 16) 2^-23 absg, du
    likewise. silu has |silu'| <= 1.1, so silu(g + dg) is within 1.1 dg of
    silu(g), and the product moves by at most 1.1 dg (|u| + du) +
    |silu(g)| du. The epilogue itself (expf, one add, one divide, one
    multiply in float32) gets 2^-12 |ref|, the SwiGLU term of dense_oracle;
    the bf16 output rounding 2^-8 |ref| and no margin. No absolute floor."""
    H = x.shape[1]
    g, u, absg, absu = gate_up_parts64(x, w, r)
    ref = silu64(g) * u
    dg = (H + 16) * 2.0 ** -23 * absg
    du = (H + 16) * 2.0 ** -23 * absu
    bound = (SWIGLU_REL * ref.abs() + 1.1 * dg * (u.abs() + du)
             + silu64(g).abs() * du)
    return ref, bound


def down_ref64(act, w, topk_w, r):
    """(ref, absref), float64 [T, H]: sum_k w_k (act[pos(t, k)] . W[e]^T)
    and the same over magnitudes."""
    H = w.shape[1]
    y = torch.zeros(r.TK, H, dtype=torch.float64)
    ya = torch.zeros(r.TK, H, dtype=torch.float64)
    offs = r.offsets.tolist()
    a = f64(act)
    for e in range(r.E):
        lo, hi = offs[e], offs[e + 1]
        if hi > lo:
            we = f64(w[e])
            y[lo:hi] = a[lo:hi] @ we.t()
            ya[lo:hi] = a[lo:hi].abs() @ we.abs().t()
    tw = topk_w.double()[:, :, None]
    ys = y[r.pos_of_slot].reshape(r.T, r.K, H)
    yas = ya[r.pos_of_slot].reshape(r.T, r.K, H)
    return (ys * tw).sum(1), (yas * tw.abs()).sum(1)


def down_bound(ref, absref, I, K):
    """2^-8 |ref| + (I + 16 + K) 2^-23 absref: the skinny-GEMM bound (I
    accumulations in any order and at most 15 split-merge additions, each
    off by at most 2^-23 of a running sum that absref bounds) plus the K
    multiply-adds of the combine. One bf16 output rounding, no margin, no
    absolute floor. A workspace kept in bf16 adds 2^-9 of a partial per
    split, which the cancelling family puts far outside this."""
    return 2.0 ** -8 * ref.abs() + (I + 16 + K) * 2.0 ** -23 * absref


# --------------------------------------------------------------------------
# gate_up families
# --------------------------------------------------------------------------

PROBE_H = (128, 384, 896)               # 1, 3 and 7 K blocks
PROBE_I = (16, 48, 160)
INT_H = 384
INT_I = (16, 160)
SAT_GATES = (-100.0, -1000.0, 1000.0)   # all exact in bf16
SAT_H, SAT_I = 128, 48
BOUNDED_GATE_UP = ("EDGE_B", 896, 160)


@functools.lru_cache(maxsize=None)
def gate_up_probe_case(H, I):
    """Routing EDGE_A. Gate weights are seeded from {32, 64, 128}: expf(-g)
    < 2^-25, 1 + e = 1 and silu(g) = g exactly in float32. Up weights are
    randn cast to bf16. Launch r has x[t] one-hot (1.0) at k = (r T + t)
    mod H, r = 0 .. ceil(H / T) - 1, so every k is hit; act[p, n] must then
    equal w_gate[e, n, k] w_up[e, n, k] bit for bit (a power of two times a
    bf16 value)."""
    r = routing("EDGE_A")
    g = torch.Generator().manual_seed(H * 7 + I)
    gate = torch.tensor([32.0, 64.0, 128.0])[
        torch.randint(0, 3, (r.E, I, H), generator=g)]
    up = torch.randn(r.E, I, H, generator=g)
    w = torch.cat([gate, up], dim=1).to(BF16).contiguous()
    return SimpleNamespace(r=r, w=w, H=H, I=I, launches=-(-H // r.T))


def gate_up_probe_x(c, launch):
    x = torch.zeros(c.r.T, c.H, dtype=BF16)
    t = torch.arange(c.r.T)
    x[t, (launch * c.r.T + t) % c.H] = 1
    return x


def gate_up_probe_expected(c, launch):
    r = c.r
    t = torch.div(r.slots.long(), r.K, rounding_mode="floor")
    k = (launch * r.T + t) % c.H                            # [TK]
    col = f64(c.w[r.expert_of_pos, :, k])                   # [TK, 2I]
    prod = col[:, :c.I] * col[:, c.I:]
    expect = prod.to(BF16)
    assert torch.equal(f64(expect), prod)
    return expect


def integer_rows(rows, width, seed):
    """[rows, width] with at most 16 nonzeros in {+-1, +-2} per row: k = 0
    and k = width - 1 (so the first and the last split see every row), 10
    of the first and last k of the 32-subtiles (which include those of the
    128-blocks), taken in turn so that the rows together cover all of them,
    and 4 seeded positions."""
    g = torch.Generator().manual_seed(seed)
    edges = sorted({32 * j for j in range(width // 32)}
                   | {32 * j + 31 for j in range(width // 32)})
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])
    x = torch.zeros(rows, width)
    for m in range(rows):
        pos = {edges[(10 * m + j) % len(edges)] for j in range(10)}
        pos |= {0, width - 1}
        pos |= set(torch.randperm(width, generator=g)[:4].tolist())
        pos = torch.tensor(sorted(pos))
        assert len(pos) <= 16
        x[m, pos] = vals[torch.randint(0, 4, (len(pos),), generator=g)]
    return x


@functools.lru_cache(maxsize=None)
def gate_up_integer_case(name, I, H=INT_H):
    """Integer x rows (integer_rows) against dense w in {-2 .. 2}: sum |x|
    |w| <= 64 (asserted), so g and u are exact integers in float32 whatever
    the order, and the output is within (2^-8 + 2^-12) |ref|, the SwiGLU
    bound of dense_oracle. A lost or duplicated product moves g or u by at
    least 1, far outside it."""
    r = routing(name)
    g = torch.Generator().manual_seed(len(name) + 31 * I + H)
    x = integer_rows(r.T, H, seed=I + H + r.T).to(BF16)
    w = torch.randint(-2, 3, (r.E, 2 * I, H), generator=g).to(BF16)
    gg, uu, absg, absu = gate_up_parts64(x, w, r)
    assert float(torch.maximum(absg, absu).max()) <= 64
    ref = silu64(gg) * uu
    return SimpleNamespace(r=r, x=x, w=w, H=H, I=I, ref=ref,
                           bound=SWIGLU_REL * ref.abs())


@functools.lru_cache(maxsize=None)
def gate_up_saturation_case():
    """Routing EDGE_A, H = 128, I = 48. Gate row n is SAT_GATES[n mod 3] at
    every k and x[t] is one-hot, so g is exactly -100, -1000 or +1000: e^-g
    overflows for the first two (the output must be finite and below 2^-126
    in magnitude) and underflows for the last, where silu(g) = g and the
    output must equal bf16(1000 u); up rows with n mod 6 = 2 are all 1, so
    those outputs are exactly 1000."""
    r = routing("EDGE_A")
    g = torch.Generator().manual_seed(5)
    n = torch.arange(SAT_I)
    gate = torch.tensor(SAT_GATES)[n % 3][None, :, None].expand(
        r.E, SAT_I, SAT_H)
    up = torch.randn(r.E, SAT_I, SAT_H, generator=g)
    up[:, n % 6 == 2, :] = 1.0
    w = torch.cat([gate, up], dim=1).to(BF16).contiguous()
    x = torch.zeros(r.T, SAT_H, dtype=BF16)
    t = torch.arange(r.T)
    x[t, (7 * t) % SAT_H] = 1
    tok = torch.div(r.slots.long(), r.K, rounding_mode="floor")
    u = f64(w[r.expert_of_pos, SAT_I:, (7 * tok) % SAT_H])   # [TK, I]
    big = (n % 3 == 2)
    expect_big = (1000.0 * u[:, big]).to(BF16)
    assert bool((expect_big[:, (n[big] % 6 == 2)] == 1000).all())
    return SimpleNamespace(r=r, x=x, w=w, big=big, expect_big=expect_big)


def check_saturation(out, c, what="saturation"):
    out = out.detach().cpu()
    assert bool(torch.isfinite(out.float()).all()), f"{what}: not finite"
    small = out[:, ~c.big].float().abs()
    assert float(small.max()) < 2.0 ** -126, (what, float(small.max()))
    assert_equal(out[:, c.big], c.expect_big, what)


@functools.lru_cache(maxsize=None)
def gate_up_bounded_case():
    name, H, I = BOUNDED_GATE_UP
    r = routing(name)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(r.T, H, generator=g).to(BF16)
    w = (torch.randn(r.E, 2 * I, H, generator=g) / H ** 0.5).to(BF16)
    ref, bound = gate_up_bound(x, w, r)
    return SimpleNamespace(r=r, x=x, w=w, H=H, I=I, ref=ref, bound=bound)


# --------------------------------------------------------------------------
# down + combine families
# --------------------------------------------------------------------------

# (routing, H, I) -> literal split count
DOWN_PROBE = {("EDGE_A", 144, 896): 1, ("EDGE_A", 144, 3072): 8,
              ("ONE_EACH", 16, 896): 1}
DOWN_INTEGER = {
    ("EDGE_A", 144, 896): 1, ("EDGE_A", 144, 1792): 2,
    ("EDGE_A", 144, 3072): 8, ("EDGE_A", 144, 2048): 16,
    ("ONE_TOKEN", 160, 2048): 16, ("NSUB1_TILES", 16, 896): 1,
    ("EDGE_B", 160, 896): 1, ("EDGE_B", 144, 1792): 2,
    ("BOUND_TIGHT", 144, 3072): 8, ("BOUND_TIGHT", 16, 896): 1,
    ("ONE_EACH", 16, 1792): 2, ("LAST_ONLY", 160, 256): 2,
}
DOWN_BOUNDED = {("EDGE_A", 144, 1792): 2, ("EDGE_A", 144, 3072): 8}
DOWN_CANCEL = {("EDGE_A", 144, 768): 2, ("EDGE_A", 144, 1024): 8}
DETERMINISM = (("EDGE_A", 144, 3072), ("BOUND_TIGHT", 144, 3072))


def case_splits(name, H, I):
    r = routing(name)
    return down_num_splits(r.TK, r.E, H, I)


def table_key(name, H, I):
    r = routing(name)
    return (r.T, r.K, r.E, H, I)


@functools.lru_cache(maxsize=None)
def down_probe_case(name, H, I):
    """Launch r has act[p] one-hot (1.0) at k = (r TK + p) mod I, r = 0 ..
    ceil(I / TK) - 1, so every k is hit, and topk_w[t] one-hot in k-slot r
    mod K: out[t] must be column k of w_down[e] for the one visible slot of
    t, bit for bit. The zero weight multiplies the other slots' workspace
    rows, so an unwritten row that holds NaN shows."""
    r = routing(name)
    g = torch.Generator().manual_seed(H + I)
    w = torch.randn(r.E, H, I, generator=g).to(BF16)
    return SimpleNamespace(r=r, w=w, H=H, I=I, splits=case_splits(name, H, I),
                           launches=-(-I // r.TK))


def down_probe_inputs(c, launch):
    r = c.r
    act = torch.zeros(r.TK, c.I, dtype=BF16)
    p = torch.arange(r.TK)
    act[p, (launch * r.TK + p) % c.I] = 1
    topk_w = torch.zeros(r.T, r.K)
    topk_w[:, launch % r.K] = 1.0
    return act, topk_w


def down_probe_expected(c, launch):
    r = c.r
    slot = torch.arange(r.T) * r.K + launch % r.K
    p = r.pos_of_slot[slot]
    k = (launch * r.TK + p) % c.I
    return c.w[r.expert_of_pos[p], :, k].contiguous()       # [T, H] bf16


def down_probe_launches_cpu(c):
    """All launches when few, else the first, the last and one middle
    launch that makes the last k-slot the visible one."""
    if c.launches <= 6:
        return list(range(c.launches))
    mid = c.launches // 2
    last_k = [r for r in range(mid, c.launches) if r % c.r.K == c.r.K - 1]
    return sorted({0, last_k[0] if last_k else mid, c.launches - 1})


@functools.lru_cache(maxsize=None)
def down_integer_case(name, H, I):
    """act as integer_rows, w in {-2 .. 2}, dyadic topk_w: every product,
    partial and sum is exact in float32 (|y| <= 64, weights in eighths), so
    the output must torch.equal the float64 reference cast to bf16."""
    r = routing(name)
    g = torch.Generator().manual_seed(len(name) + H + 3 * I)
    act = integer_rows(r.TK, I, seed=H + I + r.TK).to(BF16)
    w = torch.randint(-2, 3, (r.E, H, I), generator=g).to(BF16)
    topk_w = dyadic_weights(r.T, r.K, seed=H)
    ref, absref = down_ref64(act, w, topk_w, r)
    assert float(absref.max()) <= 64
    assert torch.equal(ref.float().double(), ref)
    return SimpleNamespace(r=r, act=act, w=w, topk_w=topk_w, H=H, I=I,
                           splits=case_splits(name, H, I), ref=ref,
                           expect=ref.to(BF16))


def _down_case(r, act, w, name, H, I):
    ref, absref = down_ref64(act, w, r.topk_w, r)
    return SimpleNamespace(r=r, act=act, w=w, topk_w=r.topk_w, H=H, I=I,
                           splits=case_splits(name, H, I), ref=ref,
                           bound=down_bound(ref, absref, I, r.K))


@functools.lru_cache(maxsize=None)
def down_bounded_case(name, H, I):
    """randn act against randn / sqrt(I) weights, seeded softmax topk_w."""
    r = routing(name)
    g = torch.Generator().manual_seed(H + I + 11)
    act = torch.randn(r.TK, I, generator=g).to(BF16)
    w = (torch.randn(r.E, H, I, generator=g) / I ** 0.5).to(BF16)
    return _down_case(r, act, w, name, H, I)


@functools.lru_cache(maxsize=None)
def down_cancel_case(name, H, I):
    """The two halves of I nearly cancel, as in dense_oracle.cancel_case:
    act = [a, -a], w = [w1, w1 + 2^-4 noise]. The split partials are ~16x
    the result, so 2^-8 |ref| is small and the bound is its float32 term: a
    workspace or partial rounded to bf16 (2^-9 of a partial each) is
    several times that. Same bound as the bounded family."""
    r = routing(name)
    g = torch.Generator().manual_seed(H + I + 12)
    h = I // 2
    a = torch.randn(r.TK, h, generator=g)
    w1 = torch.randn(r.E, H, h, generator=g) / I ** 0.5
    w2 = w1 + 2.0 ** -4 / I ** 0.5 * torch.randn(r.E, H, h, generator=g)
    act = torch.cat([a, -a], dim=1).to(BF16)
    w = torch.cat([w1, w2], dim=2).to(BF16)
    return _down_case(r, act, w, name, H, I)


# --------------------------------------------------------------------------
# route
# --------------------------------------------------------------------------

# (T, E, K): n = T K hits 1, 255, 256, 257, 511, 512, 513 and 4096 (the
# sort's 256 threads own ceil(n / 256) slots each: the ownership edges), E
# hits 1, 3, 8 and 64, K hits 1 and E
ROUTE_SHAPES = ((1, 1, 1), (255, 3, 1), (85, 64, 3), (128, 8, 2),
                (257, 3, 1), (511, 8, 1), (64, 8, 8), (171, 3, 3),
                (512, 64, 8))
ROUTE_KINDS = ("ties", "negative", "inf_cut", "inf_sel")
# largest |sel - max| of any finite selected logit in the cases below
ROUTE_MAX_GAP = 6.0


def route_logits(T, E, K, kind, seed=0):
    """Integer-valued logits from a small set, so ties are everywhere,
    the K cut included. "ties": {-3 .. 3}. "negative": {-6 .. -1} (the
    argmax must not start from 0). "inf_cut": each row keeps K seeded
    finite entries and has -inf in the other E - K (the cut runs between
    the finite and the masked ones). "inf_sel": -inf in E - K + 1 entries,
    which puts one -inf into the selection, with weight exactly 0; needs K
    >= 2 (returns None otherwise). NaN logits and rows that are all -inf
    are outside the kernel's contract and are not built."""
    g = torch.Generator().manual_seed(seed + 13 * T + 7 * E + K)
    if kind == "negative":
        return torch.randint(-6, 0, (T, E), generator=g).float()
    logits = torch.randint(-3, 4, (T, E), generator=g).float()
    if kind == "ties":
        return logits
    masked = E - K if kind == "inf_cut" else E - K + 1
    if kind == "inf_sel" and K < 2:
        return None
    for t in range(T):
        idx = torch.randperm(E, generator=g)[:masked]
        logits[t, idx] = float("-inf")
    return logits


def route_ref64(logits, K):
    """(topk_idx i32 [T, K], topk_w float64 [T, K], offsets i32 [E + 1],
    slots i32 [T K], rel [T, K]): the selection of a stable descending sort
    (lowest index first among equals, -inf included), the float64 softmax
    over the selected logits, the stable sort of the slots by expert, and
    the relative bound of route_weight_bound."""
    E = logits.shape[1]
    vals, idx = torch.sort(logits.double(), dim=-1, descending=True,
                           stable=True)
    vals, idx = vals[:, :K], idx[:, :K]
    gap = vals - vals[:, :1]                  # <= 0, -inf for a masked one
    ex = torch.exp(gap)
    w = ex / ex.sum(dim=1, keepdim=True)
    flat = idx.reshape(-1)
    slots = torch.sort(flat, stable=True).indices
    offsets = torch.zeros(E + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(flat, minlength=E), 0)
    return (idx.to(torch.int32).contiguous(), w, offsets.to(torch.int32),
            slots.to(torch.int32), route_weight_bound(gap, K))


EXPF_ULP = 1.0      # HIP's documented maximum error of expf, in ulp


def route_weight_bound(gap, K):
    """Relative bound on w_k = e_k / sum_j e_j, e_j = expf(sel_j - max),
    for finite gaps down to about -80 (e_j a normal float32).

    - the subtraction is rounded to float32: the argument of expf is off by
      at most 2^-24 |gap_j|, which is a relative error of e_j of 2^-24
      |gap_j| (d exp(x) / exp(x) = dx);
    - expf is within EXPF_ULP ulp, at most EXPF_ULP 2^-23 relative;
      together a_j = 2^-24 |gap_j| + EXPF_ULP 2^-23;
    - the denominator is a sum of positive terms: the relative error of its
      terms carries over as at most max_j a_j, and its K - 1 float32
      additions add (K - 1) 2^-24;
    - the division is correctly rounded: 2^-24.
    rel_k = a_k + max_j a_j + K 2^-24, first order; the second-order terms
    are below 2^-44. A selected -inf has e = 0 exactly: reference 0, bound
    0, and it takes no part in max_j."""
    a = 2.0 ** -24 * gap.abs() + EXPF_ULP * 2.0 ** -23
    a = torch.where(torch.isfinite(gap), a, torch.zeros_like(a))
    return a + a.max(dim=1, keepdim=True).values + K * 2.0 ** -24


def check_route(out, logits, K, what="route"):
    """Indices, offsets and slots torch.equal, weights within the relative
    bound and exactly 0 where the reference is 0. Returns the worst
    err/bound of the weights."""
    idx, w, offsets, slots, rel = route_ref64(logits, K)
    o_idx, o_w, o_off, o_slots = [t.detach().cpu() for t in out]
    assert o_idx.dtype == o_off.dtype == o_slots.dtype == torch.int32
    assert o_w.dtype == torch.float32
    assert_equal(o_idx, idx, what + " topk_idx")
    assert_equal(o_off, offsets, what + " offsets")
    assert_equal(o_slots, slots, what + " slots")
    zero = w == 0
    assert bool((o_w[zero] == 0).all()), what + ": masked weight not 0"
    return assert_within(o_w, w, rel * w, what + " topk_w")


def counts_logits(counts_pairs, E, seed=0):
    """Tie-free logits [T, E] that route token t to the expert pair
    counts_pairs[t] = (first, second): 8 and 4 on the pair, distinct
    values below 0 elsewhere."""
    g = torch.Generator().manual_seed(seed)
    T = len(counts_pairs)
    base = -1.0 - 0.37 * torch.arange(E, dtype=torch.float32)
    logits = torch.stack(
        [base[torch.randperm(E, generator=g)] for _ in range(T)])
    for t, (a, b) in enumerate(counts_pairs):
        logits[t, a] = 8.0
        logits[t, b] = 4.0
    return logits
