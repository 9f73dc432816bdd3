"""CPU proof that the routed-MoE oracle (moe_oracle.py) has teeth.

A float32 emulation of the two grouped GEMMs and the combine that follows
the kernels' structure - moe_find_tile over the static tile grid, 64-row
tiles of 16-row sub-tiles, 16 NSUB-column waves, the staggered wrapping
K-block order, the (I / 128) / SK split ranges, a slot-indexed float32
workspace that starts as NaN and the combine's order - must pass every
family at every shape the GPU tests use, and each mutant of it must be
rejected by the family named in its test.
"""
import pytest
import torch

import moe_oracle as mo
from moe_oracle import BF16
from wva_amd import ops

NAN = float("nan")


def record(family, ratio, note=""):
    print(f"\n[moe-emu] family={family} ratio={ratio:.3f} {note}")


# --------------------------------------------------------------------------
# float32 emulation of the kernels, with mutants
# --------------------------------------------------------------------------

def cdiv(a, b):
    """C integer division (truncating), for row counts that a corrupt
    offset table makes negative."""
    return int(a / b)


def find_tile(offs, E, tile, mutant=None):
    """moe_find_tile: (expert, row0, rows) or None."""
    begin = offs[0]
    for e in range(E):
        end = offs[e + 1]
        n_e = end - begin
        tiles_e = cdiv(n_e + mo.BM - 1, mo.BM)
        hit = tile <= tiles_e if mutant == "tile_le" else tile < tiles_e
        if hit and begin >= 0:
            return e, begin + tile * mo.BM, min(mo.BM, n_e - tile * mo.BM)
        tile -= tiles_e
        begin = end
    return None


def stream(a, b, bx, by, k_begin, k_end, mutant=None):
    """moe_mma_stream: [rows(a), rows(b)] float32. Workgroup (bx, by)
    starts at block (5 bx + 3 by) mod nkb and wraps; a block is four
    32-wide MFMA steps. Dead rows arrive as zero rows."""
    nkb = (k_end - k_begin) // mo.KT
    start = (5 * bx + 3 * by) % nkb
    if mutant == "stagger_no_wrap":          # blocks before the start lost
        blocks = list(range(start, nkb))
    elif mutant == "no_wrap":                # runs past the end of the range
        blocks = list(range(start, start + nkb))
        pad = (0, nkb * mo.KT)
        a = torch.nn.functional.pad(a, pad)
        b = torch.nn.functional.pad(b, pad)
    else:
        blocks = [(start + i) % nkb for i in range(nkb)]
    acc = torch.zeros(a.shape[0], b.shape[0])
    for kb in blocks:
        k0 = k_begin + kb * mo.KT
        for kk in range(3 if mutant == "drop_kk" else 4):
            k = k0 + 32 * kk
            acc = acc + a[:, k:k + 32] @ b[:, k:k + 32].t()
    return acc


def tile_rows(tile, TK):
    """(p [16 mt], live [16 mt]) of a tile, or None if it owns no
    sub-tile."""
    _, row0, rows = tile
    mt = cdiv(rows + 15, 16)
    if mt <= 0:
        return None
    m = torch.arange(16 * mt)
    p = row0 + m
    return p, (m < rows) & (p < TK)


def emulate_gate_up(x, w, offsets, slots, top_k, mutant=None):
    """moe_gate_up_swiglu_kernel. Rows that no workgroup writes stay NaN."""
    T, H = x.shape
    E, I = w.shape[0], w.shape[1] // 2
    TK = T * top_k
    offs, sl = offsets.tolist(), slots.long()
    xf = x.float()
    act = torch.full((TK, I), NAN, dtype=BF16)
    grid_y = mo.num_m_tiles(TK, E) - (1 if mutant == "grid_short" else 0)
    for by in range(grid_y):
        tile = find_tile(offs, E, by, mutant)
        rows = tile and tile_rows(tile, TK)
        if not rows:
            continue
        p, live = rows
        slot = torch.where(live, sl[p.clamp(0, TK - 1)], torch.zeros(()).long())
        tok = slot if mutant == "slot_for_token" else torch.div(
            slot, top_k, rounding_mode="trunc")
        a = xf[tok.clamp(0, T - 1)] * live[:, None]
        we = w[tile[0]]
        for bx in range(-(-I // mo.NT)):
            n = torch.arange(bx * mo.NT, min(I, (bx + 1) * mo.NT))
            up_rows = n if mutant == "up_no_offset" else n + I
            g = stream(a, we[n].float(), bx, by, 0, H, mutant)
            u = stream(a, we[up_rows].float(), bx, by, 0, H, mutant)
            if mutant == "swap_gate_up":
                g, u = u, g
            val = (g / (1.0 + torch.exp(-g)) * u).to(BF16)
            act[p[live][:, None], n[None, :]] = val[live]
    return act


def emulate_down(act, w, topk_w, offsets, slots, splits, mutant=None):
    """moe_down_kernel<NSUB> + moe_combine_kernel. The workspace is flat
    [SK, TK, H] float32 that starts as NaN; a store past column H lands in
    the next row, as it would in memory."""
    TK, I = act.shape
    E, H, _ = w.shape
    T, K = topk_w.shape
    offs, sl = offsets.tolist(), slots.long()
    nsub = mo.down_nsub(TK)
    wg_cols = mo.NT * nsub
    wave_cols = 16 * nsub
    af = act.float()
    size = splits * TK * H
    ws = torch.full((size + wg_cols,), NAN)
    per = (I // mo.KT) // splits
    grid_y = mo.num_m_tiles(TK, E) - (1 if mutant == "grid_short" else 0)
    for by in range(grid_y):
        tile = find_tile(offs, E, by, mutant)
        rows = tile and tile_rows(tile, TK)
        if not rows:
            continue
        p, live = rows
        a = af[p.clamp(0, TK - 1)] * live[:, None]
        slot = sl[p.clamp(0, TK - 1)]
        ok = live & (slot >= 0) & (slot < TK)
        dst_row = p if mutant == "ws_sorted_pos" else slot
        for bx in range(-(-H // wg_cols)):
            n = bx * wg_cols + torch.arange(wg_cols)
            n_live = n < H
            # a wave whose first column is past H exits before any store
            wave_on = (n // wave_cols) * wave_cols < H
            b = w[tile[0]][n.clamp(max=H - 1)].float() * n_live[:, None]
            stored = wave_on if mutant == "dead_written" else n_live
            for sk in range(splits):
                k0 = sk * per * mo.KT
                acc = stream(a, b, bx, by, k0, k0 + per * mo.KT, mutant)
                if mutant == "ws_bf16":
                    acc = acc.to(BF16).float()
                idx = ((sk * TK + dst_row[ok])[:, None] * H
                       + n[stored][None, :])
                ws[idx] = acc[ok][:, stored]
    ws = ws[:size].reshape(splits, TK, H)
    n_k = K - 1 if mutant == "combine_drop_k" else K
    n_s = splits - 1 if mutant == "combine_drop_split" else splits
    out = torch.zeros(T, H)
    for k in range(n_k):
        s = torch.zeros(T, H)
        for sk in range(n_s):
            s = s + ws[sk, k::K]
        out = out + topk_w[:, k, None] * s
    return out.to(BF16)


def run_gate_up(c, x=None, mutant=None):
    return emulate_gate_up(c.x if x is None else x, c.w, c.r.offsets,
                           c.r.slots, c.r.K, mutant)


def run_down(c, act=None, topk_w=None, mutant=None):
    return emulate_down(c.act if act is None else act, c.w,
                        c.topk_w if topk_w is None else topk_w,
                        c.r.offsets, c.r.slots, c.splits, mutant)


def ratio(out, ref, bound):
    return mo.error_ratio(out, ref, bound)[0]


def differs(out, expect):
    return int(((out != expect) | torch.isnan(out.float())).sum())


# --------------------------------------------------------------------------
# heuristics and routings
# --------------------------------------------------------------------------

def test_split_literals_match_heuristic_port():
    for (T, K, E, H, I), n in mo.SPLIT_TABLE.items():
        assert mo.down_num_splits(T * K, E, H, I) == n, (T, K, E, H, I)
    for table in (mo.DOWN_PROBE, mo.DOWN_INTEGER, mo.DOWN_BOUNDED,
                  mo.DOWN_CANCEL):
        for key, n in table.items():
            assert mo.case_splits(*key) == n, key
    # every row of the issue's table is an integer case
    keys = {mo.table_key(*key) for key in mo.DOWN_INTEGER}
    assert set(mo.SPLIT_TABLE) <= keys
    assert mo.down_nsub(16) == 1 and mo.down_nsub(17) == 2


def test_tile_bound_is_met_and_never_exceeded():
    assert mo.num_m_tiles(260, 4) == 8 == mo.live_tiles(mo.BOUND_TIGHT)
    assert mo.num_m_tiles(64, 64) == 64 == mo.live_tiles(mo.ONE_EACH)
    assert mo.num_m_tiles(16, 4) == 4 == mo.live_tiles(mo.NSUB1_TILES)
    for name in mo.ROUTINGS:
        r = mo.routing(name)
        assert sum(r.counts) == r.T * r.K
        assert mo.live_tiles(r.counts) <= mo.num_m_tiles(r.TK, r.E), name
        # the last grid index that finds a tile is the live count - 1
        offs = r.offsets.tolist()
        live = mo.live_tiles(r.counts)
        assert find_tile(offs, r.E, live - 1) is not None
        assert find_tile(offs, r.E, live) is None


def test_routing_contract():
    for name in mo.ROUTINGS:
        r = mo.routing(name)
        offs = r.offsets.tolist()
        assert offs[0] == 0 and offs[-1] == r.TK
        for e in range(r.E):
            seg = r.slots[offs[e]:offs[e + 1]]
            assert bool((seg[1:] > seg[:-1]).all()), (name, e)
        assert torch.allclose(r.topk_w.sum(1), torch.ones(r.T))
    for T, K in ((120, 2), (8, 8), (9, 8), (5, 3)):
        w = mo.dyadic_weights(T, K)
        assert torch.equal(w.sum(1), torch.ones(T))
        assert torch.equal(w * 8, (w * 8).round())


# --------------------------------------------------------------------------
# the unmutated emulation passes every family at every GPU shape, and the
# fp32 references of ops are held to the same bounds
# --------------------------------------------------------------------------

class TestEmulationPasses:
    @pytest.mark.parametrize("I", mo.PROBE_I)
    @pytest.mark.parametrize("H", mo.PROBE_H)
    def test_gate_up_probe(self, H, I):
        c = mo.gate_up_probe_case(H, I)
        for launch in range(c.launches):
            mo.assert_equal(run_gate_up(c, mo.gate_up_probe_x(c, launch)),
                            mo.gate_up_probe_expected(c, launch),
                            f"gate_up probe launch {launch}")

    @pytest.mark.parametrize("I", mo.INT_I)
    @pytest.mark.parametrize("name", mo.MAIN_ROUTINGS)
    def test_gate_up_integer(self, name, I):
        c = mo.gate_up_integer_case(name, I)
        w = mo.assert_within(run_gate_up(c), c.ref, c.bound, "emulation")
        ref32 = ops.moe_gate_up_swiglu_ref(c.x, c.w, c.r.offsets, c.r.slots,
                                           c.r.K)
        mo.assert_within(ref32.to(BF16), c.ref, c.bound, "ops ref")
        record(f"gate_up integer {name} I={I}", w)

    def test_gate_up_saturation(self):
        c = mo.gate_up_saturation_case()
        mo.check_saturation(run_gate_up(c), c)

    def test_gate_up_bounded(self):
        c = mo.gate_up_bounded_case()
        w = mo.assert_within(run_gate_up(c), c.ref, c.bound, "emulation")
        ref32 = ops.moe_gate_up_swiglu_ref(c.x, c.w, c.r.offsets, c.r.slots,
                                           c.r.K)
        mo.assert_within(ref32.to(BF16), c.ref, c.bound, "ops ref")
        record("gate_up bounded", w)

    @pytest.mark.parametrize("key", list(mo.DOWN_PROBE))
    def test_down_probe(self, key):
        c = mo.down_probe_case(*key)
        assert c.splits == mo.DOWN_PROBE[key]
        launches = mo.down_probe_launches_cpu(c)
        assert launches[0] == 0 and launches[-1] == c.launches - 1
        for launch in launches:
            act, topk_w = mo.down_probe_inputs(c, launch)
            mo.assert_equal(run_down(c, act, topk_w),
                            mo.down_probe_expected(c, launch),
                            f"down probe launch {launch}")

    @pytest.mark.parametrize("key", list(mo.DOWN_INTEGER))
    def test_down_integer(self, key):
        c = mo.down_integer_case(*key)
        assert c.splits == mo.DOWN_INTEGER[key]
        mo.assert_equal(run_down(c), c.expect, "emulation")
        ref32 = ops.moe_down_combine_ref(c.act, c.w, c.topk_w, c.r.offsets,
                                         c.r.slots)
        mo.assert_equal(ref32.to(BF16), c.expect, "ops ref")

    @pytest.mark.parametrize("key", list(mo.DOWN_BOUNDED))
    def test_down_bounded(self, key):
        c = mo.down_bounded_case(*key)
        assert c.splits == mo.DOWN_BOUNDED[key]
        w = mo.assert_within(run_down(c), c.ref, c.bound, "emulation")
        ref32 = ops.moe_down_combine_ref(c.act, c.w, c.topk_w, c.r.offsets,
                                         c.r.slots)
        mo.assert_within(ref32.to(BF16), c.ref, c.bound, "ops ref")
        record(f"down bounded {key}", w)

    @pytest.mark.parametrize("key", list(mo.DOWN_CANCEL))
    def test_down_cancel(self, key):
        c = mo.down_cancel_case(*key)
        assert c.splits == mo.DOWN_CANCEL[key]
        w = mo.assert_within(run_down(c), c.ref, c.bound, "emulation")
        ref32 = ops.moe_down_combine_ref(c.act, c.w, c.topk_w, c.r.offsets,
                                         c.r.slots)
        mo.assert_within(ref32.to(BF16), c.ref, c.bound, "ops ref")
        record(f"down cancel {key}", w)

    @pytest.mark.parametrize("T,E,K", mo.ROUTE_SHAPES)
    def test_route_reference(self, T, E, K):
        """ops.moe_route_ref (float32 softmax) against the float64 oracle
        on every route case."""
        for kind in mo.ROUTE_KINDS:
            logits = mo.route_logits(T, E, K, kind)
            if logits is None:
                continue
            gap = torch.sort(logits, dim=-1, descending=True).values[:, :K]
            gap = (gap - gap[:, :1]).abs()
            assert float(gap[torch.isfinite(gap)].amax()) <= mo.ROUTE_MAX_GAP
            mo.check_route(ops.moe_route_ref(logits, K), logits, K,
                           f"{kind} {T, E, K}")

    def test_route_cases_hold_what_they_claim(self):
        logits = mo.route_logits(128, 8, 2, "ties")
        vals = torch.sort(logits, dim=-1, descending=True).values
        assert bool((vals[:, 1] == vals[:, 2]).any())   # a tie across the cut
        assert bool((mo.route_logits(64, 8, 8, "negative") < 0).all())
        cut = mo.route_logits(128, 8, 2, "inf_cut")
        assert bool((torch.isinf(cut).sum(1) == 6).all())
        sel = mo.route_logits(128, 8, 2, "inf_sel")
        _, w, _, _, _ = mo.route_ref64(sel, 2)
        assert bool((w[:, 1] == 0).all()) and bool((w[:, 0] == 1).all())
        assert mo.route_logits(255, 3, 1, "inf_sel") is None
        ns = {T * K for T, _, K in mo.ROUTE_SHAPES}
        assert ns == {1, 255, 256, 257, 511, 512, 513, 4096}
        assert {E for _, E, _ in mo.ROUTE_SHAPES} == {1, 3, 8, 64}


def test_clamps_on_the_emulation():
    """A corrupt routing gives wrong numbers, never an access outside the
    tensors: offsets that run past T K (p < TK) and slots outside [0, T K)
    (the token clamp of gate_up, the skipped store of down). Checked on the
    emulation only; no GPU test launches such a routing. Negative offsets
    are not covered by the kernels' guards (a skipped expert leaves a
    negative tile index behind) and are outside the contract."""
    c = mo.down_integer_case("NSUB1_TILES", 16, 896)
    good = run_down(c)
    offs = c.r.offsets.clone()
    offs[-1] += 40                                    # past T K
    out = emulate_down(c.act, c.w, c.topk_w, offs, c.r.slots, c.splits)
    mo.assert_equal(out, good, "rows past T K are dead")
    slots = c.r.slots.clone()
    victim = int(slots[3])
    slots[3] = c.r.TK + 5
    out = emulate_down(c.act, c.w, c.topk_w, offs, slots, c.splits)
    t = victim // c.r.K
    assert bool(torch.isnan(out[t].float()).all())    # its row is unwritten
    keep = torch.arange(c.r.T) != t
    mo.assert_equal(out[keep], good[keep], "other tokens")
    g = mo.gate_up_integer_case("EDGE_A", 16)
    slots = g.r.slots.clone()
    slots[5], slots[6] = -7, g.r.TK + 100
    out = emulate_gate_up(g.x, g.w, g.r.offsets, slots, g.r.K)
    assert bool(torch.isfinite(out.float()).all())


# --------------------------------------------------------------------------
# every mutant is rejected by a named family
# --------------------------------------------------------------------------

def gate_up_probe_bad(c, mutant):
    return sum(differs(run_gate_up(c, mo.gate_up_probe_x(c, launch), mutant),
                       mo.gate_up_probe_expected(c, launch))
               for launch in range(c.launches))


def down_probe_bad(c, mutant):
    bad = 0
    for launch in mo.down_probe_launches_cpu(c):
        act, topk_w = mo.down_probe_inputs(c, launch)
        bad += differs(run_down(c, act, topk_w, mutant),
                       mo.down_probe_expected(c, launch))
    return bad


class TestMutantsAreRejected:
    def test_tile_grid_one_short(self):
        """Only a routing that fills the static bound sees it."""
        for name in ("BOUND_TIGHT", "ONE_EACH"):
            c = mo.gate_up_integer_case(name, 16)
            assert ratio(run_gate_up(c, mutant="grid_short"), c.ref,
                         c.bound) > 100
        c = mo.down_integer_case("BOUND_TIGHT", 144, 3072)
        assert differs(run_down(c, mutant="grid_short"), c.expect) > 0
        # every other routing has a spare tile: the mutant is invisible
        for name in ("EDGE_A", "EDGE_B", "LAST_ONLY"):
            c = mo.gate_up_integer_case(name, 16)
            assert torch.equal(run_gate_up(c, mutant="grid_short"),
                               run_gate_up(c))

    def test_tile_scan_off_by_one(self):
        for name in ("EDGE_A", "BOUND_TIGHT"):
            c = mo.gate_up_integer_case(name, 16)
            assert ratio(run_gate_up(c, mutant="tile_le"), c.ref,
                         c.bound) > 100
        c = mo.down_integer_case("EDGE_A", 144, 896)
        assert differs(run_down(c, mutant="tile_le"), c.expect) > 0

    def test_last_subtile_of_a_block_dropped(self):
        c = mo.gate_up_probe_case(128, 16)
        assert gate_up_probe_bad(c, "drop_kk") > 0
        assert down_probe_bad(mo.down_probe_case("EDGE_A", 144, 896),
                              "drop_kk") > 0
        c = mo.gate_up_integer_case("EDGE_A", 16)
        assert ratio(run_gate_up(c, mutant="drop_kk"), c.ref, c.bound) > 1
        c = mo.down_integer_case("EDGE_A", 144, 896)
        assert differs(run_down(c, mutant="drop_kk"), c.expect) > 0

    @pytest.mark.parametrize("mutant", ["no_wrap", "stagger_no_wrap"])
    def test_k_block_order(self, mutant):
        """Needs nkb >= 2 and a workgroup whose start is not block 0: at
        nkb = 1 both mutants are the kernel, and at nkb = 3 the 3 by term
        vanishes, so only I > 64 (bx > 0) staggers there."""
        for H in (384, 896):
            assert gate_up_probe_bad(mo.gate_up_probe_case(H, 160), mutant) > 0
        assert gate_up_probe_bad(mo.gate_up_probe_case(896, 16), mutant) > 0
        assert gate_up_probe_bad(mo.gate_up_probe_case(384, 48), mutant) == 0
        assert gate_up_probe_bad(mo.gate_up_probe_case(128, 160), mutant) == 0
        for key in (("EDGE_A", 144, 896), ("EDGE_A", 144, 3072)):
            assert down_probe_bad(mo.down_probe_case(*key), mutant) > 0
        c = mo.down_integer_case("EDGE_A", 144, 1792)
        assert differs(run_down(c, mutant=mutant), c.expect) > 0
        c = mo.down_integer_case("EDGE_A", 144, 2048)      # nkb = 1
        assert differs(run_down(c, mutant=mutant), c.expect) == 0

    def test_slot_gathered_for_token(self):
        c = mo.gate_up_probe_case(384, 16)
        assert gate_up_probe_bad(c, "slot_for_token") > 0
        c = mo.gate_up_integer_case("ONE_EACH", 16)
        assert ratio(run_gate_up(c, mutant="slot_for_token"), c.ref,
                     c.bound) > 1

    def test_workspace_at_sorted_position(self):
        for key in mo.DOWN_PROBE:
            assert down_probe_bad(mo.down_probe_case(*key),
                                  "ws_sorted_pos") > 0
        c = mo.down_integer_case("EDGE_A", 144, 896)
        assert differs(run_down(c, mutant="ws_sorted_pos"), c.expect) > 0

    def test_combine_drops_the_last_split(self):
        for key, n in mo.DOWN_INTEGER.items():
            if n > 1:
                c = mo.down_integer_case(*key)
                assert differs(run_down(c, mutant="combine_drop_split"),
                               c.expect) > 0, key

    def test_combine_drops_the_last_k_slot(self):
        for key in mo.DOWN_INTEGER:
            c = mo.down_integer_case(*key)
            assert differs(run_down(c, mutant="combine_drop_k"),
                           c.expect) > 0, key
        for key in mo.DOWN_PROBE:
            assert down_probe_bad(mo.down_probe_case(*key),
                                  "combine_drop_k") > 0

    @pytest.mark.parametrize("mutant", ["swap_gate_up", "up_no_offset"])
    def test_gate_and_up_rows(self, mutant):
        for H in mo.PROBE_H:
            assert gate_up_probe_bad(mo.gate_up_probe_case(H, 16), mutant) > 0
        c = mo.gate_up_integer_case("EDGE_A", 160)
        assert ratio(run_gate_up(c, mutant=mutant), c.ref, c.bound) > 1

    def test_dead_second_subtile_written(self):
        """H = 144 = 4 x 32 + 16: the wave at column 128 has a dead second
        sub-tile. H = 160 and H = 16 (NSUB = 1) have none."""
        hit = 0
        for key in mo.DOWN_INTEGER:
            c = mo.down_integer_case(*key)
            bad = differs(run_down(c, mutant="dead_written"), c.expect)
            if key[1] == 144:
                assert bad > 0, key
                hit += 1
            elif mo.down_nsub(c.r.TK) == 1 or key[1] % 32 == 0:
                assert bad == 0, key
        assert hit >= 5

    def test_workspace_rounded_to_bf16(self):
        """Rejected by the cancelling family; the plain bounded family and
        the integer family (exact partials) let it through."""
        for key in mo.DOWN_CANCEL:
            c = mo.down_cancel_case(*key)
            w = ratio(run_down(c, mutant="ws_bf16"), c.ref, c.bound)
            record(f"ws_bf16 cancel {key}", w)
            assert w > 1.0, key
        for key in mo.DOWN_BOUNDED:
            c = mo.down_bounded_case(*key)
            record(f"ws_bf16 bounded {key}",
                   ratio(run_down(c, mutant="ws_bf16"), c.ref, c.bound))
        c = mo.down_integer_case("EDGE_A", 144, 3072)
        assert differs(run_down(c, mutant="ws_bf16"), c.expect) == 0


# --------------------------------------------------------------------------
# what the old check sees
# --------------------------------------------------------------------------

ALL_MUTANTS = ("grid_short", "tile_le", "drop_kk", "no_wrap",
               "stagger_no_wrap", "ws_sorted_pos", "combine_drop_split",
               "combine_drop_k", "dead_written", "ws_bf16")


def test_randn_and_loose_tolerance_miss_the_moe_mutants():
    """The check of test_moe_grouped_gpu.py (randn, rtol = 2^-7 / atol =
    1e-3, E = 4, K = 2, H = 160, I = 256 at T in {1, 17, 67, 130} and I =
    2048 at T = 1, routings from a seeded permutation) run on the down
    emulation with every mutant that touches the down path.

    Found: a workspace rounded to bf16 does not pass outright, contrary to
    a per-element estimate: 2.6 % of the elements (2640 of 103 360) are
    outside, all through the tail where the two split partials cancel and
    atol = 1e-3 is all that is left; the check sees it, without saying
    which elements must be wrong. A dead sub-tile's columns being written
    cannot arise there at all (H = 160 has no half-dead wave). A tile grid
    one short of the bound is visible only below 64 slots (T = 1, and T =
    17 when no expert is empty), where the bound is E or T K one-tile
    experts and the emulation's NaN workspace shows the lost rows (on the
    GPU the workspace is uninitialised memory); no old routing fills the
    bound with a full tile in front of a partial one (T = 67, 130), and
    there the output is bit-equal to the unmutated emulation. Both K-block
    mutants are the kernel at every old shape: I = 2048 is 16 splits of one
    block, I = 256 two splits of one block, so the old suite never runs
    the wrap. The remaining mutants (scan off by one, dropped sub-tile,
    workspace at the sorted position, combine dropping a split or a
    k-slot) are seen, in most elements."""
    from test_moe_grouped_gpu import GEMM_TOL, T_SET, ROUTINGS, routed_logits

    H, E, K = 160, 4, 2
    g = torch.Generator().manual_seed(22)
    weights = {I: (torch.randn(E, H, I, generator=g) / I ** 0.5).to(BF16)
               for I in (256, 2048)}
    shapes = [(256, T, routing) for T in T_SET for routing in ROUTINGS]
    shapes.append((2048, 1, "balanced"))
    outside = {m: 0 for m in ALL_MUTANTS}
    same = {m: True for m in ALL_MUTANTS}
    total = 0
    for I, T, routing in shapes:
        ga = torch.Generator().manual_seed(200 + T)
        act = torch.randn(T * K, I, generator=ga).to(BF16)
        _, topk_w, offsets, slots = ops.moe_route_ref(
            routed_logits(T, E, routing, T), K)
        counts = (offsets[1:] - offsets[:-1]).tolist()
        met = mo.live_tiles(counts) == mo.num_m_tiles(T * K, E)
        assert not met or T * K < mo.BM     # never with a full tile in it
        splits = mo.down_num_splits(T * K, E, H, I)
        assert (I // mo.KT) // splits == 1              # nkb = 1 everywhere
        ref = ops.moe_down_combine_ref(act, weights[I], topk_w, offsets,
                                       slots)
        clean = emulate_down(act, weights[I], topk_w, offsets, slots, splits)
        torch.testing.assert_close(clean.float(), ref, **GEMM_TOL)
        for m in ALL_MUTANTS:
            out = emulate_down(act, weights[I], topk_w, offsets, slots,
                               splits, m)
            if m == "grid_short" and met:
                assert bool(torch.isnan(out.float()).any())
                continue
            same[m] &= torch.equal(out, clean)
            err = (out.float() - ref).abs()
            bad = ~(err <= GEMM_TOL["atol"] + GEMM_TOL["rtol"] * ref.abs())
            outside[m] += int(bad.sum())
            if m == "ws_bf16":
                total += bad.numel()
    passes = {m: outside[m] == 0 for m in ALL_MUTANTS}
    print("\n[moe-emu] old check, elements outside:", outside, "of", total,
          "bit-equal:", same)
    assert 0 < outside["ws_bf16"] < 0.05 * total
    for m in ("grid_short", "dead_written", "no_wrap", "stagger_no_wrap"):
        assert same[m], m
    for m in ("tile_le", "drop_kk", "ws_sorted_pos", "combine_drop_split",
              "combine_drop_k"):
        assert not passes[m], m
