"""What the filter-gradient edge tests (tests/test_wgrad_edges_gpu.py) rest on, checked without a GPU: the geometry table reaches
every split class on every tile of csrc/wgrad2.hip when tile and workgroup target are forced through cn_conv_tune (so a later change
to the plan cannot quietly empty a class), the hand replays of the slice rules agree with what cn_conv_wgrad_plan reports, and the
float64 reference on integer inputs is the integer result exactly."""
import pytest
import torch

from confignet_amd._lib import lib
from tests import wgrad_edge_cases as W


@pytest.fixture(autouse=True)
def _no_tuning_left_behind():
    yield
    lib.cn_conv_tune(-1, 0, 0)


def test_the_table_reaches_every_split_class_on_every_tile():
    """1 slice / 2 to 7 / a multiple of 8 / 8 or more and no multiple of 8 (the grid is then padded to whole groups of 8 slices
    and the padding workgroups must leave): each of the five tiles sees all four, and the count the library plans is the one the
    forced-target arithmetic gives by hand."""
    seen = {tile[0]: {} for tile in W.TILES}
    for name, case in W.TABLE.items():
        g = W.geom(case)
        plan = W.forced_plan(case)
        for tile in W.TILES:
            for want in W.WANTS:
                assert plan[(tile[0], want)] == W.replayed_splits(g, tile, want), (name, tile[1], want, plan[(tile[0], want)])
                # ... and the one the device-free report of the launch names, with the tile that was forced and whole stages per slice
                lib.cn_conv_tune(tile[0], 0, want * W.tiles_of(g, tile))
                rc, route, cfg, slices, rows_per, _ = W.reported_plan(g)
                assert (rc, route, cfg, slices) == (0, 3, tile[0], W.replayed_splits(g, tile, want)), (name, tile[1], want)
                assert rows_per % tile[4] == 0 and -(-W.rows(g) // rows_per) == slices, (name, tile[1], want, rows_per)
                seen[tile[0]].setdefault(W.split_class(plan[(tile[0], want)]), []).append((name, want, plan[(tile[0], want)]))
    for tile in W.TILES:
        print(tile[1], {c: v for c, v in seen[tile[0]].items() if c != "1"})
        assert set(seen[tile[0]]) == set(W.SPLIT_CLASSES), (tile[1], sorted(seen[tile[0]]))


def test_the_pinned_split_counts():
    """The counts the table was built for: shape I gives 1 / 3 / 8 / 10 / 15 slices on the 16-deep tiles and 1 / 3 / 8 / 9 / 12 on
    the 32-deep ones, F reaches 8 / 10 / 15, H 8 and 9, E 7; B and C (M = 40 / 30) stay at one slice on every tile."""
    plan = {name: W.forced_plan(W.TABLE[name]) for name in "BCEFHI"}
    for tile in W.TILES:
        deep16 = tile[4] == 16
        assert [plan["I"][(tile[0], w)] for w in W.WANTS] == ([1, 3, 8, 10, 15] if deep16 else [1, 3, 8, 9, 12]), tile[1]
        assert {plan[n][(tile[0], w)] for n in "BC" for w in W.WANTS} == {1}, tile[1]
        if deep16:
            assert [plan["F"][(tile[0], w)] for w in W.WANTS] == [1, 3, 8, 10, 15], tile[1]
            assert [plan["H"][(tile[0], w)] for w in W.WANTS] == [1, 3, 8, 9, 9], tile[1]
            assert [plan["E"][(tile[0], w)] for w in W.WANTS] == [1, 3, 7, 7, 7], tile[1]


def test_a_slice_of_the_table_ends_short_of_a_stage_and_of_the_prologue():
    """The other edges the table is there for, from the plan's own numbers, on every tile: a last slice shorter than one stage (KB
    rows) behind full ones, a launch with fewer K steps than the prologue has stages in flight, a stage advance longer than
    out_w * out_h (several digits wrap in one step)."""
    short_last, short_launch, multi_wrap = [], [], []
    for name, case in W.TABLE.items():
        g = W.geom(case)
        m = W.rows(g)
        for tile in W.TILES:
            kb = tile[4]
            if kb > g.out_w * g.out_h:
                multi_wrap.append((name, tile[1]))
            for want in W.WANTS:
                s = W.replayed_splits(g, tile, want)
                r = -(-(-(-m // s)) // kb) * kb if s > 1 else m
                last = m - (s - 1) * r
                if s > 1 and last < kb:
                    short_last.append((name, tile[1], s, last))
                if -(-min(r, m) // kb) < 3:
                    short_launch.append((name, tile[1], s))
    for tile in W.TILES:
        assert any(t == tile[1] for _, t, _, _ in short_last), (tile[1], short_last)
        assert any(t == tile[1] for _, t, _ in short_launch) and any(t == tile[1] for _, t in multi_wrap), tile[1]


@pytest.mark.parametrize("name", list(W.TABLE) + [r[0] for r in W.ROUTING])
def test_the_reference_on_integer_inputs_is_exact(name):
    """float64 and float32 autograd on the CPU give the same integers: the reference is right, 9 M < 2^24 holds, and the sum
    really does not depend on its order."""
    case = W.TABLE[name] if name in W.TABLE else {r[0]: r[1] for r in W.ROUTING}[name]
    assert 9 * W.rows(W.geom(case)) < 2 ** 24
    x, gy = W.integer_inputs(case, seed=5)
    assert float(x.abs().max()) == 3.0 and float(gy.abs().max()) == 3.0
    ref = W.reference(x, gy, case)
    ref32 = W.reference(x, gy, case, dtype=torch.float32)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == W.filter_shape(case)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) > 0
    assert torch.equal(ref.float(), ref32)


def test_the_bf16_slice_rule_takes_the_xcd_order_where_the_tests_say():
    """The bf16 kernel's slice rule by hand (wgrad_edge_cases.bf16_planned_splits): the two extra bf16 shapes of the GPU test take the
    XCD-ordered grid, one with a whole number of groups of 8 slices and one with a padded last group; no table shape does."""
    for case, want in zip(W.BF16_XCD, ((16, True), (22, True))):
        assert W.bf16_planned_splits(W.geom(case)) == want, case
    for name in W.BF16_TABLE:
        assert not W.bf16_planned_splits(W.geom(W.TABLE[name]))[1], name


def test_the_bf16_replay_is_what_the_plan_reports():
    """bf16_planned_splits against cn_conv_wgrad_plan for every table entry and routing shape the bf16 kernel takes and the two XCD
    shapes, under every forced tile and target as well: the bf16 rule ignores the tuning, and so must the report."""
    cases = list(W.TABLE.values()) + [r[1] for r in W.ROUTING] + list(W.BF16_XCD)
    taken = 0
    for tile in [None] + W.TILES:
        for want in W.WANTS if tile else (0,):
            for case in cases:
                g = W.geom(case)
                if tile:
                    lib.cn_conv_tune(tile[0], 0, want * W.tiles_of(g, tile))
                rc, route, cfg, slices, rows_per, xcd = W.reported_plan(g, bf16=True)
                if g.cin % 8 or g.cout % 8:
                    assert (rc, route) == (-3, 6), case
                    continue
                bm, bn = W.bf16_tile(g)
                assert (rc, route) == (0, 5) and [t for t in W.TILES if t[0] == cfg][0][2:4] == (bm, bn), case
                assert (slices, xcd) == W.bf16_planned_splits(g), (case, slices, xcd)
                assert rows_per % 32 == 0 and -(-W.rows(g) // rows_per) == slices, (case, rows_per)
                taken += 1
    assert taken >= 26 * (len(W.BF16_TABLE) + 2)
    for name in W.BF16_TABLE:
        assert W.geom(W.TABLE[name]).cin % 8 == 0 and W.geom(W.TABLE[name]).cout % 8 == 0, name
