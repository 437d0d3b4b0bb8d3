"""mld_row_growth_segment_device and mld_row_growth_collect_*_device (RowGrowth) against their restatement
(row_growth_restatement: the reference's loops in plain Python, the tail composed from the oracle's parts;
test_row_growth_cpu.py pins both and holds the scenes).  Every record, every row table and every written list entry must
be BIT-EQUAL: integers, and the bit patterns of the doubles.  Records, row tables, lists and the merge arrays lie between
guard bytes, and what a call must not write keeps them.  Every table of cases asserts the state or flag it was built to
reach, so that a table that degenerates fails."""
import numpy as np
import pytest

from mono_lidar_depth_amd import CameraPinhole, ProjectedClouds, RowGrowth, capi

import row_growth_restatement as RG
from helpers import make_estimator
from test_row_growth_cpu import (GENEROUS, IDENTITY, SCENE_CAM, SWEEP_CAM, SWEEP_GROWTH, SWEEP_SEEDS, Scene, at, line, quirk_cases,
                                 reference_grid, scene_frame, scene_params, sweep_params, sweep_records, three_rows)

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD32 = np.frombuffer(bytes([GUARD] * 4), dtype=np.int32)[0]
PAD = 5
WIDE_CAM = (512, 48, 64.0, 256.0, 24.0)


class Guarded:
    """`nbytes` between guard bytes, all of them the guard pattern before the call; the payload starts 8-byte aligned."""

    def __init__(self, nbytes, dev, lead=8, fill=None):
        import torch
        self.size, self.lead = nbytes, lead
        self.buf = torch.full((lead + nbytes + PAD,), GUARD, dtype=torch.uint8, device=dev)
        if fill is not None:
            self.buf[lead:lead + nbytes] = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).to(dev)

    def view(self, dtype):
        return self.buf[self.lead:self.lead + self.size].view(dtype)

    def read(self, dtype):
        whole = self.buf.cpu().numpy()
        assert (whole[:self.lead] == GUARD).all() and (whole[self.lead + self.size:] == GUARD).all(), "a guard byte was overwritten"
        return whole[self.lead:self.lead + self.size].copy().view(dtype)


@pytest.fixture(scope="module")
def objects():
    """One estimator per camera (identity transform), RowGrowth objects on them; closed at the end."""
    made, objs = {}, []

    def obj(cam, n_seq, G, P, max_features=64, max_points=4096, row_capacity=64):
        if cam not in made:
            made[cam] = make_estimator(capi.params_c0(), camera=CameraPinhole(*cam), T=IDENTITY, max_frames=1)
        rg = RowGrowth(made[cam], n_seq, max_features, max_points, row_capacity, growth=G, parameters=P)
        objs.append(rg)
        return rg

    yield obj
    for rg in objs:
        rg.close()
    for e in made.values():
        e.close()


def dev():
    import torch
    return torch.device("cuda:0")


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()) if a is not None and a.size else None


def segment(rg, lists, n_visible=None, slack=0):
    """The cloud stage on the visible lists `lists` ([n, 2] arrays or None): (records [S], row tables with the guard where
    nothing was written).  n_visible: what the device array says (default: the lengths); slack: more room in uv than points."""
    import torch
    S = len(lists)
    uv = [up(np.concatenate([a, np.full((slack, 2), 1e9)])) if a is not None and (a.size or slack) else None for a in lists]
    nvis = torch.tensor([0 if a is None else a.shape[0] for a in lists] if n_visible is None else n_visible, dtype=torch.int64,
                        device=dev())
    rows = [Guarded(4 * (rg.row_capacity + 1), dev()) for _ in range(S)]
    cloud = Guarded(16 * S, dev())
    torch.cuda.synchronize()
    rg.segment(uv, nvis, [g.view(torch.int32) for g in rows], cloud.view(torch.int32).view(S, 4))
    rg._est.synchronize()
    return cloud.read(RG.CLOUD_DTYPE), [g.read(np.int32) for g in rows], (uv, rows, cloud)


def run(rg, scenes, uvs, cap=0, tracks=False, merge=False, rows_override=None):
    """Segment and collect for the scenes (uvs: per sequence [n, 2] or None).  rows_override: per sequence None or (row_start,
    n_rows, n_vis) put in place of what the segment call wrote.  Returns per sequence (records, list rows [n, cap], depth,
    types) - the last two None without merge - and the tensors' owners."""
    import torch
    S = len(scenes)
    _, _, (vis_uv, rows, cloud) = segment(rg, [sc.vis_uv for sc in scenes])
    if rows_override is not None:
        for s, o in enumerate(rows_override):
            if o is not None:
                row_start, n_rows, n_vis = o
                rows[s].view(torch.int32)[:] = torch.from_numpy(np.asarray(row_start, dtype=np.int32)).to(dev())
                cloud.view(torch.int32).view(S, 4)[s, :2] = torch.tensor([n_rows, n_vis], dtype=torch.int32, device=dev())
    ns = [0 if uv is None else int(np.asarray(uv).reshape(-1, 2).shape[0]) for uv in uvs]
    rec = [Guarded(72 * n, dev()) if n else None for n in ns]
    grown = [Guarded(4 * cap * n, dev()) if n else None for n in ns] if cap else None
    depth = types = None
    dsize, dtype = (4, np.float32) if tracks else (8, np.float64)
    if merge:
        depth = [Guarded(dsize * n, dev(), fill=(100.0 + 0.5 * np.arange(n)).astype(dtype)) if n else None for n in ns]
        types = [Guarded(4 * n, dev(), fill=(50 + np.arange(n)).astype(np.int32)) if n else None for n in ns]
    view = lambda gs, t: [g.view(t) if g is not None else None for g in gs] if gs is not None else None  # noqa: E731
    pm = [up(sc.pm.reshape(-1)) for sc in scenes]
    index, cam = [up(sc.index) for sc in scenes], [up(sc.cam) for sc in scenes]
    tail = (pm, index, cam, vis_uv, [g.view(torch.int32) for g in rows], cloud.view(torch.int32).view(S, 4), view(rec, torch.int64), cap,
            view(grown, torch.int32), view(depth, torch.float32 if tracks else torch.float64), view(types, torch.int32))
    torch.cuda.synchronize()
    if tracks:
        u = [up(np.asarray(uv, dtype=np.float32).reshape(-1, 2)[:, 0]) if n else None for uv, n in zip(uvs, ns)]
        v = [up(np.asarray(uv, dtype=np.float32).reshape(-1, 2)[:, 1]) if n else None for uv, n in zip(uvs, ns)]
        torch.cuda.synchronize()
        rg.collect_tracks(u, v, *tail)
    else:
        f = [up(np.asarray(uv, dtype=np.float64).reshape(-1, 2)) if n else None for uv, n in zip(uvs, ns)]
        torch.cuda.synchronize()
        rg.collect(f, *tail)
    rg._est.synchronize()
    out = []
    for s, n in enumerate(ns):
        if not n:
            out.append((np.zeros(0, dtype=RG.DTYPE), np.zeros((0, cap), np.int32), None, None))
            continue
        out.append((rec[s].read(RG.DTYPE), grown[s].read(np.int32).reshape(n, cap) if cap else np.zeros((n, 0), np.int32),
                    depth[s].read(dtype) if merge else None, types[s].read(np.int32) if merge else None))
    for g in rows:
        g.read(np.int32)
    cloud.read(np.int32)
    return out


def rows_of(lists, cap):
    """What the list rows must hold: the first min(n_grown, cap, 1024) entries, the guard pattern behind them."""
    rows = np.full((len(lists), cap), GUARD32, dtype=np.int32)
    for i, vis in enumerate(lists):
        m = min(vis.size, cap, RG.MAX_LIST)
        rows[i, :m] = vis[:m]
    return rows


def check(got, want, what=""):
    rec, grown = got[0], got[1]
    wrec, wlists = want
    bad = RG.same_records(rec, wrec)
    if bad:
        rows = [i for i in range(wrec.size) if RG.same_records(rec[i:i + 1], wrec[i:i + 1])]
        raise AssertionError(f"{what}: fields {bad} differ in features {rows[:8]}: got {rec[rows[0]]} want {wrec[rows[0]]}")
    if grown.shape[1]:
        assert np.array_equal(grown, rows_of(wlists, grown.shape[1])), what


def expected(scene, P, G, uv, cam=SCENE_CAM, tracks=False, seq=None):
    return RG.records(scene_frame(P, cam), P, G, seq if seq is not None else scene.sequence(), uv, tracks)


# ---- the cloud stage ---------------------------------------------------------------------------------------------------------

def scan(n, breaks, seed=0):
    """A visible list of n points whose rows start at `breaks` (and at 0): x falls inside a row and jumps up by more than 50
    at a break."""
    rng = np.random.default_rng(9300 + seed)
    x = np.empty(n)
    cur = 5000.0
    for i in range(n):
        cur = cur + rng.uniform(50.5, 400.0) if i in breaks else cur - rng.uniform(0.0, 3.0)
        x[i] = cur
    return np.stack([x, rng.uniform(1.0, 30.0, n)], axis=1)


SEGMENT_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)


def test_segment_at_the_sizes_where_the_blocks_and_the_groups_end(objects):
    rg = objects(SCENE_CAM, len(SEGMENT_SIZES), GENEROUS, scene_params())
    lists = [scan(n, {b for b in (63, 64, 1023, 1024, 7, 700, 2048) if b < n}, n) for n in SEGMENT_SIZES]
    rec, rows, _ = segment(rg, lists, slack=3)
    for s, a in enumerate(lists):
        wrec, wrows = RG.cloud_record(a[:, 0], rg.row_capacity, GUARD32)
        assert rec[s] == wrec and np.array_equal(rows[s], wrows), SEGMENT_SIZES[s]
    assert rec["n_rows"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] and rec["n_vis"].tolist() == list(SEGMENT_SIZES)
    assert (rec["flags"] == 0).all() and rec["longest_row"][-1] == 2048 - 1024


def test_segment_clamps_the_count_to_the_capacity_and_reads_it_on_the_gpu(objects):
    rg = objects(SCENE_CAM, 3, GENEROUS, scene_params())
    a = scan(200, {50, 120}, 1)
    rec, rows, _ = segment(rg, [a, a[:100], None], n_visible=[200, 170, 9])  # the second export was truncated at 100
    assert rec["n_vis"].tolist() == [200, 100, 0] and rec["n_rows"].tolist() == [3, 2, 0]
    assert rows[1][:3].tolist() == [0, 50, 100] and rows[2][0] == 0 and (rows[2][1:] == GUARD32).all()


def test_a_jump_of_exactly_fifty_opens_no_row_and_one_ulp_more_does(objects):
    rg = objects(SCENE_CAM, 2, GENEROUS, scene_params())
    x = np.array([300.0, 250.0, 300.0, 260.0, np.nextafter(310.0, 400.0), 100.0])
    lists = [np.stack([x, np.ones(6)], axis=1), np.stack([x[:4], np.ones(4)], axis=1)]
    rec, rows, _ = segment(rg, lists)
    assert rec["n_rows"].tolist() == [2, 1] and rows[0][:3].tolist() == [0, 4, 6] and rows[1][:2].tolist() == [0, 4]
    assert rec["longest_row"].tolist() == [4, 4]


def test_rows_at_the_capacity_and_one_beyond_it(objects):
    """The count is complete, the entries beyond the capacity keep the guard, the features are flagged."""
    P = scene_params()
    rg = objects(SCENE_CAM, 2, GENEROUS, P, row_capacity=3)
    three = Scene(three_rows(), row_capacity=3)
    four = Scene(three_rows() + [line(200.0, 4.0, 30, 40.0, y=1.0)], row_capacity=3)
    rec, rows, _ = segment(rg, [three.vis_uv, four.vis_uv])
    assert rec["n_rows"].tolist() == [3, 4] and rec["flags"].tolist() == [0, RG.ROWS_TRUNCATED]
    assert rows[0].tolist() == [0, 30, 60, 90] and rows[1].tolist() == [0, 30, 60, 90]  # (90: the row that did not fit starts there)
    uv = np.array([at(20.0, 12), at(30.0, 5), (np.nan, 3.0)])
    got = run(rg, [three, four], [uv, uv], cap=4)
    check(got[0], expected(three, P, GENEROUS, uv), "at the capacity")
    check(got[1], expected(four, P, GENEROUS, uv), "beyond the capacity")
    assert got[0][0]["state"].tolist() == [1, 1, 0] and got[0][0]["flags"].tolist() == [0, 0, RG.NONFINITE]
    assert (got[1][0]["flags"] == RG.ROWS_TRUNCATED).all() and (got[1][0]["type"] == 0).all() and (got[1][1] == GUARD32).all()


# ---- the feature stage: hand-made scenes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(quirk_cases()))
def test_the_quirk_cases_of_the_cpu_file(objects, name):
    rows, P, G, feature, _ = quirk_cases()[name]
    scene = Scene(rows, expect_rows=False)
    uv = np.array([feature])
    got = run(objects(SCENE_CAM, 1, G, P), [scene], [uv], cap=64)[0]
    want = expected(scene, P, G, uv)
    check(got, want, name)
    assert got[0]["state"][0] == 1 and got[0]["flags"][0] == 0 and got[0]["n_grown"][0] == want[1][0].size > 0


def aligned(u0, n, v, y):
    """A row at du = 1 whose x continues the seed row's (u = 400 - c at x = -0.05 c)."""
    return line(float(u0), 1.0, n, v, x0=-0.05 * (400.0 - u0), dx=0.05, y=y)


# (crossing column and length of the row above; of the row below; the rows the second seed may come from)
CROSSINGS = [((1, 2), (63, 64), "both"), ((63, 64), (64, 65), "both"), ((64, 65), (65, 130), "both"), ((65, 66), (1, 63), "both"),
             ((129, 130), (None, 40), "top"), ((None, 1), (2, 3), "bottom"), ((None, 2), (None, 1), "none")]


@pytest.mark.parametrize("top,bottom,which", CROSSINGS)
def test_rows_of_every_length_and_crossings_at_every_column(objects, top, bottom, which):
    """The seed is column 101 of a row of 200 at du = 1 (u = 299, the feature at 300.5); the rows above and below cross the
    feature at the given column - their last one, 1, 63, 64, 65 - or nowhere (None: the row lies left of the feature, or has
    one point).  At du = 1 the pick is always c - 1."""
    P = scene_params()

    def row(c, n, v, y):
        return aligned(300 + c, n, v, y) if c is not None else aligned(290, n, v, y)

    scene = Scene([row(*top, 10.0, -0.5), aligned(400, 200, 20.0, 0.0), row(*bottom, 30.0, 0.5)], W=512)
    uv = np.array([(300.5, 20.5), (300.5, 20.0)])
    got = run(objects(WIDE_CAM, 1, GENEROUS, P), [scene], [uv], cap=128)[0]
    want = expected(scene, P, GENEROUS, uv, WIDE_CAM)
    check(got, want, f"{top} {bottom}")
    rec = got[0]
    # (three returns in the window, all at z = 10: the first in scan order, column 101, is the seed)
    assert (rec["seed_vis"] == top[1] + 101).all() and (rec["seed_row"] == 1).all() and (rec["n_nb"] == 3).all()
    if which == "none":
        assert rec["state"].tolist() == [-1, -1] and (rec["second_vis"] == -1).all()
        return
    picks = {0: top[0] - 1 if top[0] else None, 2: top[1] + 200 + bottom[0] - 1 if bottom[0] else None}
    for r in rec:
        assert r["state"] in (1, -3) and r["second_vis"] == picks[int(r["second_row"])]
    if which == "both":  # the second feature lies half way: the tie goes to the bottom row
        assert rec["second_row"].tolist() == [0 if abs(10.0 - 20.5) < abs(30.0 - 20.5) else 2, 2]
    else:
        assert (rec["second_row"] == (0 if which == "top" else 2)).all()


def test_the_seed_in_the_first_row_the_last_row_and_a_single_row(objects):
    P = scene_params()
    scene, single = Scene(three_rows()), Scene([line(200.0, 4.0, 30, 20.0)])
    uv = np.array([at(10.0, 12), at(30.0, 12), at(20.0, 12)])
    got = run(objects(SCENE_CAM, 2, GENEROUS, P), [scene, single], [uv, uv[2:]], cap=16)
    check(got[0], expected(scene, P, GENEROUS, uv), "three rows")
    check(got[1], expected(single, P, GENEROUS, uv[2:]), "one row")
    assert got[0][0]["seed_row"].tolist() == [0, 2, 1] and got[0][0]["second_row"].tolist() == [1, 1, 2]
    assert got[0][0]["state"].tolist() == [1, 1, 1] and got[1][0]["state"].tolist() == [-1] and got[1][0]["seed_row"][0] == 0


def test_growth_ends_at_the_seed_distance_the_neighbour_distance_and_both_ends_of_the_row(objects):
    P = scene_params()
    scene = Scene(three_rows())
    uv = np.array([at(20.0, 12), at(20.0, 28), at(20.0, 1), at(20.0, 29), at(20.0, 0)])
    got = run(objects(SCENE_CAM, 1, GENEROUS, P), [scene], [uv], cap=16)[0]
    check(got, expected(scene, P, GENEROUS, uv), "the ends")
    # (left of column 0 no row crosses the feature: state -1, nothing grown)
    assert got[0]["n_first"].tolist() == [8, 5, 5, 4, 0] and got[0]["state"].tolist() == [1, 1, 1, 1, -1]
    # a step of 1.5 between the columns 13 and 14 against a neighbour limit of 0.7: one point up, and none down, because
    # `last` is still the point above the seed
    rows = three_rows()
    rows[1] = [(u, v, x - (1.0 if c >= 14 else 0.0), y, z) for c, (u, v, x, y, z) in enumerate(rows[1])]
    stepped, G = Scene(rows), RG.growth(0, 5, 0, 0.7, 0, 2, 0, -1)
    got = run(objects(SCENE_CAM, 1, G, P), [stepped], [uv[:1]], cap=16)[0]
    check(got, expected(stepped, P, G, uv[:1]), "the neighbour distance")
    assert got[0]["n_first"][0] == 1 and got[1][0, 0] == 30 + 13


@pytest.mark.parametrize("count", [-1, 0, 1, 2, 4, 5, 256])
def test_every_count(objects, count):
    P = scene_params()
    G = GENEROUS.replace(depth_segmentation_max_pointcount=count)
    scene = Scene(three_rows())
    uv = np.array([at(20.0, 12), at(20.0, 2), at(10.0, 27)])
    for cap in (0, 1):
        got = run(objects(SCENE_CAM, 1, G, P), [scene], [uv], cap=cap)[0]
        check(got, expected(scene, P, G, uv), f"count {count}")
    n_grown = got[0]["n_grown"].tolist()
    assert (got[0]["state"] == 1).all()
    assert n_grown[0] == {-1: 16, 0: 2, 1: 2, 2: 2, 4: 4, 5: 5, 256: 16}[count]


def test_a_row_of_eleven_hundred_points_caps_the_list(objects):
    P = scene_params()
    rows = [line(200.0, 4.0, 30, 10.0, y=-0.5), line(250.0, 0.2, 1100, 20.0, dx=0.001), line(200.0, 4.0, 30, 30.0, y=0.5)]
    rows[1] = [(u, v, x - 7.0 + 0.55, y, z) for u, v, x, y, z in rows[1]]  # (its middle above the columns 14 of the others)
    scene = Scene(rows)
    uv = np.array([(140.5, 20.5), at(10.0, 14)])
    got = run(objects(SCENE_CAM, 1, GENEROUS, P), [scene], [uv], cap=1024)[0]
    want = expected(scene, P, GENEROUS, uv)
    check(got, want, "1100 points")
    r = got[0][0]
    assert r["flags"] == RG.LIST_CAPPED and r["type"] == 0 and r["n_first"] == 1099 and r["n_grown"] > 1099 and r["state"] == 1
    assert (got[1][0] != GUARD32).all() and got[0][1]["flags"] == RG.LIST_CAPPED and got[0][1]["n_first"] == 8


def test_the_early_results_and_the_features_without_a_window(objects):
    """The early 4 with the thresholds disabled, the early 3 on a window whose returns are all at infinity, type 2 for
    features that are not finite or see no return."""
    P = scene_params(treshold_depth_enabled=0, treshold_depth_local_enabled=0)
    rows = three_rows()
    u, v, x, y, _ = rows[1][5]
    rows[1][5] = (u, v, x, y, 150.0)
    u, v, x, y, _ = rows[1][20]
    rows[1][20] = (u, v, x, y, np.inf)
    scene = Scene(rows)
    uv = np.array([at(20.0, 5), at(20.0, 20), at(20.0, 12), (np.nan, 20.0), (100.0, np.inf), (100.0, 40.0), (-30.0, 20.0), (300.0, 20.0)])
    for tracks in (False, True):
        got = run(objects(SCENE_CAM, 1, GENEROUS, P), [scene], [uv], cap=8, tracks=tracks, merge=True)[0]
        want = expected(scene, P, GENEROUS, uv, tracks=tracks)
        check(got, want, "early results")
        assert got[0]["type"].tolist() == [4, 3, 20, 2, 2, 2, 2, 2]
        assert got[0]["flags"].tolist() == [0, 0, 0, RG.NONFINITE, RG.NONFINITE, 0, 0, 0] and got[0]["seed_z"][0] == 150.0
        # the merge: the three decided entries are overwritten, the others and the guards are not touched
        depth, types = got[2], got[3]
        assert types.tolist() == [4, 3, 20] + [50 + i for i in range(3, 8)]
        assert depth[:2].tolist() == [-1.0, -1.0] and depth[3:].tolist() == [100.0 + 0.5 * i for i in range(3, 8)]
        assert depth[2] == (np.float32 if tracks else np.float64)(got[0]["depth"][2]) and depth[2] > 0


def test_values_that_point_outside_their_arrays(objects):
    """Map and index values, row bounds and the row count: the bad cell is empty, the bad row point ends the walk, the bad
    row is empty, a seed no row holds ends the feature - and every one of them raises BAD_INPUT."""
    P = scene_params()
    uv = np.array([at(20.0, 12), at(20.0, 20), at(10.0, 5)])
    cases = {}
    sc = Scene(three_rows())
    sc.pm[20, 152] = sc.n_vis + 40  # the cell of the seed of feature 0
    sc.pm[21, 120] = -2             # a cell in the window of feature 1
    cases["map"] = (sc, None, [RG.BAD_INPUT, RG.BAD_INPUT, 0], [0, 1, 1])
    sc = Scene(three_rows())
    sc.index[30 + 14] = sc.n_points  # two columns above the seed of feature 0
    sc.index[60 + 19] = -1           # the second seed of feature 1 in the bottom row (the top row's is tried next)
    cases["index"] = (sc, None, [RG.BAD_INPUT, RG.BAD_INPUT, 0], [1, 1, 1])
    sc = Scene(three_rows())
    rs = RG.cloud_record(sc.vis_uv[:, 0], 64, GUARD32)[1]
    rs[3] = 91  # the bottom row ends beyond the visible points
    cases["row end"] = (sc, (rs, 3, 90), [RG.BAD_INPUT, RG.BAD_INPUT, 0], [1, 1, 1])
    sc = Scene(three_rows())
    rs = RG.cloud_record(sc.vis_uv[:, 0], 64, GUARD32)[1]
    rs[1] = 95  # the first row ends beyond the visible points, and the search ends in it: no row holds the seeds
    cases["row start"] = (sc, (rs, 3, 90), [RG.BAD_INPUT] * 3, [0, 0, 0])
    sc = Scene(three_rows())
    cases["row count"] = (sc, (RG.cloud_record(sc.vis_uv[:, 0], 64, GUARD32)[1], -5, 90), [RG.BAD_INPUT] * 3, [0, 0, 0])
    cases["visible count"] = (sc, (RG.cloud_record(sc.vis_uv[:, 0], 64, GUARD32)[1], 3, 40), [RG.BAD_INPUT] * 3, None)
    rg = objects(SCENE_CAM, 1, GENEROUS, P)
    for name, (scene, override, flags, states) in cases.items():
        seq = scene.sequence()
        if override is not None:
            seq = RG.Sequence(scene.pm, scene.index, scene.n_vis, scene.cam, scene.vis_uv, override[0], override[1], override[2], 64)
        got = run(rg, [scene], [uv], cap=16, rows_override=[override])[0]
        check(got, expected(scene, P, GENEROUS, uv, seq=seq), name)
        assert got[0]["flags"].tolist() == flags, name
        if states is not None:
            assert got[0]["state"].tolist() == states, name


@pytest.mark.parametrize("tracks", [False, True])
def test_three_sequences_in_one_call_equal_their_runs_alone(objects, tracks):
    """One without features, one without points, one ordinary."""
    P = scene_params()
    full, empty = Scene(three_rows()), Scene([])
    uv = np.array([at(20.0, 12), at(10.0, 3), (150.7, 29.2), (10.0, 10.0), (np.inf, 1.0)])
    rg3, rg1 = objects(SCENE_CAM, 3, GENEROUS, P), objects(SCENE_CAM, 1, GENEROUS, P)
    got = run(rg3, [full, empty, full], [None, uv, uv], cap=8, tracks=tracks)
    assert got[0][0].size == 0
    for s, scene in ((1, empty), (2, full)):
        alone = run(rg1, [scene], [uv], cap=8, tracks=tracks)[0]
        want = expected(scene, P, GENEROUS, uv, tracks=tracks)
        check(got[s], want, f"sequence {s}")
        check(alone, want, f"sequence {s} alone")
        assert np.array_equal(got[s][1], alone[1])
    assert (got[1][0]["type"] == 2).all() and got[2][0]["type"].tolist()[:2] == [20, 20]


def test_more_features_than_one_grid_column(objects):
    """65 635 features of one sequence: the blocks beyond 65 535 take their features by the grid's stride."""
    P = scene_params()
    scene = Scene(three_rows())
    base = np.array([at(20.0, c) for c in range(30)] + [at(10.0, c) for c in range(30)] + [(np.nan, 1.0), (30.0, 40.0)] * 20)
    uv = np.tile(base, (657, 1))[:65635]
    wrec, wlists = expected(scene, P, GENEROUS, base)
    reps = -(-65635 // base.shape[0])
    want = (np.tile(wrec, reps)[:65635], (wlists * reps)[:65635])
    got = run(objects(SCENE_CAM, 1, GENEROUS, P, max_features=70000), [scene], [uv], cap=2)[0]
    check(got, want, "grid stride")


# ---- the reference's grid through the real chain ---------------------------------------------------------------------------

def test_the_references_grid_through_export_segment_and_collect(objects):
    import torch
    pts, _ = reference_grid()
    cam = (2000, 2000, 600.0, 1000.0, 1000.0)
    P = capi.params_c0().replace(pixelarea_search_witdh=10, pixelarea_search_height=10, radiusSearch_count_min=1, do_use_ransac_plane=0)
    rg = objects(cam, 1, GENEROUS, P)
    pc = ProjectedClouds(rg._est, 1, 400)
    cloud = torch.from_numpy(np.concatenate([pts, np.zeros((400, 1))], axis=1).astype(np.float32)).to(dev())
    nvis = torch.zeros(1, dtype=torch.int64, device=dev())
    uv, index = [torch.empty((400, 2), dtype=torch.float64, device=dev())], [torch.empty(400, dtype=torch.int32, device=dev())]
    cam_t, pm = [torch.empty((400, 3), dtype=torch.float64, device=dev())], [torch.empty((2000, 2000), dtype=torch.int32, device=dev())]
    rows, cl = [torch.full((65,), -7, dtype=torch.int32, device=dev())], torch.empty((1, 4), dtype=torch.int32, device=dev())
    rec, grown = [torch.empty((1, 9), dtype=torch.int64, device=dev())], [torch.full((1, 16), -7, dtype=torch.int32, device=dev())]
    f = [torch.tensor([[1000.0, 1000.0]], dtype=torch.float64, device=dev())]
    torch.cuda.synchronize()
    pc.export([cloud], None, nvis, uv, index, cam=cam_t, pixel_map=pm)
    rg.segment(uv, nvis, rows, cl)
    rg.collect(f, pm, index, cam_t, uv, rows, cl, rec, 16, grown)
    rg._est.synchronize()
    pc.close()
    c, r = RowGrowth.cloud_records(cl)[0], RowGrowth.records(rec[0])[0]
    assert (c["n_rows"], c["n_vis"], c["longest_row"], c["flags"]) == (20, 400, 20, 0)
    assert rows[0].cpu().tolist()[:21] == list(range(0, 401, 20))
    assert (r["seed_vis"], r["state"], r["seed_row"], r["second_vis"], r["n_first"], r["n_grown"]) == (210, 1, 10, 230, 4, 8)
    assert grown[0].cpu().tolist()[0] == [211, 212, 209, 208, 231, 232, 229, 228] + [-7] * 8
    assert r["type"] == 20 and r["depth"] == 20.0 and r["flags"] == 0 and r["n_nb"] == 1


# ---- the randomised sweep ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep():
    """The restatement of the whole sweep, computed once."""
    return {name: sweep_records(name) for name in SWEEP_GROWTH}


def test_the_sweep_reaches_every_state(sweep):
    """A condition on the sweep, not a measurement: the restatement alone gives every state and type 20 at least 20 times."""
    states = np.concatenate([rec["state"] for runs in sweep.values() for _, _, rec, _ in runs])
    types = np.concatenate([rec["type"] for runs in sweep.values() for _, _, rec, _ in runs])
    for state in (1, -1, -2, -3):
        assert (states == state).sum() >= 20, state
    assert (types == 20).sum() >= 20


@pytest.mark.parametrize("name", sorted(SWEEP_GROWTH))
def test_the_randomised_sweep(objects, sweep, name):
    """40 synthetic scan-ordered clouds on a 96 x 40 image, eight sequences per call, both feature forms alternating."""
    P, G = sweep_params(), SWEEP_GROWTH[name]()
    rg = objects(SWEEP_CAM, 8, G, P, max_points=2048, row_capacity=16)
    runs = sweep[name]
    assert len(runs) == SWEEP_SEEDS
    for first in range(0, SWEEP_SEEDS, 8):
        batch = runs[first:first + 8]
        tracks = (first // 8) % 2 == 1
        got = run(rg, [b[0] for b in batch], [b[1] for b in batch], cap=12, tracks=tracks)
        for s, (scene, uv, rec, lists) in enumerate(batch):
            want = (rec, lists) if not tracks else expected(scene, P, G, uv, SWEEP_CAM, tracks=True)
            check(got[s], want, f"{name} seed {first + s}")
