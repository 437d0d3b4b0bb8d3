"""mld_nearest_depths_collect_*_device (NearestDepths, TrackletBatch.nearest_depths) against its restatement
(nearest_depth_restatement: the neighbour rule in NumPy, the main path composed from the oracle's parts;
test_nearest_depths_cpu.py pins both).  Every record and every written list entry must be BIT-EQUAL: integers, and the bit
patterns of the doubles.  Records and lists lie between guard bytes, and the unwritten tail of a list row keeps them.

A wavefront reads the disc in squares of half size 4, 8, 16, 32, 64 (capped at the radius).  Shapes and what they reach:
  1 x 1       the cell or nothing
  11 x 11     the corner trap ((3, 3) of the first square is farther than (4, 0) of the second); the twelve cells at d2 25
  65 x 7      a row longer than a wavefront; the disc of R = 3 (29 cells) against k = 28, 29, 30
  70 x 37     clipping at every border, the disc that touches one column, the empty disc, the clamp, non-finite features
  130 x 70    R = 64: a disc taller than the image; the list filled at the first, a middle and the last stage
"""
import collections

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimatorError, NearestDepths, ProjectedClouds, TrackletBatch, capi, synth

import depth_image_frames as F
import feature_trace_restatement as T
import nearest_depth_restatement as N
from helpers import kitti_camera, make_estimator, make_oracle
from test_nearest_depths_cpu import COUNTS, RADII

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD32 = np.frombuffer(bytes([GUARD] * 4), dtype=np.int32)[0]
PAD = 5
C0 = capi.params_c0()


class Seq:
    """The input arrays of one sequence, made directly (no projection): one return in a fraction `density` of the cells, in
    the middle of its pixel for the camera F.camera(W, H); the upper half of the image on the plane z = 10.3 m (a millimetre
    of noise), the rest anywhere in 8 .. 13 m.  The visible list is shuffled, the original indices are a permutation of a
    cloud with `extra` points no cell shows."""

    def __init__(self, W, H, density, seed, extra=7, cells=None):
        rng = np.random.default_rng(9900 + seed)
        self.W, self.H = W, H
        if cells is None:
            ys, xs = np.nonzero(rng.random((H, W)) < density)
        else:
            xs, ys = (np.asarray(c, dtype=np.int64) for c in zip(*cells)) if cells else (np.zeros(0, np.int64),) * 2
        n_vis = xs.size
        self.n_points = n_vis + extra
        z = np.where(ys < (H + 1) // 2, 10.3 + rng.uniform(-1e-3, 1e-3, n_vis), rng.uniform(8.0, 13.0, n_vis))
        vis = rng.permutation(n_vis)  # cell k holds the visible index vis[k]
        self.index = rng.permutation(self.n_points)[:n_vis].astype(np.int32)
        self.index_len = n_vis
        self.pm = np.full((H, W), -1, dtype=np.int32)
        self.pm[ys, xs] = vis
        self.cam = rng.uniform(-5.0, 5.0, (self.n_points, 3))
        self.cam[:, 2] = rng.uniform(1.0, 50.0, self.n_points)
        o = self.index[vis]
        self.cam[o, 0] = (xs + 0.5 - 32.0) / 64.0 * z
        self.cam[o, 1] = (ys + 0.5 - 32.0) / 64.0 * z
        self.cam[o, 2] = z

    def vis_at(self, x, y):
        return int(self.pm[y, x])


_FRAMES = {}


def frame(W, H, P=C0):
    """The oracle that holds the calibration of the W x H camera (its viewing rays); made once per shape and parameter set."""
    key = (W, H, bytes(P))
    if key not in _FRAMES:
        _FRAMES[key] = make_oracle(P, F.camera(W, H), F.SMALL_T)
    return _FRAMES[key]


def expected(q, uv, R, k, P=C0, tracks=False):
    return N.records(frame(q.W, q.H, P), P, q.pm, q.index, q.index_len, q.n_points, q.cam, uv, R, k, tracks)


class Guarded:
    """`nbytes` between guard bytes, all of them the guard pattern before the call; the payload starts 8-byte aligned."""

    def __init__(self, nbytes, dev, lead=8):
        import torch
        self.size, self.lead = nbytes, lead
        self.buf = torch.full((lead + nbytes + PAD,), GUARD, dtype=torch.uint8, device=dev)

    def view(self, dtype):
        return self.buf[self.lead:self.lead + self.size].view(dtype)

    def read(self, dtype):
        whole = self.buf.cpu().numpy()
        ok = bool((whole[:self.lead] == GUARD).all() and (whole[self.lead + self.size:] == GUARD).all())
        return whole[self.lead:self.lead + self.size].copy().view(dtype), ok


def upload(seqs, uvs, cap, tracks=False, lists=True):
    """The device tensors of one call.  uvs: per sequence a float64 [n, 2] array, or None (no feature: null arrays).  The
    buffers are made on torch's stream, which nothing orders against the context's: torch.cuda.synchronize() before the
    call."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None and a.size else None  # noqa: E731
    ns = [0 if uv is None else int(np.asarray(uv).reshape(-1, 2).shape[0]) for uv in uvs]
    d = dict(ns=ns, cap=cap, tracks=tracks, map=[torch.from_numpy(q.pm.reshape(-1).copy()).to(dev) for q in seqs],
             index=[up(q.index) for q in seqs], cam=[up(q.cam) for q in seqs],
             rec=[Guarded(64 * n, dev) if n else None for n in ns],
             nb=[Guarded(4 * cap * n, dev) if n else None for n in ns] if (cap and lists) else None)
    if tracks:
        d["u"] = [up(np.asarray(uv, dtype=np.float32)[:, 0]) if n else None for uv, n in zip(uvs, ns)]
        d["v"] = [up(np.asarray(uv, dtype=np.float32)[:, 1]) if n else None for uv, n in zip(uvs, ns)]
    else:
        d["uv"] = [up(np.asarray(uv, dtype=np.float64).reshape(-1, 2)) if n else None for uv, n in zip(uvs, ns)]
    torch.cuda.synchronize()
    return d


def call(nd, d):
    import torch
    rec = [g.view(torch.int64) if g is not None else None for g in d["rec"]]
    nb = [g.view(torch.int32) if g is not None else None for g in d["nb"]] if d["nb"] is not None else None
    if d["tracks"]:
        nd.collect_tracks(d["u"], d["v"], d["map"], d["index"], d["cam"], rec, d["cap"], nb)
    else:
        nd.collect(d["uv"], d["map"], d["index"], d["cam"], rec, d["cap"], nb)


def read(d):
    out, ok = [], True
    for s, n in enumerate(d["ns"]):
        if not n:
            out.append((np.zeros(0, dtype=N.DTYPE), np.zeros((0, d["cap"]), dtype=np.int32)))
            continue
        rec, good = d["rec"][s].read(N.DTYPE)
        ok = ok and good
        nb = np.zeros((n, 0), dtype=np.int32)
        if d["nb"] is not None:
            nb, good = d["nb"][s].read(np.int32)
            ok = ok and good
            nb = nb.reshape(n, d["cap"])
        out.append((rec, nb))
    assert ok, "a guard byte was overwritten"
    return out


def run(nd, seqs, uvs, cap=0, tracks=False, lists=True):
    d = upload(seqs, uvs, cap, tracks, lists)
    call(nd, d)
    nd._est.synchronize()
    return read(d)


def rows_of(lists, cap):
    """What the list rows must hold: the first min(n_nb, cap) entries, the guard pattern behind them."""
    rows = np.full((len(lists), cap), GUARD32, dtype=np.int32)
    for i, vis in enumerate(lists):
        m = min(vis.size, cap)
        rows[i, :m] = vis[:m]
    return rows


def check(got, want, what=""):
    (rec, nb), (wrec, wlists) = got, want
    bad = N.same_records(rec, wrec)
    if bad:
        rows = [i for i in range(wrec.size) if N.same_records(rec[i:i + 1], wrec[i:i + 1])]
        raise AssertionError(f"{what}: fields {bad} differ in features {rows[:8]}: got {rec[rows[0]]} want {wrec[rows[0]]}")
    assert (rec["pad_"] == 0).all()
    if nb.shape[1]:
        assert np.array_equal(nb, rows_of(wlists, nb.shape[1])), what
    assert ((rec["n_in_radius"] > 0) | (rec["type"] == 2)).all()  # (C0's radiusSearch_count_min is 1)


@pytest.fixture(scope="module")
def objects():
    """One estimator per image shape (identity transform), NearestDepths objects on them; closed at the end."""
    made, objs = {}, []

    def obj(W, H, n_seq, max_features, R, k, P=None):
        if (W, H) not in made:
            made[(W, H)] = make_estimator(C0, camera=F.camera(W, H), T=F.SMALL_T, max_frames=1)
        nd = NearestDepths(made[(W, H)], n_seq, max_features, R, k, parameters=P)
        objs.append(nd)
        return nd

    yield obj
    for nd in objs:
        nd.close()
    for e in made.values():
        e.close()


def grid_features(W, H, nx=7, ny=5):
    xs = np.linspace(0.0, W - 1.0, nx)
    ys = np.linspace(0.0, H - 1.0, ny)
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2))


@pytest.mark.parametrize("density", [1.0, 0.0])
def test_one_cell(objects, density):
    q = Seq(1, 1, density, 1)
    uv = np.array([(0.0, 0.0), (0.5, 0.99), (1.0, 0.0), (0.0, 1.5), (1.0, 1.0), (2.0, 0.0), (-0.5, 0.0), (-1.5, 0.0)])
    got = run(objects(1, 1, 1, 8, 1, 1), [q], [uv], cap=1)[0]
    check(got, expected(q, uv, 1, 1), "1 x 1")
    assert got[0]["n_in_radius"].tolist() == [int(density)] * 4 + [0, 0, int(density), 0]


def test_the_corner_trap(objects):
    """Returns only at (8, 8), d2 18 from the centre (5, 5) and in the FIRST square, and at (9, 5), d2 16 and in the second."""
    q = Seq(11, 11, 0.0, 2, cells=[(8, 8), (9, 5)])
    uv = np.array([(5.0, 5.0), (5.9, 5.9)])
    near, far = q.vis_at(9, 5), q.vis_at(8, 8)
    for k, want in ((1, [near]), (2, [near, far])):
        got = run(objects(11, 11, 1, 2, 5, k), [q], [uv], cap=k)[0]
        check(got, expected(q, uv, 5, k), f"corner trap k = {k}")
        assert got[1][0].tolist() == want and got[0]["n_in_radius"].tolist() == [2, 2]
        assert (got[0]["d2_first"][0], got[0]["d2_last"][0]) == (16, 16 if k == 1 else 18)


def test_ties_come_in_row_major_order_and_a_list_may_end_inside_one(objects):
    """The twelve cells with d2 = 25 around (5, 5)."""
    ring = [(5 + dx, 5 + dy) for dy in range(-5, 6) for dx in range(-5, 6) if dx * dx + dy * dy == 25]
    assert len(ring) == 12
    q = Seq(11, 11, 0.0, 3, cells=ring)
    uv = np.array([(5.0, 5.0)])
    order = [q.vis_at(x, y) for x, y in ring]  # (built in (y, x) order)
    for R, k, want in ((5, 12, order), (5, 5, order[:5]), (4, 12, [])):
        got = run(objects(11, 11, 1, 1, R, k), [q], [uv], cap=k)[0]
        check(got, expected(q, uv, R, k), f"ties R = {R} k = {k}")
        assert got[1][0, :len(want)].tolist() == want and got[0]["n_nb"][0] == len(want)
        assert got[0]["n_in_radius"][0] == (12 if R == 5 else 0) and (R == 5 or got[0]["type"][0] == 2)


@pytest.mark.parametrize("k", [28, 29, 30])
def test_a_list_full_exactly_full_and_short(objects, k):
    """65 x 7 with a return in every cell: the disc of R = 3 has 29 cells."""
    q = Seq(65, 7, 1.0, 4)
    uv = np.array([(32.0, 3.0), (3.0, 3.0), (61.5, 3.5), (0.0, 0.0), (64.0, 6.0), (40.0, 0.0)])
    got = run(objects(65, 7, 1, 6, 3, k), [q], [uv], cap=k)[0]
    check(got, expected(q, uv, 3, k), f"65 x 7 k = {k}")
    assert got[0]["n_in_radius"][:3].tolist() == [29] * 3 and got[0]["n_nb"][:3].tolist() == [min(k, 29)] * 3
    assert got[0]["d2_last"][0] == 9 and got[0]["d2_first"][0] == 0  # (four cells share d2 = 9: k = 28 ends inside them)


def test_borders_the_clamp_and_non_finite_features(objects):
    W, H, R = 70, 37, 9
    q = Seq(W, H, 0.3, 5)
    uv = np.array([(0.0, 0.0), (W - 1.0, H - 1.0), (-3.0, 2.0), (W - 1.0 + R, 5.0), (float(W + R), 5.0), (-0.5, 10.0), (1e300, 5.0),
                   (-1e300, 5.0), (5.0, 1e300), (5.0, -float(R)), (5.0, -float(R) - 1.0), (np.nan, 5.0), (5.0, np.nan),
                   (np.inf, 5.0), (5.0, -np.inf), (np.nan, np.inf), (35.5, 18.5), (69.99, 36.99), (0.0, H - 1.0 + R)])
    got = run(objects(W, H, 1, uv.shape[0], R, 40), [q], [uv], cap=40)[0]
    want = expected(q, uv, R, 40)
    check(got, want, "borders")
    rec = got[0]
    assert (rec["flags"][11:16] == N.NONFINITE).all() and (rec["n_in_radius"][11:16] == 0).all() and (rec["type"][11:16] == 2).all()
    assert (rec["flags"][:11] == 0).all() and (rec["n_in_radius"][[4, 6, 7, 8, 10]] == 0).all()
    assert rec["n_in_radius"][3] == int(q.pm[5, W - 1] != -1)  # (the disc touches the last column in one cell)
    assert rec["n_in_radius"][0] > 0 and rec["n_in_radius"][16] > 40  # (a truncated list)
    assert np.isnan(rec["nearest_z"][4]) and rec["nearest_orig"][4] == -1 and (rec["d2_first"][4], rec["d2_last"][4]) == (-1, -1)


@pytest.mark.parametrize("density,k", [(1.0, 256), (1.0, 1), (0.3, 256), (0.3, 1), (0.02, 256), (0.02, 1)])
def test_the_largest_radius_fills_the_list_at_the_first_a_middle_and_the_last_stage(objects, density, k):
    """R = 64 on 130 x 70: the disc is taller than the image.  With a return in every cell 256 candidates lie within 10
    pixels (the stage of half size 16), at 0.3 within 17 (the stage 32), at 0.02 the whole disc holds fewer than 256; k = 1
    ends at the first stage wherever a return is within 4 pixels."""
    q = Seq(130, 70, density, 6)
    uv = grid_features(130, 70)
    got = run(objects(130, 70, 1, uv.shape[0], 64, k), [q], [uv], cap=min(k, 32))[0]
    want = expected(q, uv, 64, k)
    check(got, want, f"130 x 70 density {density} k = {k}")
    mid = got[0][17]  # the feature in the middle of the image
    if k == 256:
        assert {1.0: mid["d2_last"] <= 100, 0.3: 256 < mid["d2_last"] <= 1024, 0.02: mid["n_nb"] < 256}[density]
    assert mid["n_in_radius"] > (3000 if density == 1.0 else 30)
    print(f"density {density} k {k}: types {collections.Counter(got[0]['type'].tolist())}")


@pytest.mark.parametrize("R", RADII)
def test_every_stage_boundary_in_radius_and_count(objects, R):
    """Every (R, k) pair of the CPU test's lists on 130 x 70 at density 0.1, 16 features each."""
    q = Seq(130, 70, 0.1, 7)
    rng = np.random.default_rng(R)
    uv = np.stack([rng.uniform(-3.0, 133.0, 16), rng.uniform(-3.0, 73.0, 16)], axis=1)
    uv[:4] = [(64.0, 35.0), (0.0, 0.0), (129.0, 69.0), (64.5, 0.0)]
    for k in COUNTS:
        got = run(objects(130, 70, 1, 16, R, k), [q], [uv], cap=k)[0]
        check(got, expected(q, uv, R, k), f"R = {R} k = {k}")


def test_bad_map_and_index_values_make_a_cell_empty(objects):
    """Map values >= index_len, negative ones other than -1, index values outside [0, n_points): BAD_INPUT on the features
    whose disc holds such a cell, the cell is empty, the other features are unaffected."""
    W, H, R, k = 70, 37, 6, 20
    clean = Seq(W, H, 0.3, 8)
    q = Seq(W, H, 0.3, 8)
    q.pm[10, 10], q.pm[10, 40], q.pm[30, 20] = q.index_len, -2, -(2 ** 31)
    q.pm[5, 60] = 2 ** 31 - 1
    filled = np.argwhere(q.pm[20:30, 45:60] >= 0)[:2] + (20, 45)
    q.index[q.pm[filled[0][0], filled[0][1]]] = -1
    q.index[q.pm[filled[1][0], filled[1][1]]] = q.n_points
    uv = np.array([(10.0, 10.0), (40.0, 10.0), (20.0, 30.0), (60.0, 5.0), (float(filled[0][1]), float(filled[0][0])),
                   (float(filled[1][1]), float(filled[1][0])), (16.0, 10.0), (10.0, 17.0), (30.0, 20.0), (55.0, 33.0), (17.0, 10.0)])
    both = run(objects(W, H, 2, uv.shape[0], R, k), [q, clean], [uv, uv], cap=k)
    want = expected(q, uv, R, k)
    check(both[0], want, "bad input")
    check(both[1], expected(clean, uv, R, k), "clean neighbour")
    rec = both[0][0]
    assert (rec["flags"][:7] == N.BAD_INPUT).all() and (rec["flags"][7:] == 0).all()  # ((16, 10): the bad cell on the rim)
    assert (both[1][0]["flags"] == 0).all()
    assert (rec["d2_first"][:6] > 0).all()  # (the cell under the feature is empty)
    same = [7, 8, 9, 10]
    assert N.same_records(rec[same], both[1][0][same]) == []


@pytest.mark.parametrize("n_seq", [1, 3, 13])
def test_batches_of_sequences_of_different_sizes(objects, n_seq):
    """Sequences with different maps and feature counts in one call, one of them without a feature (null arrays)."""
    W, H, R, k = 70, 37, 12, 24
    seqs = [Seq(W, H, (0.05, 0.3, 0.8)[s % 3], 20 + s) for s in range(n_seq)]
    rng = np.random.default_rng(n_seq)
    counts = [(5, 0, 70, 1, 64, 65, 2, 0, 33, 9, 128, 3, 17)[s] for s in range(n_seq)]
    uvs = [np.stack([rng.uniform(-2.0, W + 2.0, n), rng.uniform(-2.0, H + 2.0, n)], axis=1) if n else None for n in counts]
    got = run(objects(W, H, n_seq, 128, R, k), seqs, uvs, cap=7)
    for s in range(n_seq):
        if counts[s]:
            check(got[s], expected(seqs[s], uvs[s], R, k), f"sequence {s} of {n_seq}")
        else:
            assert got[s][0].size == 0


@pytest.mark.parametrize("cap", [0, 1, 15, 16])
def test_list_capacity_bounds_every_row(objects, cap):
    W, H, R, k = 70, 37, 10, 16
    q = Seq(W, H, 0.3, 9)
    uv = grid_features(W, H, 6, 4)
    nd = objects(W, H, 1, 24, R, k)
    got = run(nd, [q], [uv], cap=cap)[0]
    check(got, expected(q, uv, R, k), f"list_capacity {cap}")
    assert got[1].shape == (24, cap) and (got[0]["n_nb"] == 16).any()
    if cap == 16:
        with pytest.raises(ValueError, match="list_capacity"):
            run(nd, [q], [uv], cap=17)
        assert run(nd, [q], [uv], cap=16, lists=False)[0][1].shape[1] == 0  # (the table absent as a whole)


def test_the_tracks_form_truncates_float32_coordinates(objects):
    W, H, R, k = 70, 37, 8, 12
    q = Seq(W, H, 0.3, 10)
    rng = np.random.default_rng(11)
    uv = np.stack([rng.uniform(-2.0, W + 2.0, 40), rng.uniform(-2.0, H + 2.0, 40)], axis=1)
    uv[:4] = [(-0.5, 3.7), (69.9, 36.9), (-1.5, -0.99), (12.25, 7.75)]
    nd = objects(W, H, 1, 40, R, k)
    got = run(nd, [q], [uv], cap=k, tracks=True)[0]
    check(got, expected(q, uv, R, k, tracks=True), "tracks")
    trunc = np.trunc(uv.astype(np.float32)).astype(np.float64)
    again = run(nd, [q], [trunc], cap=k)[0]
    assert N.same_records(got[0], again[0]) == [] and np.array_equal(got[1], again[1])
    assert got[0]["d2_first"][0] == again[0]["d2_first"][0] and trunc[0, 0] == 0.0  # (-0.5 truncates to -0, floors to 0)


def test_two_calls_in_a_row_without_a_synchronisation_between_them(objects):
    W, H, R, k = 70, 37, 10, 16
    qa, qb = Seq(W, H, 0.6, 12), Seq(W, H, 0.1, 13)
    uv = grid_features(W, H, 8, 5)
    nd = objects(W, H, 1, 40, R, k)
    da, db = upload([qa], [uv], k), upload([qb], [uv], k)
    call(nd, da)
    call(nd, db)
    nd._est.synchronize()
    check(read(da)[0], expected(qa, uv, R, k), "first call")
    check(read(db)[0], expected(qb, uv, R, k), "second call")


# ---- real projections ---------------------------------------------------------------------------------------------------

def small_frames():
    """The 64 x 64 frames of feature_trace_restatement as F.Frame (the oracle's pixel map, point index and cloud)."""
    return [("sparse", F.Frame(C0, F.SMALL_CAM, F.SMALL_T, T.sparse_cloud(), None), T.small_features(120)),
            ("dense", F.Frame(C0, F.SMALL_CAM, F.SMALL_T, T.dense_cloud(), None), T.dense_features())]


def frame_records(fr, uv, R, k, P=None, tracks=False):
    return N.records(fr.ref, P if P is not None else fr.P, fr.pm, fr.index, fr.index.size, fr.n_points, fr.cam, uv, R, k, tracks)


def cell_is_occupied(pm, u, v, R):
    """Whether the map cell under the feature holds a return."""
    if not (np.isfinite(u) and np.isfinite(v)):
        return False
    cx, cy = N.centre_cell(u, v, pm.shape[1], pm.shape[0], R)
    return bool(0 <= cx < pm.shape[1] and 0 <= cy < pm.shape[0] and pm[cy, cx] != -1)


@pytest.mark.parametrize("R,k", [(10, 10), (24, 64)])
def test_small_frames_through_the_projected_clouds(R, k):
    """sparse_cloud and dense_cloud: ProjectedClouds.export, then NearestDepths.collect on what it wrote."""
    import torch
    dev = torch.device("cuda:0")
    frames = small_frames()
    est = make_estimator(C0, camera=F.SMALL_CAM, T=F.SMALL_T, max_frames=1)
    try:
        pc = ProjectedClouds(est, 2, 4096)
        nd = NearestDepths(est, 2, 400, R, k)
        clouds = [torch.from_numpy(fr.cloud).to(dev) for _, fr, _ in frames]
        ns = [int(c.shape[0]) for c in clouds]
        out = dict(n_visible=torch.empty(2, dtype=torch.int64, device=dev),
                   uv=[torch.empty((n, 2), dtype=torch.float64, device=dev) for n in ns],
                   index=[torch.empty(n, dtype=torch.int32, device=dev) for n in ns],
                   cam=[torch.empty((n, 3), dtype=torch.float64, device=dev) for n in ns],
                   pm=[torch.empty((64, 64), dtype=torch.int32, device=dev) for _ in ns])
        uvs = [torch.from_numpy(uv).to(dev) for _, _, uv in frames]
        rec = [torch.empty((uv.shape[0], NearestDepths.WORDS), dtype=torch.int64, device=dev) for _, _, uv in frames]
        torch.cuda.synchronize()
        pc.export(clouds, ns, out["n_visible"], out["uv"], out["index"], None, out["cam"], out["pm"])
        nd.collect(uvs, out["pm"], out["index"], out["cam"], rec)
        est.synchronize()
        seen = collections.Counter()
        for s, (name, fr, uv) in enumerate(frames):
            want, _ = frame_records(fr, uv, R, k)
            got = NearestDepths.records(rec[s])
            assert N.same_records(got, want) == [], name
            seen.update(want["type"].tolist())
            occupied = np.array([cell_is_occupied(fr.pm, u, v, R) for u, v in uv])
            assert np.array_equal(got["d2_first"] == 0, occupied), name
            assert (got["type"][got["n_in_radius"] == 0] == 2).all()
        assert seen[1] >= 5 and seen[2] >= 1, seen
        nd.close()
        pc.close()
    finally:
        est.close()


def test_three_collinear_returns_take_the_degenerate_plane():
    """The 16 x 16 frame of three points on a line, planarity check off: Hyperplane::Through takes its eigenvector branch."""
    from mono_lidar_depth_amd import CameraPinhole
    P, cam = T.collinear_parameters(), CameraPinhole(*T.COLLINEAR_CAM)
    fr = F.Frame(P, cam, F.SMALL_T, T.collinear_cloud(), None)
    uv = np.array([T.COLLINEAR_PIXEL, (3.0, 3.0), (9.4, 8.6)], dtype=np.float64)
    want, lists = frame_records(fr, uv, 6, 3)
    assert want["n_nb"].tolist() == [3, 0, 3]
    est = make_estimator(P, camera=cam, T=F.SMALL_T, max_frames=1)
    try:
        nd = NearestDepths(est, 1, 3, 6, 3)
        q = Seq(16, 16, 0.0, 0)
        q.pm, q.index, q.index_len, q.n_points, q.cam = fr.pm, fr.index, fr.index.size, fr.n_points, fr.cam
        got = run(nd, [q], [uv], cap=3)[0]
        check(got, (want, lists), "collinear")
        nd.close()
    finally:
        est.close()


VARIANTS = {"c0": {}, "no_histogram": dict(do_use_histogram_segmentation=0), "first_three": dict(do_use_triangle_size_maximation=0),
            "global_clamps": dict(treshold_depth_mode=1), "local_clamps": dict(treshold_depth_local_mode=1)}


@pytest.fixture(scope="module")
def kitti():
    """One KITTI-size HDL-64 and one VLP-16 frame with 300 integer-pixel features each (half of them near returns), and the
    expected records of every variant at both (R, k), made once."""
    clouds = [synth.make_cloud(synth.HDL64_KITTI, seed=31, frame=2), synth.make_cloud(synth.VLP16, seed=32, frame=1)]
    uvs = [np.floor(np.concatenate([synth.make_features(150, seed=40 + s), synth.make_features_near_points(cl, 150, seed=50 + s)]))
           for s, cl in enumerate(clouds)]
    want = {}
    for name, change in VARIANTS.items():
        P = C0.replace(**change)
        frames = [F.Frame(P, kitti_camera(), synth.T_CAM_LIDAR, cl, None) for cl in clouds]
        for Rk in ((10, 10), (24, 64)):
            want[(name, Rk)] = [frame_records(fr, uv, *Rk, tracks=True) for fr, uv in zip(frames, uvs)]
    return dict(clouds=clouds, uvs=uvs, want=want)


def test_the_expected_values_hold_every_result_type_the_path_can_end_in(kitti):
    """So that no test below passes on frames where every feature is type 2."""
    seen = collections.Counter()
    for recs in kitti["want"].values():
        for rec, _ in recs:
            seen.update(rec["type"].tolist())
    print(f"types of the expected records: {sorted(seen.items())}")
    assert all(seen[t] >= 5 for t in (1, 2, 3, 8, 9)) and sum(seen[t] for t in (4, 5, 6, 7)) >= 5, seen


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tracklet_batch_nearest_depths_on_kitti_size_frames(kitti, variant):
    """TrackletBatch.nearest_depths on the products of projected_clouds(cam=True, pixel_map=True): HDL-64 and VLP-16 side by
    side, at (R, k) = (10, 10) and (24, 64)."""
    import torch
    dev = torch.device("cuda:0")
    tb = TrackletBatch(C0.replace(**VARIANTS[variant]), kitti_camera(), synth.T_CAM_LIDAR, 2, 300)
    try:
        tb.attach_projected_clouds(max(c.shape[0] for c in kitti["clouds"]))
        clouds = [torch.from_numpy(c).to(dev) for c in kitti["clouds"]]
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
        f = {"features": ([f32(uv[:, 0]) for uv in kitti["uvs"]], [f32(uv[:, 1]) for uv in kitti["uvs"]])}
        pc = tb.projected_clouds(clouds, cam=True, pixel_map=True)
        for Rk in ((10, 10), (24, 64)):
            nd = tb.attach_nearest_depths(*Rk)
            assert tb.attach_nearest_depths(*Rk) is nd and (nd.radius, nd.count) == Rk
            out = tb.nearest_depths(f, pc, list_capacity=8)
            maps = [m.cpu().numpy() for m in pc["pixel_map"]]
            for s in range(2):
                want, lists = kitti["want"][(variant, Rk)][s]
                got = NearestDepths.records(out["record"][s])
                assert N.same_records(got, want) == [], (variant, Rk, s)
                nb = out["nb"][s].cpu().numpy()
                for i in range(0, 300, 7):
                    m = min(lists[i].size, 8)
                    assert np.array_equal(nb[i, :m], lists[i][:m])
                # consistency with the product on the same frame
                uv = kitti["uvs"][s].astype(np.int64)
                inside = (uv[:, 0] >= 0) & (uv[:, 0] < synth.KITTI_W) & (uv[:, 1] >= 0) & (uv[:, 1] < synth.KITTI_H)
                occupied = np.zeros(300, dtype=bool)
                occupied[inside] = maps[s][uv[inside, 1], uv[inside, 0]] != -1
                assert np.array_equal(got["d2_first"] == 0, occupied)
                assert (got["type"][got["n_in_radius"] == 0] == 2).all()
            nd.close()  # (the next pair is another object)
            tb.nearest_depth_lists = None
    finally:
        tb.close()


def test_nearest_depths_without_attach_names_both():
    tb = TrackletBatch(C0, kitti_camera(), synth.T_CAM_LIDAR, 1, 10)
    try:
        with pytest.raises(DepthEstimatorError) as e:
            tb.nearest_depths({"features": ([None], [None])}, {})
        assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED
        assert "TrackletBatch.nearest_depths without attach_nearest_depths" in str(e.value)
        for bad in ((0, 10), (65, 10), (10, 0), (10, 257)):
            with pytest.raises(DepthEstimatorError) as e:
                tb.attach_nearest_depths(*bad)
            assert e.value.code == capi.MLD_ERR_INVALID_ARG and tb.nearest_depth_lists is None
    finally:
        tb.close()


def test_close_destroys_the_object_before_the_estimator(monkeypatch):
    """With a call still queued: the object's destroy waits for it, then the estimator goes."""
    import torch
    tb = TrackletBatch(C0, F.camera(70, 37), F.SMALL_T, 1, 40)
    nd = tb.attach_nearest_depths(10, 16)
    order = []
    nd_close, est_close = nd.close, tb.est.close
    monkeypatch.setattr(nd, "close", lambda: (order.append("nearest_depths"), nd_close())[1])
    monkeypatch.setattr(tb.est, "close", lambda: (order.append("estimator"), est_close())[1])
    q = Seq(70, 37, 0.3, 14)
    uv = grid_features(70, 37, 8, 5)
    d = upload([q], [uv], 16)
    call(nd, d)
    tb.close()
    assert order == ["nearest_depths", "estimator"] and tb.nearest_depth_lists is None and nd._nd is None
    torch.cuda.synchronize()
    check(read(d)[0], expected(q, uv, 10, 16), "the call queued ahead of close()")


def _tables():
    import ctypes as C
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    return dict(uv=tab, v=tab, n=zero, map=tab, index=tab, index_len=zero, cam=tab, n_points=zero, cap=0, record=tab, nb=None)


def _refusals():
    """(what differs from _tables(), status, word, forms: "both", or the one form the word belongs to)"""
    import ctypes as C
    INV, CAP = capi.MLD_ERR_INVALID_ARG, capi.MLD_ERR_CAPACITY
    i64, ptr = (lambda v: (C.c_int64 * 1)(v)), (lambda v: (C.c_void_p * 1)(v))
    one = i64(1)
    there = dict(n=one, uv=ptr(0x1000), v=ptr(0x1000), map=ptr(0x1000), record=ptr(0x1000))  # (made-up addresses: never touched)
    return [
        (dict(uv=None), INV, "null table uv", "uv"),
        (dict(uv=None), INV, "null table u", "tracks"),
        (dict(v=None), INV, "null table v", "tracks"),
        (dict(n=None), INV, "null table n_features", "both"),
        (dict(map=None), INV, "null table map", "both"),
        (dict(index=None), INV, "null table index", "both"),
        (dict(index_len=None), INV, "null table index_len", "both"),
        (dict(cam=None), INV, "null table cam", "both"),
        (dict(n_points=None), INV, "null table n_points", "both"),
        (dict(record=None), INV, "null table record_out", "both"),
        (dict(cap=-1), INV, "list_capacity must be in 0 .. count", "both"),
        (dict(cap=17), INV, "list_capacity must be in 0 .. count", "both"),
        (dict(n=i64(-1)), INV, "negative n_features", "both"),
        (dict(index_len=i64(-1)), INV, "negative index_len", "both"),
        (dict(n_points=i64(-1)), INV, "negative n_points", "both"),
        (dict(n=i64(601)), CAP, "n_features exceeds the max_features", "both"),
        (dict(n_points=i64(8388608)), CAP, "8 388 607", "both"),
        (dict(index_len=i64(8388608)), CAP, "8 388 607", "both"),
        (dict(there, uv=ptr(None)), INV, "null array uv", "uv"),
        (dict(there, uv=ptr(None)), INV, "null array u of", "tracks"),
        (dict(there, v=ptr(None)), INV, "null array v of", "tracks"),
        (dict(there, map=ptr(None)), INV, "null array map", "both"),
        (dict(there, record=ptr(None)), INV, "null array record_out", "both"),
        (dict(there, index_len=one), INV, "null array index", "both"),
        (dict(there, n_points=one), INV, "null array cam", "both"),
        (dict(there, uv=ptr(0x1004)), INV, "uv must be 8-byte aligned", "uv"),
        (dict(there, uv=ptr(0x1002)), INV, "u must be 4-byte aligned", "tracks"),
        (dict(there, v=ptr(0x1002)), INV, "v must be 4-byte aligned", "tracks"),
        (dict(there, map=ptr(0x1002)), INV, "map must be 4-byte aligned", "both"),
        (dict(there, index=ptr(0x1002)), INV, "index must be 4-byte aligned", "both"),
        (dict(there, cam=ptr(0x1004)), INV, "cam must be 8-byte aligned", "both"),
        (dict(there, record=ptr(0x1004)), INV, "record_out must be 8-byte aligned", "both"),
        (dict(there, cap=4, nb=ptr(0x1002)), INV, "nb_out must be 4-byte aligned", "both"),
    ]


def test_collect_refuses_with_a_text_that_names_the_function_and_the_argument():
    """Every refusal of both collect calls, decided on the host before anything is queued: none of the made-up addresses
    is touched and no kernel runs.  A call with one fault reports it with its status, behind the function's name; where the
    word does not belong to one form of the features, both forms are asked.  At the end a call on good tables is accepted."""
    est = make_estimator(C0, camera=F.camera(16, 16), T=F.SMALL_T, max_frames=1)
    nd = NearestDepths(est, 1, 600, 10, 16)
    lib = capi.load()
    try:
        def both(a):
            tail = (a["n"], a["map"], a["index"], a["index_len"], a["cam"], a["n_points"], a["cap"], a["record"], a["nb"])
            return {"uv": ("mld_nearest_depths_collect_device", lib.mld_nearest_depths_collect_device, (a["uv"],) + tail),
                    "tracks": ("mld_nearest_depths_collect_tracks_device", lib.mld_nearest_depths_collect_tracks_device,
                               (a["uv"], a["v"]) + tail)}

        asked = 0
        for bad, code, word, forms in _refusals():
            for form, (name, fn, args) in both(dict(_tables(), **bad)).items():
                if forms in ("both", form):
                    rc = fn(nd._nd, *args)
                    text = lib.mld_nearest_depths_last_error(nd._nd).decode()
                    assert rc == code and text.startswith(name + ": ") and word in text, (bad.keys(), form, rc, text)
                    asked += 1
        assert asked == 24 * 2 + 3 + 6
        for name, fn, args in both(_tables()).values():
            assert fn(nd._nd, *args) == capi.MLD_OK, name  # (no features: nothing to do)
    finally:
        nd.close()
        est.close()
