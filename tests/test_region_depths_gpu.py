"""mld_region_depths_collect_device (RegionDepths, TrackletBatch.region_depths) against its NumPy restatement
(region_depth_restatement, which test_region_depths_cpu.py checks against the oracle, the reference's Histogram object code
and NumPy's order statistics).  Every record must be BIT-EQUAL: integers, and the bit patterns of the doubles.  The records
lie between guard bytes.

A block has 256 threads and takes eight cells per thread and pass (2048 cells); the list in LDS holds RegionDepths.LIST_CAPACITY depths,
the histogram RegionDepths.HIST_BINS bins.  Shapes and what they reach:
  1 x 1       one cell: every box is the cell or nothing
  65 x 7      a row longer than a wavefront; boxes of a few cells
  70 x 37     two passes over the whole image (2590 cells > 2048), the second one partly filled
  300 x 5     a box wider than the 256 cells the threads of a block are apart
  130 x 70    at density 1.0: boxes of LIST_CAPACITY - 1, LIST_CAPACITY and LIST_CAPACITY + 1 counted points, the whole
              image on the re-scanning route
"""
import numpy as np
import pytest

from mono_lidar_depth_amd import RegionDepths, TrackletBatch, capi, synth

import depth_image_frames as F
import region_depth_restatement as G
from helpers import kitti_camera, make_estimator, make_oracle

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 5
C0 = capi.params_c0()
CAP, BINS = RegionDepths.LIST_CAPACITY, RegionDepths.HIST_BINS


class Seq:
    """The input arrays of one sequence, made directly (no projection): one point in a fraction `density` of the cells, the
    visible list in shuffled order, the original indices a permutation of a cloud with `extra` points no cell shows.
    z: None (the upper half of the image within 10 .. 11 m, the rest in 8 .. 13 m), or a function (xs, ys, rng) -> depths."""

    def __init__(self, W, H, density, seed, z=None, quant=None, extra=7):
        rng = np.random.default_rng(8800 + seed)
        self.W, self.H = W, H
        ys, xs = np.nonzero(rng.random((H, W)) < density)
        n_vis = xs.size
        self.n_points = n_vis + extra
        zz = np.where(ys < H // 2, rng.uniform(10.0, 11.0, n_vis), rng.uniform(8.0, 13.0, n_vis)) if z is None else z(xs, ys, rng)
        if quant:
            zz = np.round(np.asarray(zz) / quant) * quant
        vis = rng.permutation(n_vis)                       # cell k holds the visible index vis[k]
        self.index = rng.permutation(self.n_points)[:n_vis].astype(np.int32)  # visible index -> original index
        self.pm = np.full((H, W), -1, dtype=np.int32)
        self.pm[ys, xs] = vis
        self.cam = rng.uniform(-5.0, 5.0, (self.n_points, 3))
        self.cam[:, 2] = rng.uniform(1.0, 50.0, self.n_points)
        self.cam[self.index[vis], 2] = zz
        self.mask_bits = None

    def with_mask(self, bits):
        self.mask_bits = np.asarray(bits, dtype=bool)
        return self

    def mask_words(self):
        bits = np.zeros(((self.n_points + 31) // 32) * 32, dtype=bool)
        bits[:self.n_points] = self.mask_bits
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.int32).reshape(-1).copy()

    def expected(self, boxes, P=C0, index_len=None):
        return G.region_records(self.pm, self.index, self.cam, self.n_points, boxes, P.histogram_segmentation_bin_witdh,
                                P.histogram_segmentation_min_pointcount, self.mask_bits, index_len)


def standard_boxes(q, seed=0, n_random=12):
    """1 x 1 on an occupied and on an empty cell, the whole image, boxes across each border and each corner, boxes wholly
    outside, inverted boxes, and random ones."""
    W, H = q.W, q.H
    rng = np.random.default_rng(500 + seed)
    boxes = [(0, 0, W - 1, H - 1), (-7, -9, W + 11, H + 3)]
    for cells in (np.argwhere(q.pm != -1), np.argwhere(q.pm == -1)):
        if cells.size:
            y, x = cells[cells.shape[0] // 2]
            boxes.append((x, y, x, y))
    mx, my = W // 2, H // 2
    boxes += [(-5, my - 2, mx, my + 2), (mx, my - 2, W + 5, my + 2), (mx - 3, -4, mx + 3, my), (mx - 3, my, mx + 3, H + 4),   # borders
              (-3, -3, mx, my), (mx, -3, W + 2, my), (-3, my, mx, H + 2), (mx, my, W + 2, H + 2),                              # corners
              (-9, 0, -1, H - 1), (W, 0, W + 8, H - 1), (0, -6, W - 1, -1), (0, H, W - 1, H + 5), (W + 3, H + 3, W + 9, H + 9),  # outside
              (mx + 1, 0, mx, H - 1), (0, my + 1, W - 1, my), (W - 1, H - 1, 0, 0),                                            # inverted
              (0, 0, 0, H - 1), (0, 0, W - 1, 0), (W - 1, 0, W - 1, H - 1)]                                                    # one column, one row
    for _ in range(n_random):
        x0, x1 = np.sort(rng.integers(-4, W + 4, 2))
        y0, y1 = np.sort(rng.integers(-4, H + 4, 2))
        boxes.append((x0, y0, x1, y1))
    return np.asarray(boxes, dtype=np.int32).reshape(-1, 4)


class Guarded:
    """`count` int64 between guard bytes, all of them the guard pattern before the call."""

    def __init__(self, count, dev, lead=8):
        import torch
        self.size, self.lead = 8 * count, lead
        self.buf = torch.full((lead + self.size + PAD,), GUARD, dtype=torch.uint8, device=dev)

    def view(self):
        import torch
        return self.buf[self.lead:self.lead + self.size].view(torch.int64)

    def read(self):
        whole = self.buf.cpu().numpy()
        ok = bool((whole[:self.lead] == GUARD).all() and (whole[self.lead + self.size:] == GUARD).all())
        return whole[self.lead:self.lead + self.size].copy().view(G.DTYPE), ok


def upload(seqs, boxes, masks=True):
    """The device tensors of one call.  boxes: per sequence an int32 [n, 4] array, or None (no box: null arrays).  The
    buffers are made on torch's stream, which nothing orders against the context's: torch.cuda.synchronize() before the
    call."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None and a.size else None  # noqa: E731
    d = dict(map=[torch.from_numpy(q.pm.reshape(-1).copy()).to(dev) for q in seqs], index=[up(q.index) for q in seqs],
             cam=[up(q.cam) for q in seqs], boxes=[up(b) for b in boxes],
             rec=[Guarded(RegionDepths.WORDS * b.shape[0], dev) if b is not None and b.size else None for b in boxes],
             mask=[up(q.mask_words()) if q.mask_bits is not None else None for q in seqs] if masks else None)
    if d["mask"] is not None and all(m is None for m in d["mask"]):
        d["mask"] = None
    torch.cuda.synchronize()
    return d


def call(rd, d):
    rd.collect(d["map"], d["index"], d["cam"], d["boxes"], [g.view() if g is not None else None for g in d["rec"]], d["mask"])


def read(d):
    out, ok = [], True
    for g in d["rec"]:
        if g is None:
            out.append(np.zeros(0, dtype=G.DTYPE))
            continue
        r, good = g.read()
        ok = ok and good
        out.append(r)
    assert ok, "a guard byte was overwritten"
    return out


def run(rd, seqs, boxes, masks=True):
    d = upload(seqs, boxes, masks)
    call(rd, d)
    rd._est.synchronize()
    return read(d)


def check(got, seqs, boxes, P=C0, what=""):
    for s, (q, b) in enumerate(zip(seqs, boxes)):
        if b is None or not b.size:
            assert got[s].size == 0
            continue
        want = q.expected(b, P)
        bad = G.same_records(got[s], want)
        if bad:
            rows = [i for i in range(want.size) if G.same_records(got[s][i:i + 1], want[i:i + 1])]
            raise AssertionError(f"{what} sequence {s}: fields {bad} differ in boxes {rows[:8]}: box {b[rows[0]]} got {got[s][rows[0]]} "
                                 f"want {want[rows[0]]}")
        assert (got[s]["pad_"] == 0).all()


@pytest.fixture(scope="module")
def objects():
    """One estimator per image shape (identity transform), RegionDepths objects on them; closed at the end."""
    made, objs = {}, []

    def obj(W, H, n_seq, max_boxes, P=None):
        if (W, H) not in made:
            made[(W, H)] = make_estimator(C0, camera=F.camera(W, H), T=F.SMALL_T, max_frames=1)
        rd = RegionDepths(made[(W, H)], n_seq, max_boxes, parameters=P)
        objs.append(rd)
        return rd

    yield obj
    for rd in objs:
        rd.close()
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def dense():
    """130 x 70 with a point in every cell, z in 6 .. 30 m quantised to 0.25 m (97 values for 9100 points): shared, never
    changed."""
    return Seq(130, 70, 1.0, 1, z=lambda xs, ys, rng: rng.uniform(6.0, 30.0, xs.size), quant=0.25)


@pytest.mark.parametrize("W,H,density", [(1, 1, 1.0), (1, 1, 0.0), (65, 7, 0.6), (70, 37, 0.6), (300, 5, 0.6), (130, 70, 1.0)])
def test_image_shapes_and_the_standard_boxes(objects, W, H, density):
    """Without a mask and with a random third of the points as ground, side by side in one call."""
    q0 = Seq(W, H, density, 10 * W + H, quant=0.25)
    q1 = Seq(W, H, density, 10 * W + H, quant=0.25)
    q1.with_mask(np.random.default_rng(W).random(q1.n_points) < 0.33)
    boxes = [standard_boxes(q0), standard_boxes(q1, seed=1)]
    got = run(objects(W, H, 2, boxes[0].shape[0]), [q0, q1], boxes)
    check(got, [q0, q1], boxes, what=(W, H, density))
    whole = got[0][0]
    assert tuple(whole["clip"]) == (0, 0, W - 1, H - 1) and whole["n_points"] == (q0.pm != -1).sum() and not whole["flags"] & G.HAS_MASK
    assert (got[1]["flags"] & G.HAS_MASK).all() and (got[0]["flags"] & G.EMPTY_BOX).sum() >= 8
    if density:
        assert got[1][0]["n_ground"] > 0 or W * H == 1
        assert got[0][2]["n_points"] == 1 and got[0][2]["z_min"] == got[0][2]["z_median"] == got[0][2]["z_max"]  # 1 x 1, occupied
    if W == 300:
        assert whole["n_points"] > 256 and got[0][0]["clip"][2] - got[0][0]["clip"][0] + 1 > 256
    if (W, H) == (130, 70):
        assert whole["n_points"] == 9100 > CAP  # the re-scanning route
        assert (got[0]["flags"] & G.HIST_FOUND).any()


def test_box_counts_of_0_1_64_65_and_257_side_by_side(objects, dense):
    """Sequences of different n_boxes in one call - one of them without a box and with null arrays for boxes and records
    - and a call in which no sequence has a box (nothing is launched)."""
    counts = [64, 0, 257, 1, 65]
    seqs = [Seq(70, 37, 0.5, 40 + s, quant=0.25) for s in range(5)]
    rng = np.random.default_rng(3)
    boxes = []
    for q, n in zip(seqs, counts):
        b = np.concatenate([standard_boxes(q, seed=n, n_random=max(n, 40))] * 2)[:n] if n else None
        boxes.append(b if b is None else b[rng.permutation(n)])
    rd = objects(70, 37, 5, 257)
    check(run(rd, seqs, boxes), seqs, boxes, what="counts")
    none = [None] * 5
    assert [r.size for r in run(rd, seqs, none)] == [0] * 5
    with pytest.raises(ValueError, match="257"):
        rd.collect(*[upload(seqs[:1] * 5, [np.zeros((258, 4), dtype=np.int32)] * 5)[k] for k in ("map", "index", "cam", "boxes")],
                   [None] * 5)


def capacity_boxes(q):
    """On the dense 130 x 70 frame with 32 holes: 64 x 32 cells without a hole (CAP points), the same with one hole
    (CAP - 1), 65 x 32 cells with 31 holes (CAP + 1)."""
    assert CAP == 64 * 32
    holes = [(64 + 10, 5)] + [(k, 32 + k % 32) for k in range(31)]  # (x, y)
    pm = q.pm.copy()
    for x, y in holes:
        pm[y, x] = -1
    return pm, np.array([(64, 0, 127, 31), (0, 0, 63, 31), (0, 32, 64, 63), (0, 0, 129, 69)], dtype=np.int32)


@pytest.mark.parametrize("route", ["shipped", "ab", "ab-rescan", "ab-tiny-list"])
def test_boxes_at_the_list_capacity_take_both_median_routes(dense, monkeypatch, route):
    """CAP - 1 and CAP counted points stay in the LDS list, CAP + 1 and the whole image are scanned again for every pass:
    by construction, from n_points.  In the A/B library the list capacity can be set: 0 sends every box through the
    re-scanning route, 5 all but the smallest; the records stay the same bit for bit."""
    import copy
    q = copy.copy(dense)
    q.pm, big = capacity_boxes(dense)
    boxes = [np.concatenate([big, standard_boxes(q)])]
    if route != "shipped":
        monkeypatch.setattr(capi, "_lib", capi.load_ab())
    if route == "ab-rescan":
        monkeypatch.setenv("MLD_REGION_LIST_CAPACITY", "0")
    if route == "ab-tiny-list":
        monkeypatch.setenv("MLD_REGION_LIST_CAPACITY", "5")
    est = make_estimator(C0, camera=F.camera(130, 70), T=F.SMALL_T, max_frames=1)
    try:
        rd = RegionDepths(est, 1, boxes[0].shape[0])
        got = run(rd, [q], boxes)
        check(got, [q], boxes, what=route)
        assert list(got[0]["n_points"][:4]) == [CAP - 1, CAP, CAP + 1, 9100 - 32]
        # duplicates: z is quantised to 0.25 m, so the median's rank falls into a run of equal values and the nearest point
        # is one of several
        z = q.cam[q.index[q.pm[0:32, 0:64].reshape(-1)], 2]
        assert (z == z.min()).sum() > 1 and (z == got[0][1]["z_median"]).sum() > 1
        assert got[0][1]["nearest_orig"] == q.index[q.pm[0:32, 0:64].reshape(-1)[np.argmin(z)]]
        rd.close()
    finally:
        est.close()


def ramp(k_extra):
    """130 x 70, every cell a point, bin width 1 m: the cells (x < 128, y) hold 3.0 + 128 * y + x metres - one point per bin -,
    column 128 holds 3.0 + 512 in row 0 and copies of 3.0 + 511 below, column 129 and the rows from 4 on 3.0 + 511 too."""
    def z(xs, ys, rng):
        v = 3.0 + 128.0 * ys + xs
        v = np.where((xs >= 128) | (ys >= 4), 3.0 + 511.0, v)
        return np.where((xs == 128) & (ys == 0), 3.0 + 512.0, v)
    return Seq(130, 70, 1.0, 77, z=z)


def test_a_run_of_bins_beyond_the_histogram_storage_sets_hist_capped_and_one_just_short_does_not(objects):
    P = C0.replace(histogram_segmentation_bin_witdh=1.0, histogram_segmentation_min_pointcount=1)
    q = ramp(0)
    assert BINS == 512
    boxes = [np.array([(0, 0, 127, 3),     # 512 bins, the run ends on the last bin: fits
                       (0, 0, 128, 3),     # 513 bins: capped
                       (0, 0, 127, 2),     # 384 bins
                       (0, 0, 129, 69),    # capped on the re-scanning route
                       (5, 1, 60, 1)], dtype=np.int32)]
    got = run(objects(130, 70, 1, 5, P), [q], boxes)
    check(got, [q], boxes, P, what="ramp")
    r = got[0]
    assert list(r["flags"]) == [G.HIST_FOUND, G.HIST_CAPPED, G.HIST_FOUND, G.HIST_CAPPED, G.HIST_FOUND]
    assert (r["hist_lower"][0], r["hist_higher"][0], r["n_seg"][0]) == (3.0, 4.0, 1)
    assert (r["hist_lower"][1], r["hist_higher"][1], r["n_seg"][1]) == (-1.0, -1.0, 0)
    # nothing else of a capped record changes
    assert r["n_points"][1] == 516 and r["z_min"][1] == 3.0 and r["z_max"][1] == 515.0 and r["z_median"][1] == 3.0 + 257.0


def test_all_points_ground_and_no_mask_for_some_sequences(objects, dense):
    import copy
    all_ground = copy.copy(dense).with_mask(np.ones(dense.n_points, dtype=bool))
    plain = copy.copy(dense)
    some = copy.copy(dense).with_mask(np.arange(dense.n_points) % 3 == 0)
    seqs = [all_ground, plain, some]
    boxes = [standard_boxes(dense, n_random=4)] * 3
    got = run(objects(130, 70, 3, boxes[0].shape[0]), seqs, boxes)  # (the table has a null entry for `plain`)
    check(got, seqs, boxes, what="masks")
    assert (got[0]["n_points"] == 0).all() and got[0]["n_ground"][0] == 9100 and got[0]["z_median"][0] == -1.0
    assert got[0]["flags"][0] == G.HAS_MASK and got[1]["flags"][0] & G.HAS_MASK == 0 and got[1]["n_ground"].sum() == 0
    assert 0 < got[2]["n_ground"][0] < 9100 and got[2]["n_points"][0] + got[2]["n_ground"][0] == 9100
    # without the table at all
    got = run(objects(130, 70, 3, boxes[0].shape[0]), seqs, boxes, masks=False)
    for q in seqs:
        q.mask_bits = None
    check(got, seqs, boxes, what="no mask table")


def test_bad_input_sets_the_flag_of_the_boxes_that_meet_it_and_nothing_else(objects):
    """A map value beyond index_len (and a negative one), an index beyond n_points (and a negative one), a NaN, a zero and
    a negative z: each in a cell of its own.  The boxes that contain such a cell carry BAD_INPUT and skip it, the others
    are as if nothing had happened; the arrays are uploaded at their exact sizes, index_len shortened by the tensor's
    length, so a read beyond them would leave the allocation."""
    q = Seq(70, 37, 1.0, 5, quant=0.25)
    clean = q.expected(standard_boxes(q))
    cells = [(3, 3), (10, 3), (20, 20), (30, 20), (40, 30), (50, 30), (60, 35)]  # (x, y)
    vis = [int(q.pm[y, x]) for x, y in cells]
    q.pm[3, 3] = q.index.size + 5
    q.pm[3, 10] = -2
    q.index[vis[2]] = q.n_points
    q.index[vis[3]] = -1
    q.cam[q.index[vis[4]], 2] = np.nan
    q.cam[q.index[vis[5]], 2] = 0.0
    q.cam[q.index[vis[6]], 2] = -4.0
    single = np.array([(x, y, x, y) for x, y in cells], dtype=np.int32)
    around = np.array([(x - 2, y - 1, x + 2, y + 1) for x, y in cells], dtype=np.int32)
    std = standard_boxes(q)
    boxes = [np.concatenate([single, around, std])]
    got = run(objects(70, 37, 1, boxes[0].shape[0]), [q], boxes)
    check(got, [q], boxes, what="bad input")
    r = got[0]
    assert (r["flags"][:7] == G.BAD_INPUT).all() and (r["n_points"][:7] == 0).all() and (r["nearest_orig"][:7] == -1).all()
    assert (r["flags"][7:14] & G.BAD_INPUT).all() and (r["n_points"][7:14] == 14).all()
    hit = np.array([any(b[0] <= x <= b[2] and b[1] <= y <= b[3] for x, y in cells) for b in std])
    assert ((r["flags"][14:] & G.BAD_INPUT) != 0).tolist() == hit.tolist() and hit.any() and not hit.all()
    assert not G.same_records(r[14:][~hit], clean[~hit])  # the other boxes are unaffected


def test_two_calls_queued_back_to_back_equal_the_calls_run_apart(objects):
    """No synchronisation between the two calls: the second call's descriptors and boxes must not disturb the first."""
    seqs_a = [Seq(70, 37, 0.7, 60 + s, quant=0.25) for s in range(2)]
    seqs_b = [Seq(70, 37, 0.3, 70 + s) for s in range(2)]
    boxes_a = [standard_boxes(q, seed=2) for q in seqs_a]
    boxes_b = [standard_boxes(q, seed=3, n_random=30)[::-1].copy() for q in seqs_b]
    rd = objects(70, 37, 2, 64)
    apart = [run(rd, seqs_a, boxes_a), run(rd, seqs_b, boxes_b)]
    da, db = upload(seqs_a, boxes_a), upload(seqs_b, boxes_b)
    call(rd, da)
    call(rd, db)
    rd._est.synchronize()
    for got, want, seqs, boxes in ((read(da), apart[0], seqs_a, boxes_a), (read(db), apart[1], seqs_b, boxes_b)):
        check(got, seqs, boxes, what="queued")
        assert all(not G.same_records(g, w) for g, w in zip(got, want))


# ---- a real plane mask, and the wrapper ------------------------------------------------------------------------------
def road_cloud():
    """A flat road (lidar z = -1.73 m) 4 .. 20 m ahead and a board across it on legs, 2 m wide, from 0.4 m to 1.5 m above the
    road, 12 m ahead: float32 [n, 4] in the lidar frame, and the board's points.  Fewer than 6000 points, so that the
    estimator's sample - the only points its mask can mark - is the whole cloud."""
    gx, gy = np.meshgrid(np.arange(4.0, 20.0, 0.25), np.arange(-3.0, 3.0, 0.1))
    road = np.stack([gx.reshape(-1), gy.reshape(-1), np.full(gx.size, synth.GROUND_Z)], axis=1)
    by, bz = np.meshgrid(np.arange(-1.0, 1.0, 0.05), np.arange(synth.GROUND_Z + 0.4, synth.GROUND_Z + 1.5, 0.05))
    board = np.stack([np.full(by.size, 12.0), by.reshape(-1), bz.reshape(-1)], axis=1)
    rng = np.random.default_rng(12)
    pts = np.concatenate([road, board])
    assert pts.shape[0] < 6000
    order = rng.permutation(pts.shape[0])
    cloud = np.zeros((pts.shape[0], 4), dtype=np.float32)
    cloud[:, :3] = pts[order]
    return cloud, np.nonzero(order >= road.shape[0])[0]


def test_a_ransac_plane_mask_takes_the_road_out_of_an_obstacles_box_and_the_wrapper_equals_collect():
    """TrackletBatch: ransac_planes() estimates the road, region_depths() runs the projected-clouds export and the collect.
    The box around the board reaches down over the road in front of it.  Without the mask the histogram's first local
    maximum is a bin of road points nearer than the board; with the mask the road is gone and the bin holds the board
    (camera z 11.73 m).  Records are bit-equal to the restatement on the oracle's arrays and its estimated plane, and the
    wrapper gives what RegionDepths.collect gives on the arrays of projected_clouds()."""
    import torch
    dev = torch.device("cuda:0")
    cloud, board = road_cloud()
    n = cloud.shape[0]
    cam_model = kitti_camera()
    # (C0 refines the plane's inliers with a threshold of 10.2 m, which makes every point a ground point)
    P = C0.replace(ransac_plane_refinement_treshold=0.2)
    ref = make_oracle(P, cam_model, synth.T_CAM_LIDAR)
    ref.set_cloud(cloud)
    coeffs_ref, inl_ref = ref.estimate_ground_plane(5)
    pm = ref.pixel_map().reshape(synth.KITTI_H, synth.KITTI_W)
    index, cam = ref.point_index(), np.ascontiguousarray(ref.cloud_camera_cs().T)
    z_board = float(cam[board[0], 2])
    assert abs(z_board - 11.73) < 1e-5
    ys, xs = np.nonzero(np.isin(np.where(pm >= 0, index[np.clip(pm, 0, None)], -1), board))
    box = (int(xs.min()) - 4, int(ys.min()) - 4, int(xs.max()) + 4, int(ys.max()) + 60)  # 60 rows of road in front of the board
    boxes = np.array([box, (0, 0, synth.KITTI_W - 1, synth.KITTI_H - 1), (box[0], box[1], box[2], int(ys.max()))], dtype=np.int32)
    bits = np.zeros(n, dtype=bool)
    bits[inl_ref] = True
    assert bits.sum() == n - board.size and not bits[board].any()  # the plane's inliers are the road, all of it
    bw, mc = C0.histogram_segmentation_bin_witdh, C0.histogram_segmentation_min_pointcount
    want_plain = G.region_records(pm, index, cam, n, boxes, bw, mc)
    want_masked = G.region_records(pm, index, cam, n, boxes, bw, mc, bits)

    tb = TrackletBatch(P, cam_model, synth.T_CAM_LIDAR, 1, 16)
    try:
        tb.attach_ransac_planes(n)
        tb.attach_projected_clouds(n)
        with pytest.raises(Exception, match="attach_region_depths"):
            tb.region_depths([None], [None])
        rd = tb.attach_region_depths(8)
        clouds = [torch.from_numpy(cloud).to(dev)]
        bx = [torch.from_numpy(boxes).to(dev)]
        torch.cuda.synchronize()
        coeffs, masks, status, _ = tb.ransac_planes(clouds, [5])
        assert status[0] == 0 and np.array_equal(coeffs[0].view(np.uint32), np.asarray(coeffs_ref, dtype=np.float32).view(np.uint32))
        plain = RegionDepths.records(tb.region_depths(clouds, bx)[0])
        masked = RegionDepths.records(tb.region_depths(clouds, bx, masks)[0])
        assert not G.same_records(plain, want_plain) and not G.same_records(masked, want_masked)
        # the wrapper equals collect on the arrays of projected_clouds(), and takes that dict as well
        pc = tb.projected_clouds(clouds, cam=True, pixel_map=True)
        rec = [torch.full((3, RegionDepths.WORDS), -1, dtype=torch.int64, device=dev)]
        torch.cuda.synchronize()
        rd.collect(pc["pixel_map"], pc["index"], pc["cam"], bx, rec, masks)
        tb.est.synchronize()
        assert not G.same_records(RegionDepths.records(rec[0]), masked)
        assert not G.same_records(RegionDepths.records(tb.region_depths(pc, bx, masks)[0]), masked)
    finally:
        tb.close()
    m, p = masked[0], plain[0]
    assert m["flags"] & G.HIST_FOUND and m["hist_lower"] <= z_board < m["hist_higher"] and m["n_ground"] > 100 and m["n_points"] > 100
    assert m["z_min"] == z_board == m["z_median"] and m["n_seg"] > 100
    assert not (p["hist_lower"] <= z_board < p["hist_higher"]) and p["z_min"] < z_board - 1.0 and p["n_ground"] == 0
    assert masked[2]["flags"] & G.HIST_FOUND and masked[2]["hist_lower"] <= z_board < masked[2]["hist_higher"]
