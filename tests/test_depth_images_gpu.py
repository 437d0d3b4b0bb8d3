"""mld_depth_images_render_device (DepthImages, TrackletBatch.depth_images) against the ORACLE: OracleDepthEstimator.
calculate_depth on the grid's coordinates, with the oracle's own pixel map, point index, camera-frame cloud and plane mask
uploaded as the input arrays, so nothing here depends on the GPU projection.  The bar is helpers.assert_depth_parity: types
identical, main-path depths bit-equal, type-16 depths within DEPTH_TOL_M.  depth32 is (float32)depth bit for bit, the record
is the histogram of the types, and every output lies between guard bytes, at an odd address where its type allows.

A tile of the lane kernel is 64 x 16 grid pixels, a lane's list holds 32 entries.  Shapes and what they reach:
  1 x 1       one pixel: every window is the pixel
  64 x 64     whole tiles;  63 x 15, 64 x 16, 65 x 17   the tile's edges - 1, + 0, + 1
  65 x 7      a second tile of one column; an image lower than the windows
  70 x 37     part tiles in both directions, three rows of tiles
  130 x 20    three tiles across
  63 x 63     at density 1.0 every window is full: 70 narrow and 210 wide neighbours, all on the cooperative route
"""
import collections
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthImages, GroundPlane, TrackletBatch, capi, synth

import depth_image_frames as F
from helpers import DEPTH_TOL_M, assert_depth_parity, kitti_camera, make_estimator

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 5
C0 = capi.params_c0()
SHAPES = [(1, 1), (64, 64), (65, 7), (70, 37), (130, 20), (63, 15), (64, 16), (65, 17), (63, 63)]


class Guarded:
    """`count` elements of `dtype` between guard bytes, all of them the guard pattern before the call."""

    def __init__(self, count, dtype, dev, lead):
        import torch
        self.size = count * torch.empty(0, dtype=dtype).element_size()
        self.lead, self.dtype = lead, dtype
        self.buf = torch.full((lead + self.size + PAD,), GUARD, dtype=torch.uint8, device=dev)

    def view(self):
        return self.buf[self.lead:self.lead + self.size].view(self.dtype)

    def read(self, kind):
        """(payload as a NumPy array of `kind`, guards before and after untouched)"""
        whole = self.buf.cpu().numpy()
        ok = bool((whole[:self.lead] == GUARD).all() and (whole[self.lead + self.size:] == GUARD).all())
        return whole[self.lead:self.lead + self.size].copy().view(kind), ok


OUTPUTS = (("type", np.uint8, 3), ("depth32", np.float32, 4), ("depth", np.float64, 8))  # (name, kind, guard bytes ahead)


def prepare(frames, grid=None, tables=True, planes=True):
    """The device buffers and the arguments of one call on `frames` (one image size).  tables: True, or per output (type,
    depth32, depth) False (null table), True, or a list of S booleans.  The buffers are made on torch's stream, which nothing
    orders against the context's: torch.cuda.synchronize() before the call."""
    import torch
    dev = torch.device("cuda:0")
    S = len(frames)
    g = F.grid_of(frames[0].W, frames[0].H, grid)
    n = g[4] * g[5]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None and a.size else None  # noqa: E731
    d = dict(map=[torch.from_numpy(q.pm.reshape(-1).copy()).to(dev) for q in frames], index=[up(q.index) for q in frames],
             cam=[up(q.cam) for q in frames], mask=[up(q.mask_words()) for q in frames])
    tables = (tables,) * 3 if isinstance(tables, bool) else tables
    bufs = dict(record=Guarded(DepthImages.WORDS * S, torch.int64, dev, 8))
    kinds = dict(type=torch.uint8, depth32=torch.float32, depth=torch.float64)
    for (name, _, lead), flag in zip(OUTPUTS, tables):
        want = [bool(flag) if isinstance(flag, bool) else bool(flag[s]) for s in range(S)]
        bufs[name] = None if flag is False else [Guarded(n, kinds[name], dev, lead) if want[s] else None for s in range(S)]
    tab = lambda gs: None if gs is None else [x.view() if x is not None else None for x in gs]  # noqa: E731
    kw = dict(coeffs=np.stack([q.coeffs for q in frames]) if planes else None, masks=d["mask"] if planes else None, grid=g,
              **{name: tab(bufs[name]) for name, _, _ in OUTPUTS})
    return dict(S=S, grid=g, g=bufs, args=(d["map"], d["index"], d["cam"], bufs["record"].view()), kw=kw, keep=d)


def run(di, q):
    """Per sequence a dict: type, depth32, depth ([grid_h, grid_w] or None) and rec.  Every guard byte holds."""
    import torch
    torch.cuda.synchronize()
    di.render(*q["args"], **q["kw"])
    di._est.synchronize()
    recs, ok = q["g"]["record"].read(np.int64)
    recs = recs.view(F.DTYPE)
    gw, gh = q["grid"][4], q["grid"][5]
    out = []
    for s in range(q["S"]):
        r = dict(rec=recs[s])
        for name, kind, _ in OUTPUTS:
            gs = q["g"][name]
            r[name] = None
            if gs is not None and gs[s] is not None:
                a, good = gs[s].read(kind)
                ok = ok and good
                r[name] = a.reshape(gh, gw)
        out.append(r)
    assert ok, "a guard byte was overwritten"
    return out


def check(got, frame, grid=None, what="", plane=True):
    """One sequence against the oracle on the grid.  Returns the largest deviation of a road depth."""
    depth_ref, types_ref = frame.expected(grid)
    assert got["type"] is not None
    types = got["type"].astype(np.int32)
    dev = 0.0
    if got["depth"] is not None:
        diff = assert_depth_parity(got["depth"].reshape(-1), types.reshape(-1), depth_ref.reshape(-1), types_ref.reshape(-1))
        dev = float(diff[types_ref.reshape(-1) == 16].max(initial=0.0))
        if got["depth32"] is not None:
            assert np.array_equal(got["depth32"].view(np.uint32), got["depth"].astype(np.float32).view(np.uint32)), what
    else:
        assert np.array_equal(types, types_ref), what
        if got["depth32"] is not None:
            assert np.abs(got["depth32"].astype(np.float64) - depth_ref).max(initial=0.0) <= DEPTH_TOL_M + 98.0 * 2.0 ** -24, what
    rec = got["rec"]
    counts = np.bincount(types_ref.reshape(-1), minlength=21)
    assert np.array_equal(rec["counts"], counts), (what, rec["counts"], counts)
    assert rec["n_pixels"] == types_ref.size and rec["n_depth"] == int((depth_ref >= 0).sum()), what
    assert 0 <= rec["n_cooperative"] <= rec["n_pixels"] - counts[2] and rec["pad_"] == 0, what
    has_plane = plane and frame.plane is not None and frame.n_points > 0 and frame.P.do_use_ransac_plane  # (no points: no mask)
    assert rec["flags"] & ~F.BAD_INPUT == (F.HAS_PLANE if has_plane else 0), what
    return dev


@pytest.fixture(scope="module")
def estimators():
    """One estimator per image shape on the identity transform, the golden case's and the KITTI one; closed with their
    objects at the end."""
    made, objects = {}, []

    def obj(frame, n_seq, P=None):
        key = (frame.W, frame.H, frame.T is F.SMALL_T)
        if key not in made:
            made[key] = make_estimator(frame.P, camera=frame.cam_model, T=frame.T, max_frames=1)
        di = DepthImages(made[key], n_seq, parameters=P if P is not None else frame.P)
        objects.append(di)
        return di

    yield obj
    for di in objects:
        di.close()
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def frames():
    """The frames several tests share; their oracle answers are computed once and never changed."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = {"mixed": F.mixed_frame, "golden_c0": F.golden_frame, "grid": lambda: F.pixel_frame(70, 37, 0.5, 2)}[name]()
        return made[name]

    return get


@pytest.mark.parametrize("route", ["shipped", "ab", "ab-coop"])
@pytest.mark.parametrize("which", ["mixed", "golden_c0"])
def test_parity_frames_on_both_libraries_and_both_routes(frames, monkeypatch, which, route):
    """Every pixel of the frames that reach eleven result types, on the shipped library, on the A/B library, and on the A/B
    library with every pixel that clears the neighbour test sent through the cooperative kernel."""
    fr = frames(which)
    if route != "shipped":
        monkeypatch.setattr(capi, "_lib", capi.load_ab())
    if route == "ab-coop":
        monkeypatch.setenv("MLD_DEPTH_IMAGE_COOP", "1")
    est = make_estimator(fr.P, camera=fr.cam_model, T=fr.T, max_frames=1)
    try:
        di = DepthImages(est, 1)
        got = run(di, prepare([fr]))[0]
        dev = check(got, fr, what=(which, route))
        rec = got["rec"]
        print(f"{which} {route}: n_cooperative {rec['n_cooperative']} of {rec['n_pixels']}, largest road deviation {dev:.3e} m")
        rest = rec["n_pixels"] - rec["counts"][2]
        if route == "ab-coop":
            assert rec["n_cooperative"] == rest
        elif which == "mixed":
            assert 0 < rec["n_cooperative"] < rest  # the dense half overflows a lane's list, the sparse quarter does not
        di.close()
    finally:
        est.close()


@pytest.mark.parametrize("density", [0.05, 0.5, 1.0])
@pytest.mark.parametrize("W,H", SHAPES)
def test_image_shapes_and_densities(estimators, W, H, density):
    fr = F.pixel_frame(W, H, density, 10 * W + H)
    got = run(estimators(fr, 1), prepare([fr]))[0]
    check(got, fr, what=(W, H, density))
    if density == 1.0:  # every cell holds a point: the pixels whose narrow window (C0: half sizes 3 and 4.5) has more than 32 cells
        nx = np.minimum(np.arange(W) + 3, W - 1) - np.maximum(np.arange(W) - 3, 0) + 1
        ny = np.minimum(np.arange(H) + 4.5, H - 1).astype(int) - np.maximum(np.arange(H) - 4.5, 0).astype(int) + 1
        assert got["rec"]["n_cooperative"] >= int((ny[:, None] * nx[None, :] > 32).sum()) > 0 or W * H == 1  # (+ long road lists)


GRIDS = [(0, 0, 1, 1), (3, 2, 4, 4), (0, 0, 100, 100), (5, 7, 71, 38), (69, 36, 1, 1, 1, 1), (0, 11, 1, 1, 70, 1), (33, 0, 1, 1, 1, 37),
         (1, 0, 2, 1), (0, 1, 1, 3), (2, 3, 7, 5, 9, 6)]


@pytest.mark.parametrize("grid", GRIDS, ids=["-".join(map(str, g)) for g in GRIDS])
def test_grids_equal_the_same_pixels_of_the_full_render_bitwise(estimators, frames, grid):
    """Sub-grids, steps larger than the image, one pixel in the last corner, a single row and a single column: the oracle's
    answer, and bit for bit the pixels of the full render (a tile of a sub-grid covers other pixels than a tile of the full
    one)."""
    fr = frames("grid")
    di = estimators(fr, 1)
    full = run(di, prepare([fr]))[0]
    got = run(di, prepare([fr], grid=grid))[0]
    check(got, fr, grid, what=grid)
    x0, y0, sx, sy, gw, gh = F.grid_of(fr.W, fr.H, grid)
    pick = np.ix_(y0 + sy * np.arange(gh), x0 + sx * np.arange(gw))
    assert np.array_equal(got["type"], full["type"][pick])
    assert np.array_equal(got["depth"].view(np.uint64), full["depth"][pick].view(np.uint64))
    assert np.array_equal(got["depth32"].view(np.uint32), full["depth32"][pick].view(np.uint32))


def batch_frames(n_seq):
    """Distinct clouds; of 17: number 3 has no plane, number 5 an empty cloud, number 7 a full map."""
    W, H = 70, 37
    out = []
    for s in range(n_seq):
        density = [0.3, 0.05, 0.6, 0.2, 0.1, 0.0, 0.45, 1.0, 0.02][s % 9]
        out.append(F.pixel_frame(W, H, density, 500 + s, plane=(s != 3)))
    return out


@pytest.mark.parametrize("n_seq", [1, 3, 17])
def test_batches_of_distinct_sequences_do_not_affect_one_another(estimators, n_seq):
    """A sequence without a plane, one with an empty cloud, single output entries None; then every sequence alone gives
    the same bits."""
    seqs = batch_frames(n_seq)
    tables = ([s != 1 or n_seq == 1 for s in range(n_seq)], [s != 2 for s in range(n_seq)], [s != 0 or n_seq == 1 for s in range(n_seq)])
    got = run(estimators(seqs[0], n_seq), prepare(seqs, tables=(True, tables[1], tables[2])))
    for s, fr in enumerate(seqs):
        check(got[s], fr, what=(n_seq, s))
        assert (got[s]["depth32"] is None) == (s == 2) and (got[s]["depth"] is None) == (s == 0 and n_seq > 1)
    if n_seq == 17:
        assert got[3]["rec"]["flags"] == 0 and got[3]["rec"]["counts"][16] == 0
        assert got[5]["rec"]["counts"][2] == 70 * 37 and got[5]["rec"]["n_depth"] == 0
        alone = estimators(seqs[0], 1)
        for s, fr in enumerate(seqs):
            one = run(alone, prepare([fr]))[0]
            assert np.array_equal(one["type"], got[s]["type"]), s
            if got[s]["depth"] is not None:
                assert np.array_equal(one["depth"].view(np.uint64), got[s]["depth"].view(np.uint64)), s
            assert one["rec"].tobytes() == got[s]["rec"].tobytes(), s
    # a type table with single entries None
    got = run(estimators(seqs[0], n_seq), prepare(seqs, tables=(tables[0], False, True)))
    for s, fr in enumerate(seqs):
        assert (got[s]["type"] is None) == (s == 1 and n_seq > 1) and got[s]["depth32"] is None
        depth_ref, types_ref = fr.expected()
        assert np.array_equal(got[s]["rec"]["counts"], np.bincount(types_ref.reshape(-1), minlength=21))
        assert np.abs(got[s]["depth"] - depth_ref).max() <= DEPTH_TOL_M


PARAMETERS = {"histogram-off": dict(do_use_histogram_segmentation=0), "triangle-max-off": dict(do_use_triangle_size_maximation=0),
              "planar-check-off": dict(do_check_triangleplanar_condition=0), "ransac-plane-off": dict(do_use_ransac_plane=0)}
for _g in (0, 1):
    for _l in (0, 1):
        for _v in (0, 1):
            PARAMETERS[f"thresholds-{_g}{_l}{_v}"] = dict(treshold_depth_enabled=1, treshold_depth_local_enabled=1, treshold_depth_mode=_g,
                                                          treshold_depth_local_mode=_l, treshold_depth_local_valuetype=_v)


@pytest.mark.parametrize("name", list(PARAMETERS))
def test_parameters(estimators, name):
    """The mixed frame's cloud and a sparser one under other parameter sets; the threshold cases with bounds that cut:
    depths of 8 .. 13 m against a global interval of 9 .. 12 m and a local value of 0.02 (m, or of the interval)."""
    P = C0.replace(**PARAMETERS[name])
    if name.startswith("thresholds"):
        P = P.replace(treshold_depth_min=9, treshold_depth_max=12, treshold_depth_local_value=0.02)
    from test_coverage_maps_cpu import mixed_cloud
    import feature_trace_restatement as R
    cl = mixed_cloud()
    seqs = [F.Frame(P, F.SMALL_CAM, F.SMALL_T, cl, R.small_plane(cl)), F.pixel_frame(64, 64, 0.08, 901, P=P)]
    got = run(estimators(seqs[0], 2, P), prepare(seqs))
    seen = collections.Counter()
    for s, fr in enumerate(seqs):
        check(got[s], fr, what=(name, s))
        seen.update(fr.expected()[1].reshape(-1).tolist())
    assert seen[1] > 100 and (seen[16] > 20 or name == "ransac-plane-off")
    if name.startswith("thresholds-00"):
        assert sum(seen[t] for t in (4, 5, 6, 7)) > 20  # (the rejecting modes have their own result types)


@pytest.fixture(scope="module")
def kitti_frames():
    """Two synthetic HDL-64 frames on the KITTI camera, C0, the analytic plane."""
    scanner = synth.Scanner(64, 1024, 2.0, -24.9)
    out = []
    for seed in (3, 4):
        cloud = synth.make_cloud(scanner, seed=seed)
        out.append(F.Frame(C0, kitti_camera(), synth.T_CAM_LIDAR, cloud, synth.make_ground_plane(cloud)))
    return out


def test_kitti_size_with_road_depths_beyond_75_m(kitti_frames):
    """1242 x 375, S = 2: 20 x 24 tiles a sequence.  The road fallback is the main producer of depths here, out to more than
    75 m, where sums about the camera's origin would lose the fit."""
    est = make_estimator(C0, max_frames=1)
    try:
        di = DepthImages(est, 2)
        got = run(di, prepare(kitti_frames))
        for s, fr in enumerate(kitti_frames):
            dev = check(got[s], fr, what=("kitti", s))
            depth_ref, types_ref = fr.expected()
            road = depth_ref[types_ref == 16]
            rec = got[s]["rec"]
            print(f"kitti seed {3 + s}: {dict(collections.Counter(types_ref.reshape(-1).tolist()))}; road depths "
                  f"{road.min():.1f} .. {road.max():.1f} m; largest road deviation {dev:.3e} m; n_cooperative {rec['n_cooperative']}")
            assert (types_ref == 16).sum() > (types_ref == 1).sum() > 1000
            if s == 0:
                assert road.max() > 75.0
        di.close()
    finally:
        est.close()


def test_through_the_product_against_the_depth_call(kitti_frames):
    """TrackletBatch.projected_clouds -> .depth_images on every third pixel, against mld_calculate_depths_device at the same
    coordinates on the same cloud and plane: types equal, main-path depths bit-equal, road depths within the tolerance."""
    import torch
    fr = kitti_frames[0]
    assert fr.n_points > 1024
    dev = torch.device("cuda:0")
    grid = (1, 2, 3, 3)
    g = F.grid_of(fr.W, fr.H, grid)
    uv = F.grid_uv(g)
    tb = TrackletBatch(C0, kitti_camera(), synth.T_CAM_LIDAR, 1, uv.shape[0])
    try:
        tb.attach_projected_clouds(fr.n_points)
        tb.attach_depth_images()
        cloud = torch.from_numpy(fr.cloud).to(dev)
        mask = torch.from_numpy(fr.mask_words()).to(dev)
        pc = tb.projected_clouds([cloud], cam=True, pixel_map=True)
        out = tb.depth_images(pc, fr.coeffs[None], [mask], grid=grid, f64=True)
        assert tuple(out["type"][0].shape) == (g[5], g[4]) and out["depth32"][0].dtype == torch.float32
        tb.est.setInputCloud(fr.cloud, GroundPlane(*fr.plane))
        depth = torch.empty(uv.shape[0], dtype=torch.float64, device=dev)
        types = torch.empty(uv.shape[0], dtype=torch.int32, device=dev)
        tb.est.CalculateDepths([torch.from_numpy(uv).to(dev)], [depth], [types])
        tb.est.synchronize()
        d, t = depth.cpu().numpy(), types.cpu().numpy()
        assert_depth_parity(out["depth"][0].cpu().numpy().reshape(-1), out["type"][0].cpu().numpy().reshape(-1).astype(np.int32), d, t)
        assert np.array_equal(out["depth32"][0].cpu().numpy(), out["depth"][0].cpu().numpy().astype(np.float32))
        rec = DepthImages.records(out["record"])[0]
        assert np.array_equal(rec["counts"], np.bincount(t, minlength=21)) and rec["n_pixels"] == uv.shape[0]
        assert (t == 16).sum() > 1000 and (t == 1).sum() > 100
        bare = tb.depth_images(pc, grid=grid)
        assert bare["depth"] is None and DepthImages.records(bare["record"])[0]["counts"][16] == 0
    finally:
        tb.close()
        tb.est.close()


@pytest.mark.parametrize("route", ["shipped", "ab-coop"])
def test_three_collinear_neighbours_take_the_degenerate_plane_like_the_depth_call(monkeypatch, route):
    """16 x 16, one sequence, one grid pixel whose narrow window holds exactly three points on a line: Hyperplane::Through
    takes its smallest-eigenvector branch, on the lane route and (A/B library) on the cooperative one.  Type and depth equal
    mld_calculate_depths_device on the same cloud, bit for bit."""
    import torch
    import feature_trace_restatement as R
    from mono_lidar_depth_amd import CameraPinhole
    if route != "shipped":
        monkeypatch.setattr(capi, "_lib", capi.load_ab())
        monkeypatch.setenv("MLD_DEPTH_IMAGE_COOP", "1")
    P, cl = R.collinear_parameters(), R.collinear_cloud()
    fr = F.Frame(P, CameraPinhole(*R.COLLINEAR_CAM), F.SMALL_T, cl, None)
    px, py = R.COLLINEAR_PIXEL
    assert int((fr.pm[py - 4:py + 5, px - 3:px + 4] >= 0).sum()) == 3 == int((fr.pm >= 0).sum())
    est = make_estimator(P, camera=fr.cam_model, T=fr.T, max_frames=1)
    try:
        di = DepthImages(est, 1)
        got = run(di, prepare([fr], grid=(px, py, 1, 1, 1, 1), planes=False))[0]
        assert got["rec"]["n_pixels"] == 1 and got["rec"]["n_cooperative"] == (1 if route == "ab-coop" else 0)
        dev = torch.device("cuda:0")
        est.setInputCloud(cl)
        depth = torch.empty(1, dtype=torch.float64, device=dev)
        types = torch.empty(1, dtype=torch.int32, device=dev)
        est.CalculateDepths([torch.from_numpy(np.array([[px, py]], dtype=np.float64)).to(dev)], [depth], [types])
        est.synchronize()
        depth, types = depth.cpu().numpy(), types.cpu().numpy()
        print(f"collinear {route}: depth call type {types[0]} depth {depth[0]!r}; image type {got['type'][0, 0]} "
              f"depth {got['depth'][0, 0]!r}")
        assert int(got["type"][0, 0]) == int(types[0])
        assert np.array_equal(got["depth"].reshape(-1).view(np.int64), depth.view(np.int64))
        assert np.array_equal(got["depth32"].reshape(-1).view(np.uint32), depth.astype(np.float32).view(np.uint32))
        di.close()
    finally:
        est.close()


def test_bad_map_and_index_values_count_as_empty_cells(estimators):
    """Map values >= index_len and < -1, and index values >= n_points or negative, that still point INSIDE the allocations:
    a missing check shows as a wrong result, not as a fault.  Expected: the frame without those cells, and the flag."""
    import torch
    dev = torch.device("cuda:0")
    W, H = 70, 37
    fr, other = F.pixel_frame(W, H, 0.3, 81), F.pixel_frame(W, H, 0.3, 82)
    rng = np.random.default_rng(5)
    n_vis = fr.index.size
    cells = np.argwhere(fr.pm != -1)
    picked = cells[rng.choice(len(cells), 60, replace=False)]
    pm = fr.pm.copy()
    index = np.concatenate([np.arange(64, dtype=np.int32) % fr.n_points, fr.index, np.arange(64, dtype=np.int32) % fr.n_points])
    gone = []
    for k, (y, x) in enumerate(picked):
        gone.append(int(fr.index[fr.pm[y, x]]))
        how = k % 4
        if how == 0:
            pm[y, x] = n_vis + int(rng.integers(0, 64))
        elif how == 1:
            pm[y, x] = -2 - int(rng.integers(0, 60))
        elif how == 2:
            index[64 + fr.pm[y, x]] = fr.n_points + int(rng.integers(0, 64))
        else:
            index[64 + fr.pm[y, x]] = -1 - int(rng.integers(0, 64))
    # the same frame without those points: they lie behind the camera, so the oracle's map does not show them; the plane's
    # inliers keep their original indices
    cloud = fr.cloud.copy()
    cloud[gone, 2] = -1.0
    clean = F.Frame(C0, F.camera(W, H), F.SMALL_T, cloud, fr.plane)
    assert (clean.pm == -1).sum() == (fr.pm == -1).sum() + 60
    cam = np.concatenate([fr.cam, fr.cam[:64] + 1.0])
    call = prepare([fr, other])
    d_index = torch.from_numpy(index).to(dev)[64:64 + n_vis]
    d_cam = torch.from_numpy(cam).to(dev)[:fr.n_points]
    maps, idx, cams, rec = call["args"]
    call["args"] = ([torch.from_numpy(pm.reshape(-1)).to(dev), maps[1]], [d_index, idx[1]], [d_cam, cams[1]], rec)
    got = run(estimators(fr, 2), call)
    check(got[0], clean, what="bad")
    check(got[1], other, what="its neighbour")
    assert got[0]["rec"]["flags"] == F.BAD_INPUT | F.HAS_PLANE and got[1]["rec"]["flags"] == F.HAS_PLANE


def _tables(S=1):
    tab, zero = (C.c_void_p * S)(*[None] * S), (C.c_int64 * S)(*[0] * S)
    return dict(map=(C.c_void_p * S)(*[0x1000] * S), index=tab, index_len=zero, cam=tab, n_points=zero, coeffs=None, mask=None,
                grid=(0, 0, 1, 1, 1242, 375), depth=None, depth32=None, type=None, record=C.c_void_p(0x1000))


ONE = (C.c_int64 * 1)(1)
NULLS = (C.c_void_p * 1)(None)
AT = lambda a: (C.c_void_p * 1)(a)  # noqa: E731
REFUSALS = [
    (dict(map=None), capi.MLD_ERR_INVALID_ARG, "null table map"),
    (dict(index=None), capi.MLD_ERR_INVALID_ARG, "null table index"),
    (dict(index_len=None), capi.MLD_ERR_INVALID_ARG, "null table index_len"),
    (dict(cam=None), capi.MLD_ERR_INVALID_ARG, "null table cam"),
    (dict(n_points=None), capi.MLD_ERR_INVALID_ARG, "null table n_points"),
    (dict(record=None), capi.MLD_ERR_INVALID_ARG, "null array record_out_dev"),
    (dict(record=C.c_void_p(0x1004)), capi.MLD_ERR_INVALID_ARG, "record_out_dev must be 8-byte aligned"),
    (dict(coeffs=(C.c_float * 4)()), capi.MLD_ERR_INVALID_ARG, "coeffs and mask_dev"),
    (dict(mask=NULLS), capi.MLD_ERR_INVALID_ARG, "coeffs and mask_dev"),
    (dict(grid=(0, 0, 0, 1, 1, 1)), capi.MLD_ERR_INVALID_ARG, "step_x must be >= 1"),
    (dict(grid=(0, 0, 1, -3, 1, 1)), capi.MLD_ERR_INVALID_ARG, "step_y must be >= 1"),
    (dict(grid=(0, 0, 1, 1, 0, 1)), capi.MLD_ERR_INVALID_ARG, "grid_w must be >= 1"),
    (dict(grid=(0, 0, 1, 1, 1, 0)), capi.MLD_ERR_INVALID_ARG, "grid_h must be >= 1"),
    (dict(grid=(-1, 0, 1, 1, 1, 1)), capi.MLD_ERR_INVALID_ARG, "x0 lies outside the image"),
    (dict(grid=(1242, 0, 1, 1, 1, 1)), capi.MLD_ERR_INVALID_ARG, "x0 lies outside the image"),
    (dict(grid=(0, 375, 1, 1, 1, 1)), capi.MLD_ERR_INVALID_ARG, "y0 lies outside the image"),
    (dict(grid=(1, 0, 1, 1, 1242, 1)), capi.MLD_ERR_INVALID_ARG, "grid_w: the last column"),
    (dict(grid=(0, 0, 2147483647, 1, 3, 1)), capi.MLD_ERR_INVALID_ARG, "grid_w: the last column"),
    (dict(grid=(0, 0, 1, 2, 1, 189)), capi.MLD_ERR_INVALID_ARG, "grid_h: the last row"),
    (dict(index_len=(C.c_int64 * 1)(-1)), capi.MLD_ERR_INVALID_ARG, "negative index_len"),
    (dict(n_points=(C.c_int64 * 1)(-1)), capi.MLD_ERR_INVALID_ARG, "negative n_points"),
    (dict(n_points=(C.c_int64 * 1)(8388608)), capi.MLD_ERR_CAPACITY, "8 388 607"),
    (dict(map=NULLS), capi.MLD_ERR_INVALID_ARG, "null array map"),
    (dict(index_len=ONE), capi.MLD_ERR_INVALID_ARG, "null array index"),
    (dict(n_points=ONE), capi.MLD_ERR_INVALID_ARG, "null array cam"),
    (dict(map=AT(0x1002)), capi.MLD_ERR_INVALID_ARG, "map must be 4-byte aligned"),
    (dict(index=AT(0x1002), index_len=ONE), capi.MLD_ERR_INVALID_ARG, "index must be 4-byte aligned"),
    (dict(cam=AT(0x1004), n_points=ONE), capi.MLD_ERR_INVALID_ARG, "cam must be 8-byte aligned"),
    (dict(coeffs=(C.c_float * 4)(), mask=AT(0x1001)), capi.MLD_ERR_INVALID_ARG, "mask_dev must be 4-byte aligned"),
    (dict(depth=AT(0x1004)), capi.MLD_ERR_INVALID_ARG, "depth_out must be 8-byte aligned"),
    (dict(depth32=AT(0x1002)), capi.MLD_ERR_INVALID_ARG, "depth32_out must be 4-byte aligned"),
]


@pytest.fixture(scope="module")
def kitti_object():
    est = make_estimator(C0, max_frames=1)
    di = DepthImages(est, 1)
    yield di
    di.close()
    est.close()


@pytest.mark.parametrize("bad,code,word", REFUSALS, ids=[f"{k}-" + r[2].replace(" ", "_") for k, r in enumerate(REFUSALS)])
def test_render_refuses_with_a_text_that_names_the_function_and_the_argument(kitti_object, bad, code, word):
    """Decided on the host before anything is queued: none of the made-up addresses is touched."""
    di = kitti_object
    lib = capi.load()
    a = dict(_tables(), **bad)
    rc = lib.mld_depth_images_render_device(di._di, a["map"], a["index"], a["index_len"], a["cam"], a["n_points"], a["coeffs"], a["mask"],
                                            *a["grid"], a["depth"], a["depth32"], a["type"], a["record"])
    text = lib.mld_depth_images_last_error(di._di).decode()
    assert rc == code and text.startswith("mld_depth_images_render_device: ") and word in text, text


def test_create_refuses_a_wide_window_of_more_than_1024_cells_on_a_real_context():
    est = make_estimator(C0, max_frames=1)
    try:
        with pytest.raises(Exception) as e:
            DepthImages(est, 1, parameters=C0.replace(pixelarea_search_witdh=15, pixelarea_search_height=42))
        assert "more than 1024 cells" in str(e.value)
        di = DepthImages(est, 1, parameters=C0.replace(pixelarea_search_witdh=15, pixelarea_search_height=20))  # 32 x 32 cells
        di.close()
    finally:
        est.close()
