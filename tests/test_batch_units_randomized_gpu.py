"""The batch units' depth path - depth images, feature traces, coverage maps, nearest depths - on the random parameter
sets, cameras and rotated mountings of random_batch_setups.py, against the oracle and the restatements that
test_batch_units_randomized_cpu.py pins on the same seeds.  The unit tests of the four objects are thorough about shapes,
capacities and queueing and run at C0 with single-flag variants on the identity transform; here every seed has another
search window, other thresholds and counts, a camera whose principal point is off the centre, and a mounting rotated by
some degrees.

One small image per seed, two sequences per call: the seed's own frame, and the same scanner one frame later on ANOTHER
plane, so that a descriptor that leaks from one sequence into the other shows.  The machinery is the unit tests': their
prepare / run / check with the guarded outputs.  The bars are theirs as well: helpers.assert_depth_parity for the depth
images (types identical, main-path depths bit-equal, road depths within DEPTH_TOL_M), equality of integers and float bits
for the records of the other three.  Every test prints its largest road deviation; profiles/batch_units_random_sweep.md
keeps them."""
import contextlib

import numpy as np
import pytest

from mono_lidar_depth_amd import CoverageMaps, DepthImages, FeatureTraces, GroundPlane, NearestDepths, TrackletBatch, capi, synth

import depth_image_frames as F
import feature_trace_restatement as R
import nearest_depth_restatement as N
import test_coverage_maps_gpu as CM
import test_depth_images_gpu as DI
import test_feature_traces_gpu as FT
import test_nearest_depths_gpu as ND
from helpers import assert_depth_parity, make_estimator
from random_batch_setups import SEEDS, setup
from test_batch_units_randomized_cpu import N_FEATURES, covered, features, image_frame, once, restated, traced
from test_projected_clouds_gpu import bits
from test_randomized_gpu import _random_setup

pytestmark = pytest.mark.gpu

RADIUS_COUNT = [(4, 3), (10, 10), (24, 16), (40, 64)]
LIST_CAPACITY = 32
SECOND_PLANE = (0.004, -0.006, 1.0, 1.71)  # (the first is z = -1.73 m in the lidar frame, exactly)


def second(seed):
    """The second sequence of a call: (cloud, plane) of the seed's scanner one frame on, with a plane of its own -
    tilted, 2 cm higher, its inliers the returns within 8 cm of it."""
    def make():
        cloud = synth.make_cloud(_random_setup(seed)[3], seed=200 + seed, frame=seed % 5 + 1)
        a, b, c, d = SECOND_PLANE
        dist = np.abs(a * cloud[:, 0].astype(np.float64) + b * cloud[:, 1] + c * cloud[:, 2] + d)
        plane = (np.array(SECOND_PLANE, dtype=np.float32), np.nonzero(dist < 0.08)[0].astype(np.int32))
        assert plane[1].size > 1000
        for x in (cloud, *plane):
            x.setflags(write=False)
        return cloud, plane
    return once(("second", seed), make)


def image_frames(seed):
    """Both sequences of the seed as depth-image frames; the oracle's answers are made once."""
    P, cam, T, _, _ = setup(seed, "images")
    return [image_frame(seed), once(("image2", seed), lambda: F.Frame(P, cam, T, *second(seed)))]


def restated_frames(seed):
    """Both sequences of the seed as restated frames: the traces', the coverage maps' and the nearest depths'."""
    P, cam, T, _, _ = setup(seed, "traces")
    cloud2, plane2 = second(seed)
    return [restated(seed), once(("restated2", seed), lambda: R.Restatement(P, cloud2, plane2, cam, T))]


class Arrays:
    """The arrays of a restated frame under the names the coverage and the nearest-depth helpers read."""

    def __init__(self, fr, W, H):
        self.W, self.H = W, H
        self.pm = fr.pixel_map.reshape(H, W)
        self.index, self.index_len, self.cam, self.n_points = fr.index, fr.index.size, fr.cam, fr.n_points
        self.coeffs = np.asarray(fr.plane[0], dtype=np.float32)
        self.words = fr.mask_words().view(np.int32)

    def mask_words(self):
        return self.words


@contextlib.contextmanager
def library(route):
    """"shipped": the library as built; "ab-coop": the A/B library with every depth-image pixel that clears the neighbour
    test on the cooperative kernel."""
    with pytest.MonkeyPatch.context() as mp:
        if route != "shipped":
            mp.setattr(capi, "_lib", capi.load_ab())
            mp.setenv("MLD_DEPTH_IMAGE_COOP", "1")
        yield


def seed_grid(seed, W, H):
    """A grid with steps of 2 .. 5 and an offset below the step, from the seed."""
    rng = np.random.default_rng(5700 + seed)
    sx, sy = int(rng.integers(2, 6)), int(rng.integers(2, 6))
    return int(rng.integers(0, sx)), int(rng.integers(0, sy)), sx, sy


_RENDERED = {}


def rendered(seed, route):
    """Both sequences at every pixel and on the seed's grid, checked against the oracle; rendered once per route."""
    if (seed, route) in _RENDERED:
        return _RENDERED[(seed, route)]
    frames = image_frames(seed)
    fr = frames[0]
    grid = seed_grid(seed, fr.W, fr.H)
    with library(route):
        est = make_estimator(fr.P, camera=fr.cam_model, T=fr.T, max_frames=1)
        try:
            di = DepthImages(est, 2)
            full = DI.run(di, DI.prepare(frames))
            part = DI.run(di, DI.prepare(frames, grid=grid))
            di.close()
        finally:
            est.close()
    devs = [DI.check(full[s], q, what=(seed, route, s)) for s, q in enumerate(frames)]
    devs += [DI.check(part[s], q, grid, what=(seed, route, s, grid)) for s, q in enumerate(frames)]
    x0, y0, sx, sy, gw, gh = F.grid_of(fr.W, fr.H, grid)
    pick = np.ix_(y0 + sy * np.arange(gh), x0 + sx * np.arange(gw))
    for s in range(2):
        assert np.array_equal(part[s]["type"], full[s]["type"][pick]), (seed, route, s)
        assert np.array_equal(part[s]["depth"].view(np.uint64), full[s]["depth"][pick].view(np.uint64)), (seed, route, s)
        assert np.array_equal(part[s]["depth32"].view(np.uint32), full[s]["depth32"][pick].view(np.uint32)), (seed, route, s)
    _RENDERED[(seed, route)] = dict(full=full, dev=[max(devs[s], devs[2 + s]) for s in range(2)], grid=grid)
    return _RENDERED[(seed, route)]


@pytest.mark.parametrize("route", ["shipped", "ab-coop"])
@pytest.mark.parametrize("seed", SEEDS)
def test_depth_images_equal_the_oracle_at_every_pixel(seed, route):
    """DepthImages.render on the oracle's pixel map, point index and camera-frame cloud: every pixel of both sequences meets
    the parity bar, the record is the histogram of the oracle's types, and a second render on a grid from the seed equals
    the same pixels of the full one bit for bit."""
    r = rendered(seed, route)
    for s, got in enumerate(r["full"]):
        rec = got["rec"]
        rest = rec["n_pixels"] - rec["counts"][2]
        print(f"road-deviation images {route} seed {seed} sequence {s}: {r['dev'][s]:.3e} m (every pixel and grid {r['grid']}); "
              f"types {dict((t, int(n)) for t, n in enumerate(rec['counts']) if n)}; n_cooperative {rec['n_cooperative']} of {rest}")
        if route == "ab-coop":
            assert rec["n_cooperative"] == rest


@pytest.mark.parametrize("seed", SEEDS)
def test_both_depth_image_routes_give_the_same_types_and_main_path_bits(seed):
    """The lane kernel with its serial list walk and the cooperative kernel are two restatements of one path."""
    a, b = rendered(seed, "shipped")["full"], rendered(seed, "ab-coop")["full"]
    dev = 0.0
    for s in range(2):
        assert np.array_equal(a[s]["type"], b[s]["type"]), (seed, s)
        main = a[s]["type"] != 16
        assert np.array_equal(a[s]["depth"][main].view(np.uint64), b[s]["depth"][main].view(np.uint64)), (seed, s)
        dev = max(dev, float(np.abs(a[s]["depth"][~main] - b[s]["depth"][~main]).max(initial=0.0)))
    print(f"road-deviation images shipped-vs-ab-coop seed {seed}: {dev:.3e} m")


@pytest.mark.parametrize("seed", SEEDS)
def test_feature_traces_equal_the_restatement(seed):
    """1500 features in and around the image per sequence, list capacity 32: records and all four lists, between guard
    words; the counts of the records stay complete where a list is longer than its row."""
    P, cam, T, _, _ = setup(seed, "traces")
    frames = restated_frames(seed)
    uvs = [features(seed).copy(), features(seed, 1).copy()]  # (the shared ones are read-only)
    want = [traced(seed)[:2], once(("traced2", seed), lambda: frames[1].trace(uvs[1])[:2])]
    est = make_estimator(P, camera=cam, T=T, max_frames=1)
    try:
        ft = FeatureTraces(est, 2, N_FEATURES)
        got = FT.run(ft, FT.prepare(frames, uvs, LIST_CAPACITY))
        ft.close()
    finally:
        est.close()
    for s in range(2):
        FT.check(got[s], *want[s], LIST_CAPACITY, (seed, s))
    rec = want[0][0]
    print(f"road-deviation traces seed {seed}: 0 (records and lists bit-equal); longest lists nb {rec['n_nb'].max()} "
          f"road {rec['n_road'].max()} of capacity {LIST_CAPACITY}")


@pytest.mark.parametrize("seed", SEEDS)
def test_coverage_maps_equal_the_restatement(seed):
    """All five maps, the record and 16 x 16 buckets of both sequences, between guard bytes."""
    P, cam, T, _, _ = setup(seed, "coverage")
    frames = restated_frames(seed)
    seqs = [Arrays(q, cam.width, cam.height) for q in frames]
    want = [covered(seed), covered(seed, frames[1], second(seed)[1], "second")]
    est = make_estimator(P, camera=cam, T=T, max_frames=1)
    try:
        cm = CoverageMaps(est, 2)
        got = CM.run(cm, CM.prepare(seqs, cam.width, cam.height, bucket=(16, 16)))
        cm.close()
    finally:
        est.close()
    for s in range(2):
        CM.check(got[s], want[s], (seed, s))
    assert want[0][1]["n_buckets"] == -(-cam.width // 16) * -(-cam.height // 16)
    print(f"road-deviation coverage seed {seed}: 0 (maps, records and buckets equal); max_nb {want[0][1]['max_nb']}")


@pytest.mark.parametrize("seed", SEEDS)
def test_nearest_depths_equal_the_restatement(seed):
    """The 1500 features of both sequences at the seed's (radius, count), records and list rows between guard bytes."""
    P, cam, T, _, _ = setup(seed, "nearest")
    radius, count = RADIUS_COUNT[seed % len(RADIUS_COUNT)]
    cap = min(count, LIST_CAPACITY)
    frames = restated_frames(seed)
    seqs = [Arrays(q, cam.width, cam.height) for q in frames]
    uvs = [features(seed).copy(), features(seed, 1).copy()]  # (the shared ones are read-only)
    want = [once(("nearest", seed, s), lambda: N.records(frames[s].bare, P, seqs[s].pm, seqs[s].index, seqs[s].index_len,
                                                        seqs[s].n_points, seqs[s].cam, uvs[s], radius, count)) for s in range(2)]
    est = make_estimator(P, camera=cam, T=T, max_frames=1)
    try:
        nd = NearestDepths(est, 2, N_FEATURES, radius, count)
        got = ND.run(nd, seqs, uvs, cap=cap)
        nd.close()
    finally:
        est.close()
    for s in range(2):
        ND.check(got[s], want[s], f"seed {seed} sequence {s} radius {radius} count {count}")
    types = sorted(set(want[0][0]["type"].tolist()))
    print(f"road-deviation nearest seed {seed}: 0 (records bit-equal; no road stage); radius {radius} count {count} types {types}")


@pytest.mark.parametrize("seed", SEEDS)
def test_the_chain_from_the_projection_to_the_depth_image_and_the_traces(seed):
    """TrackletBatch on the seed's parameters, camera and rotated mounting: the projected clouds equal the oracle's bit for
    bit - pixel map, point index, camera-frame cloud and the visible image points -, the depth image rendered from them
    meets the parity bar at every pixel and agrees with mld_calculate_depths_device at the same coordinates, and the traces
    of 300 tracks on them equal the restatement."""
    import torch
    dev = torch.device("cuda:0")
    P, cam, T, cloud_h, plane = setup(seed, "images")
    fr = image_frame(seed)
    uv = F.grid_uv(F.grid_of(fr.W, fr.H))
    tracks = np.ascontiguousarray(features(seed)[:300].astype(np.float32))
    want_rec, want_lists = once(("chain-traced", seed), lambda: R.Restatement(P, cloud_h, plane, cam, T).trace(
        np.trunc(tracks.astype(np.float64)))[:2])
    depth_ref, types_ref = fr.expected()
    tb = TrackletBatch(P, cam, T, 1, uv.shape[0])
    try:
        tb.attach_projected_clouds(fr.n_points)
        tb.attach_depth_images()
        tb.attach_traces()
        cloud = torch.from_numpy(cloud_h.copy()).to(dev)
        mask = torch.from_numpy(fr.mask_words()).to(dev)
        pc = tb.projected_clouds([cloud], cam=True, pixel_map=True)
        # the projection on the rotated mounting
        m = int(pc["n_visible"].cpu().numpy()[0])
        assert m == fr.index.size
        assert np.array_equal(pc["pixel_map"][0].cpu().numpy(), fr.pm)
        assert np.array_equal(pc["index"][0][:m].cpu().numpy(), fr.index)
        assert np.array_equal(bits(pc["cam"][0].cpu().numpy()), bits(fr.cam))
        assert np.array_equal(bits(pc["uv"][0][:m].cpu().numpy()), bits(np.ascontiguousarray(fr.ref.visible_image_points().T)))
        # the depth image rendered from it, against the oracle
        out = tb.depth_images(pc, fr.coeffs[None], [mask], f64=True)
        depth = out["depth"][0].cpu().numpy()
        types = out["type"][0].cpu().numpy().astype(np.int32)
        diff = assert_depth_parity(depth.reshape(-1), types.reshape(-1), depth_ref.reshape(-1), types_ref.reshape(-1))
        dev_oracle = float(diff[types_ref.reshape(-1) == 16].max(initial=0.0))
        assert np.array_equal(out["depth32"][0].cpu().numpy().view(np.uint32), depth.astype(np.float32).view(np.uint32))
        rec = DepthImages.records(out["record"])[0]
        assert np.array_equal(rec["counts"], np.bincount(types_ref.reshape(-1), minlength=21)) and rec["n_pixels"] == uv.shape[0]
        # the traces of 300 tracks on the same export
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        u, v = f32(tracks[:, 0]), f32(tracks[:, 1])
        d = [torch.empty(300, dtype=torch.float32, device=dev) for _ in range(2)]
        f = tb.prepare([cloud], fr.coeffs[None], [mask], [u], [v], [u], [v], [torch.zeros(300, dtype=torch.uint8, device=dev)],
                       [d[0]], [d[1]])
        tr = tb.traces(f, pc, list_capacity=LIST_CAPACITY)
        assert R.same_records(FeatureTraces.records(tr["trace"][0]), want_rec) == []
        for name in R.LISTS:
            rows = tr[name][0].cpu().numpy()
            for i, ls in enumerate(want_lists):
                k = min(ls[name].size, LIST_CAPACITY)
                assert np.array_equal(rows[i, :k], ls[name][:k]), (name, i)
        # the depth call at the same coordinates
        tb.est.setInputCloud(cloud_h.copy(), GroundPlane(*plane))
        d_call = torch.empty(uv.shape[0], dtype=torch.float64, device=dev)
        t_call = torch.empty(uv.shape[0], dtype=torch.int32, device=dev)
        tb.est.CalculateDepths([torch.from_numpy(uv).to(dev)], [d_call], [t_call])
        tb.est.synchronize()
        d_call, t_call = d_call.cpu().numpy(), t_call.cpu().numpy()
        diff = assert_depth_parity(depth.reshape(-1), types.reshape(-1), d_call, t_call)
        dev_call = float(diff[t_call == 16].max(initial=0.0))
        print(f"road-deviation chain seed {seed}: {dev_oracle:.3e} m against the oracle, {dev_call:.3e} m against the depth call; "
              f"{int((types_ref == 16).sum())} road pixels of {uv.shape[0]}")
    finally:
        tb.close()
        tb.est.close()
