"""The random configurations of random_batch_setups.py without a GPU: the preconditions that keep
test_batch_units_randomized_gpu.py honest.  Per seed the restatements the GPU tests compare against hold on these
parameters, cameras and mountings - Restatement.trace runs through its own assertions, coverage_restatement agrees with
the oracle's trace, nearest_depth_restatement.main_path is the oracle's main path -, and the seeds together reach what the
GPU tests are there for: every result type, road fits on windows two or three pixels wide, lists beyond a lane's 32
entries, the histogram off.  What both files need of a seed is made here, once, and left unchanged."""
import collections

import numpy as np
import pytest

import coverage_restatement as V
import depth_image_frames as F
import feature_trace_restatement as R
from random_batch_setups import SEEDS, UNITS, setup, wide_window
from test_nearest_depths_cpu import _main_path_against_the_oracle
from test_randomized_gpu import _random_setup

N_FEATURES = 1500
_MADE = {}


def once(key, make):
    if key not in _MADE:
        _MADE[key] = make()
    return _MADE[key]


def features(seed, which=0):
    """1500 features uniform in [-2, W + 2] x [-2, H + 2] of the seed's image, every other one on an integer pixel;
    which: 0 for the seed's own sequence, 1 for the second sequence of the GPU tests."""
    def make():
        cam = setup(seed, "traces")[1]
        rng = np.random.default_rng(5300 + 100 * which + seed)
        uv = np.stack([rng.uniform(-2.0, cam.width + 2.0, N_FEATURES), rng.uniform(-2.0, cam.height + 2.0, N_FEATURES)], axis=1)
        uv[::2] = np.floor(uv[::2])
        uv = np.ascontiguousarray(uv)
        uv.setflags(write=False)
        return uv
    return once(("features", seed, which), make)


def image_frame(seed):
    """The depth images' frame of the seed: the oracle's arrays and, from expected(), its answer at every pixel."""
    return once(("image", seed), lambda: F.Frame(*setup(seed, "images")))


def restated(seed):
    """The traces' frame of the seed; the coverage maps and the nearest depths have the same parameters."""
    def make():
        P, cam, T, cloud, plane = setup(seed, "traces")
        return R.Restatement(P, cloud, plane, cam, T)
    return once(("restated", seed), make)


def traced(seed):
    """(records, lists, the oracle's final (types, depths)) of features(seed) on restated(seed)."""
    def make():
        rec, lists, final = restated(seed).trace(features(seed))
        rec.setflags(write=False)
        return rec, lists, final
    return once(("traced", seed), make)


def plane_bits(n_points, plane):
    bits = np.zeros(n_points, dtype=bool)
    bits[np.asarray(plane[1], dtype=np.int64)] = True
    return bits


def covered(seed, fr=None, plane=None, key=None):
    """(maps, record, 16 x 16 buckets) of the coverage restatement on a restated frame (default: the seed's own)."""
    def make():
        P, cam, _, _, own = setup(seed, "coverage")
        q = fr if fr is not None else restated(seed)
        pl = plane if plane is not None else own
        want = V.coverage(P, q.pixel_map.reshape(cam.height, cam.width), q.index, q.cam, q.n_points, q.Tinv, pl[0],
                          plane_bits(q.n_points, pl), bucket=(16, 16))
        for a in want[0].values():
            a.setflags(write=False)
        return want
    return once(("covered", seed, key), make)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_setups_differ_from_the_generator_only_where_a_unit_refuses(seed):
    """Camera scaled by 1/4 (1/8 beyond 1242 columns), do_use_PCA off, for the depth images the M-estimator road fit; the
    windows within what the units accept; traces, coverage maps, nearest depths and row growth on one parameter set (the
    generator never draws set_all_depths_to_zero, which the row growth refuses as well)."""
    P0, cam0, T0, _, kw = _random_setup(seed)
    k = 8 if cam0.width > 1242 else 4
    seen = {}
    for unit in UNITS:
        P, cam, T, cloud, plane = setup(seed, unit)
        seen[unit] = bytes(P)
        assert (cam.width, cam.height) == (cam0.width // k, cam0.height // k)
        assert (cam.focal_length, cam.principal_point_x, cam.principal_point_y) == (
            cam0.focal_length / k, cam0.principal_point_x / k, cam0.principal_point_y / k)
        assert np.array_equal(T, T0) and cloud.shape[0] > 10000 and plane[1].size > 1000
        changed = {n for n in kw if getattr(P, n) != getattr(P0, n)}
        assert changed <= {"do_use_PCA", "plane_estimator_use_triangle_maximation", "plane_estimator_use_mestimator"}
        assert unit == "images" or changed <= {"do_use_PCA"}
        assert not P.do_use_PCA and not P.set_all_depths_to_zero and not P0.set_all_depths_to_zero
        if unit == "images":
            assert not P.plane_estimator_use_triangle_maximation and P.plane_estimator_use_mestimator
        nx, ny = wide_window(P, cam.width, cam.height)
        assert nx <= 30 and ny <= 23  # (the generator's search areas are at most 14 x 14)
        assert nx <= 64 and ny <= 64 and nx * ny <= 1024
    assert seen["traces"] == seen["coverage"] == seen["nearest"] == seen["rows"]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_trace_restatement_runs_through_its_assertions(seed):
    """Restatement.trace checks the oracle's trace against the parts it restates - the histogram's bin, the far test, the
    road states - on every feature: 1500 of them, in and around the image."""
    uv = features(seed)
    cam = setup(seed, "traces")[1]
    assert uv.shape == (N_FEATURES, 2) and (uv[::2] == np.floor(uv[::2])).all() and (uv[1::2] != np.floor(uv[1::2])).any()
    assert uv.min() < 0.0 and uv[:, 0].max() > cam.width and uv[:, 1].max() > cam.height
    rec, lists, (types, depth) = traced(seed)
    assert rec.size == N_FEATURES == len(lists)
    assert len(set(rec["main_type"].tolist())) >= 3  # (an empty class cannot pass silently)
    P = setup(seed, "traces")[0]
    assert P.do_use_ransac_plane or (rec["road_state"] == R.NOT_REACHED).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_coverage_restatement_agrees_with_the_oracles_trace(seed):
    """The fields test_the_restatement_agrees_with_the_oracles_trace_of_every_pixel compares, on every pixel of the first
    and last two rows and columns and 2000 random ones.  A map saturates at 255; the lists here reach beyond that."""
    P, cam, _, _, plane = setup(seed, "coverage")
    W, H = cam.width, cam.height
    fr = restated(seed)
    maps, rec, _ = covered(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    border = (ys < 2) | (ys >= H - 2) | (xs < 2) | (xs >= W - 2)
    rng = np.random.default_rng(5500 + seed)
    flat = np.union1d(np.nonzero(border.reshape(-1))[0], rng.choice(W * H, 2000, replace=False))
    assert flat.size >= 2000
    sat = lambda n: min(int(n), 255)  # noqa: E731
    for k in flat:
        y, x = divmod(int(k), W)
        t = fr.ref.trace_feature(float(x), float(y))
        reach = int(maps["reach"][y, x])
        assert sat(len(t["nb_idx"])) == maps["nb"][y, x], (x, y)
        assert (t["type"] == 2) == (not reach & 1), (x, y)
        if t["type"] == 16:
            assert reach & 2, (x, y)
        if t["reached_road"]:  # the oracle scanned the wide window; it walked all of it unless a neighbour was far
            assert sat(len(t["road_idx"])) == maps["road"][y, x], (x, y)
            if maps["road_far"][y, x] == 0:
                assert sat(len(t["road_pos"])) == maps["road_inl"][y, x], (x, y)
                assert (len(t["road_pos"]) >= 3) == bool(reach & 2), (x, y)
            else:
                assert len(t["road_pos"]) == 0 and not reach & 2, (x, y)
    seen = collections.Counter(maps["reach"].reshape(-1).tolist())
    assert seen[0] and seen[1] and not seen[2]
    assert rec["n_reach"] == seen[1] + seen[3] and rec["n_reach_road"] == seen[3]
    if P.do_use_ransac_plane:
        assert seen[3] and rec["n_inlier"] > 0 and rec["flags"] == V.HAS_PLANE
    else:
        assert not seen[3] and rec["flags"] == 0 and rec["n_inlier"] == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_main_path_is_the_oracle_on_the_windows_own_list(seed):
    """nearest_depth_restatement.main_path on trace_feature's list against calculate_depth with the road off: types
    identical, depths bit for bit, on the 1500 features."""
    P, cam, T, cloud, _ = setup(seed, "nearest")
    seen = _main_path_against_the_oracle(P, cam, T, cloud, features(seed))
    assert len(seen) >= 3, seen


# ---- what the seeds reach together ------------------------------------------------------------------------------------------

ALL_TYPES = {1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 16}


def test_the_seeds_together_reach_every_result_type_narrow_road_fits_long_lists_and_the_histogram_off():
    types = collections.Counter()
    narrow, long_lists, no_histogram = [], [], []
    for seed in SEEDS:
        fr = image_frame(seed)
        _, t = fr.expected()
        types.update(t.reshape(-1).tolist())
        if fr.P.pixelarea_search_witdh <= 3 and int((t == 16).sum()) >= 500:
            narrow.append(seed)
        if covered(seed)[1]["max_nb"] > 32:
            long_lists.append(seed)
        if not fr.P.do_use_histogram_segmentation:
            no_histogram.append(seed)
    print(f"types {sorted(types.items())}; narrow road fits on seeds {narrow}; narrow lists beyond 32 entries on {long_lists}; "
          f"histogram off on {no_histogram}")
    assert ALL_TYPES <= {k for k, n in types.items() if n > 0}, sorted(types.items())
    assert len(narrow) >= 3 and len(long_lists) >= 3 and len(no_histogram) >= 2


@pytest.mark.parametrize("seed", SEEDS)
def test_no_road_depth_of_a_seed_lies_a_kilometre_away(seed):
    """Far estimates of nearly collinear returns are the one class no two f64 decompositions agree on to 1e-4 m (LAB.md
    6.25); without them the plain bar applies at every pixel."""
    d, t = image_frame(seed).expected()
    road = d[t == 16]
    assert np.isfinite(road).all() and (np.abs(road) < 1000.0).all(), float(np.abs(road).max(initial=0.0))
