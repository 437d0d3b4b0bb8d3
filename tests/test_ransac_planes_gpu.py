"""mld_ransac_planes_estimate_device (RansacPlanes, TrackletBatch.ransac_planes) against the oracle's
estimate_ground_plane and against the one-slot path mld_estimate_ground_plane: coefficients as raw bits, the inlier set,
its size and the status must be EQUAL - draws, stopping rule and the association of the float sums are fixed, there is
no tolerance.

Point counts and what they reach (a wavefront takes 64 points, a block of the pass-through 1024, the sample is 6000):
  0, 1, 2            no model: status 1
  3, 4               the smallest samples (4: the refinement needs more than 3 inliers)
  63, 64, 65         one word of the sample bitmask, not full / full / a second one; 65 points = 3 mask words (odd)
  1023, 1024, 1025   a second chunk of the pass-through
  5999, 6000, 6001   the sample: all points / all points / stratified positions, which may repeat
  6143, 20 000       96 words of 64 positions would be needed for 6144; a sample that is a fraction of the cloud
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import RansacPlane, RansacPlanes, TrackletBatch, capi, synth
from oracle import oracle

from helpers import assert_depth_parity, kitti_camera, make_estimator, make_oracle

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 5999, 6000, 6001, 6143, 20000)
GUARD = 0x5A5AA5A5
PAD = 3
WINDOW = dict(ransac_plane_min_z=-1.72, ransac_plane_max_z=-1.68)


def plane_cloud(n, seed, noise=0.02, z0=-1.7):
    rng = np.random.default_rng(seed)
    cl = np.zeros((n, 4), np.float32)
    cl[:, 0] = rng.uniform(2, 40, n)
    cl[:, 1] = rng.uniform(-15, 15, n)
    cl[:, 2] = z0 + 0.01 * cl[:, 0] + rng.normal(0, noise, n)
    return cl


def share_cloud(n, frac, seed):
    """A 1 cm-noise plane at z = -1.7 holding a share `frac` of n points, the rest uniform in z in [-1.5, 3]."""
    rng = np.random.default_rng(seed)
    cl = np.zeros((n, 4), np.float32)
    cl[:, 0] = rng.uniform(2, 40, n)
    cl[:, 1] = rng.uniform(-15, 15, n)
    cl[:, 2] = rng.uniform(-1.5, 3.0, n)
    on = rng.permutation(n)[:int(round(frac * n))]
    cl[on, 2] = -1.7 + rng.normal(0, 0.01, on.size)
    return cl


def window_cloud(n, k, seed):
    """n points of which exactly k lie inside the z window [-1.72, -1.68] (the others in [-1.5, 3])."""
    rng = np.random.default_rng(seed)
    cl = np.zeros((n, 4), np.float32)
    cl[:, 0] = rng.uniform(2, 40, n)
    cl[:, 1] = rng.uniform(-15, 15, n)
    cl[:, 2] = rng.uniform(-1.5, 3.0, n)
    inside = rng.permutation(n)[:k]
    cl[inside, 2] = rng.uniform(-1.71, -1.69, k)
    return cl


def candidates_of(P, cloud):
    """The NumPy count of the points the z pass-through keeps (all of them when it is off)."""
    if not P.ransac_plane_min_z > -1001.0:
        return int(cloud.shape[0])
    lo, hi = np.float32(P.ransac_plane_min_z), np.float32(P.ransac_plane_max_z)
    ok = np.isfinite(cloud[:, :3]).all(axis=1) & ~(cloud[:, 2] < lo) & ~(cloud[:, 2] > hi)
    return int(ok.sum())


def mask_of(inl, n):
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, np.uint32(1) << (inl & 31).astype(np.uint32))
    return m


_WANT = {}


def expected(P, cloud, seed, key=None):
    """(coeffs float32[4], inliers ascending int32, status, n_candidates) from the oracle; computed once per key."""
    if key is not None and key in _WANT:
        return _WANT[key]
    n = cloud.shape[0]
    want = None
    if n >= 3:
        ref = make_oracle(P)
        ref.set_cloud(cloud)
        try:
            coeffs, inl = ref.estimate_ground_plane(seed)
            want = (coeffs, inl, 0, candidates_of(P, cloud))
        except RuntimeError:
            pass
    if want is None:
        want = (np.zeros(4, np.float32), np.empty(0, np.int32), 1, candidates_of(P, cloud))
    if key is not None:
        _WANT[key] = want
    return want


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def est():
    e = make_estimator(capi.params_c0(), max_frames=1)
    yield e
    e.close()


def device_cloud(cloud, stride, dev, offset):
    """The cloud on the device: 16- or 32-byte records, optionally one float behind a 16-byte boundary."""
    import torch
    n = cloud.shape[0]
    width = stride // 4
    host = np.full((n, width), np.nan, dtype=np.float32)  # (what lies behind x, y, z must not matter)
    host[:, :4] = cloud
    if n == 0:
        return None
    buf = torch.empty(n * width + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + n * width] if offset else buf[:n * width]
    view.copy_(torch.from_numpy(host.reshape(-1)).to(dev))
    view = view.view(n, width)
    assert view.data_ptr() % 16 == (4 if offset else 0) and view.is_contiguous()
    return view


def mask_buffers(ns, dev, misalign):
    """Per sequence a guarded buffer and the view handed to the call: `words` entries between guard words."""
    import torch
    bufs, views = [], []
    for n in ns:
        w = (n + 31) // 32
        lead = 1 if misalign else 2  # (the mask starts at an odd / an even word)
        b = torch.full((lead + w + PAD,), GUARD, dtype=torch.int32, device=dev)
        v = b[lead:lead + w] if w else None
        if w:
            assert v.data_ptr() % 8 == (4 if misalign else 0)
        bufs.append((b, lead))
        views.append(v)
    return bufs, views


def run(est, P, clouds, seeds, stride=16, offset=False, misalign=False, rp=None, max_points=None):
    """One call; returns [(coeffs, n_inliers, iterations, status, n_candidates, mask words, guards untouched)]."""
    import torch
    dev = torch.device("cuda:0")
    S = len(clouds)
    ns = [c.shape[0] for c in clouds]
    d_clouds = [device_cloud(c, stride, dev, offset) for c in clouds]
    res = torch.full((S, 8), -1, dtype=torch.int32, device=dev)
    bufs, views = mask_buffers(ns, dev, misalign)
    torch.cuda.synchronize()
    own = rp is None
    if own:
        rp = RansacPlanes(est, S, max_points or max(max(ns), 1), parameters=P)
    rp.estimate(d_clouds, seeds, res, views)
    est.synchronize()
    if own:
        rp.close()
    r = res.cpu().numpy()
    out = []
    for s, n in enumerate(ns):
        w = (n + 31) // 32
        whole, lead = bufs[s][0].cpu().numpy(), bufs[s][1]
        guard_ok = bool((whole[:lead] == GUARD).all() and (whole[lead + w:] == GUARD).all())
        out.append((r[s, :4].copy().view(np.float32), int(r[s, 4]), int(r[s, 5]), int(r[s, 6]), int(r[s, 7]),
                    whole[lead:lead + w].copy().view(np.uint32), guard_ok))
    return out


def check(got, want, n, what=""):
    coeffs, n_inl, iterations, status, n_cand, mask, guard_ok = got
    w_coeffs, w_inl, w_status, w_cand = want
    assert guard_ok, what
    assert status == w_status, (what, status, w_status)
    assert n_cand == w_cand, (what, n_cand, w_cand)
    assert np.array_equal(bits(coeffs), bits(w_coeffs)), (what, coeffs, w_coeffs)
    assert mask.size == (n + 31) // 32
    idx = np.flatnonzero(np.unpackbits(mask.view(np.uint8), bitorder="little")).astype(np.int32)
    assert np.array_equal(idx, w_inl), (what, idx.size, w_inl.size)
    assert n_inl == w_inl.size, (what, n_inl, w_inl.size)
    if status == 1:
        assert iterations == 0 and not coeffs.view(np.uint32).any() and not mask.any(), what


def check_all(P, clouds, seeds, got, tag):
    for s, (c, g) in enumerate(zip(clouds, got)):
        check(g, expected(P, c, seeds[s], key=(tag, s)), c.shape[0], f"{tag}[{s}] n={c.shape[0]}")


def size_case():
    clouds = [plane_cloud(n, 100 + n) for n in SIZES]
    seeds = [500 + 7 * k for k in range(len(SIZES))]
    return clouds, seeds


@pytest.mark.parametrize("stride,offset,misalign", [(16, False, False), (32, False, False), (16, True, True), (32, True, True)])
def test_the_sizes_in_one_call_of_16_sequences_equal_the_oracle(est, stride, offset, misalign):
    """Every boundary size in ONE call, in every layout: stride 16 and 32, cloud bases at 4 (mod 16), masks that start at
    an odd word; the guard words before and after every mask stay untouched (65 points: 3 words, 1025: 33)."""
    P = capi.params_c0()
    assert not P.ransac_plane_min_z > -1001.0  # C0: the pass-through is off
    clouds, seeds = size_case()
    got = run(est, P, clouds, seeds, stride=stride, offset=offset, misalign=misalign)
    check_all(P, clouds, seeds, got, "sizes")
    for n, g in zip(SIZES, got):
        assert g[3] == (1 if n < 3 else 0), n
        assert g[4] == n
        if 3 <= n <= 6000:
            assert g[1] == n, n  # every point within C0's refinement threshold 10.2
    assert got[SIZES.index(6001)][1] < 6000  # stratified positions repeat


PARAM_SETS = {
    "c0": {},
    "thr 0.05": dict(ransac_plane_distance_treshold=0.05, ransac_plane_refinement_treshold=0.05),
    "no refinement": dict(ransac_plane_use_refinement=0),
    "max_it 0": dict(ransac_plane_max_iterations=0),
    "max_it 5": dict(ransac_plane_max_iterations=5),
    "max_it 25": dict(ransac_plane_max_iterations=25, ransac_plane_distance_treshold=0.05, ransac_plane_refinement_treshold=0.05),
    "max_it 64": dict(ransac_plane_max_iterations=64, ransac_plane_distance_treshold=0.05, ransac_plane_refinement_treshold=0.05),
    "max_it 10000": dict(ransac_plane_max_iterations=10000, ransac_plane_distance_treshold=0.05,
                         ransac_plane_refinement_treshold=0.05),
}


def param_clouds():
    return [plane_cloud(300, 1), plane_cloud(5000, 2, noise=0.1), share_cloud(9000, 0.25, 3), share_cloud(9000, 0.15, 4),
            synth.make_cloud(synth.VLP16, seed=5, frame=2)]


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_parameter_sets_equal_the_oracle(est, name):
    P = capi.params_c0().replace(**PARAM_SETS[name])
    clouds = param_clouds()
    seeds = [40 + s for s in range(len(clouds))]
    got = run(est, P, clouds, seeds)
    check_all(P, clouds, seeds, got, name)
    assert sum(g[3] == 0 for g in got) >= len(got) - 1
    if name == "max_it 0":
        # one draw: counted (then iterations > max_iterations), or skipped - no model.  A first draw that is no plane
        # within 10 degrees of the z axis is adopted with 0 inliers.
        assert all(g[2] == (1 if g[3] == 0 else 0) for g in got)
        assert any(g[3] == 0 and g[1] == 0 for g in got)
    else:
        assert all(g[3] == 0 for g in got)


def frame_estimate_iterations(P, cloud, seed):
    """plane_out.iterations of mld_calculate_depth_frame_estimate on the same cloud and seed."""
    e = make_estimator(P)
    gp = RansacPlane(seed=seed)
    e.CalculateDepth(cloud, synth.make_features(64, seed=1), gp)
    it, coeffs = gp.iterations, np.asarray(gp.getModelCoeffs(), dtype=np.float32)
    e.close()
    return it, coeffs


@pytest.mark.parametrize("more_than,fracs", [(64, (0.3, 0.25, 0.2)), (1088, (0.15, 0.12, 0.1, 0.08))])
def test_the_stopping_rule_beyond_the_first_wavefront_of_draws_and_beyond_an_epoch(est, more_than, fracs):
    """9000 points with a small inlier share, thresholds 0.05: PCL's bound k = log(1 - p) / log(1 - w^3) is about 250 at
    w = 0.3 and about 2000 at w = 0.15, so the estimator goes beyond its first 64 draws / beyond several epochs of 256.
    The share is lowered until the GPU's record says so; the iteration count equals the one-frame path's."""
    P = capi.params_c0().replace(ransac_plane_distance_treshold=0.05, ransac_plane_refinement_treshold=0.05)
    seed = 77
    for frac in fracs:
        cloud = share_cloud(9000, frac, 9)
        got = run(est, P, [cloud], [seed])[0]
        print(f"frac {frac}: iterations {got[2]}, inliers {got[1]}")
        if got[2] > more_than:
            break
    assert got[2] > more_than and got[3] == 0, (got[2], more_than)
    check(got, expected(P, cloud, seed), 9000, f"frac {frac}")
    it, coeffs = frame_estimate_iterations(P, cloud, seed)
    assert it == got[2], (it, got[2])
    assert np.array_equal(bits(coeffs), bits(got[0]))


def test_the_z_pass_through_window(est):
    """Window [-1.72, -1.68]: 6 / 9 / 297 / 784 candidates among 64 / 300 / 7000 / 20 000 points, exactly three, exactly
    two, more than the sample holds; n_candidates equals the NumPy count; at C0's thresholds every candidate of a
    sampled position is an inlier."""
    P = capi.params_c0().replace(**WINDOW)
    shapes = [(64, 6), (300, 9), (7000, 297), (20000, 784), (500, 3), (500, 2), (20000, 7000), (1025, 1025), (2, 2)]
    clouds = [window_cloud(n, k, 200 + i) for i, (n, k) in enumerate(shapes)]
    seeds = [90 + i for i in range(len(clouds))]
    got = run(est, P, clouds, seeds)
    check_all(P, clouds, seeds, got, "window")
    for (n, k), g in zip(shapes, got):
        assert g[4] == k, (n, k, g[4])
        assert g[3] == (1 if k < 3 else 0), (n, k)
        if 3 <= k <= 6000:
            assert g[1] == k, (n, k, g[1])
    assert 0 < got[6][1] <= 6000


def test_long_sequences_whose_chunk_counts_leave_the_first_wavefront_and_the_first_round_of_the_scan(est):
    """One call on an object of max_points 262 145 with the z window on: the prefix over the chunk counts of the
    pass-through crosses from wavefront 0 to wavefront 1 (65 537 points: 65 chunks) and carries into a second round of 256
    chunks (262 145 points: 257 chunks, the last of one point); the sample is drawn through that prefix."""
    P = capi.params_c0().replace(**WINDOW)
    shapes = [(65537, 20001), (262145, 80003), (1, 1)]
    clouds = [window_cloud(n, k, 300 + i) for i, (n, k) in enumerate(shapes)]
    seeds = [70 + i for i in range(len(clouds))]
    got = run(est, P, clouds, seeds, max_points=262145)
    check_all(P, clouds, seeds, got, "long window")
    for (n, k), g in zip(shapes, got):
        assert g[4] == k and g[3] == (1 if k < 3 else 0), (n, k, g[3], g[4])


def test_a_window_that_holds_nothing_and_clouds_of_nan(est):
    none = capi.params_c0().replace(ransac_plane_min_z=5.0, ransac_plane_max_z=6.0)
    clouds = [plane_cloud(300, 1), plane_cloud(7000, 2)]
    got = run(est, none, clouds, [1, 2])
    check_all(none, clouds, [1, 2], got, "window 5..6")
    assert all(g[3] == 1 and g[4] == 0 for g in got)
    nan_all = np.full((500, 4), np.nan, np.float32)
    third = plane_cloud(3000, 8)
    third[::3] = np.nan
    wide = capi.params_c0().replace(ransac_plane_min_z=-1000.0, ransac_plane_max_z=1000.0)
    for tag, P in (("nan, off", capi.params_c0()), ("nan, on", wide)):
        got = run(est, P, [nan_all, third], [3, 4])
        check_all(P, [nan_all, third], [3, 4], got, tag)
        assert got[0][3] == 1 and got[0][4] == (500 if tag == "nan, off" else 0)
        assert got[1][3] == 0 and got[1][1] == 2000


def test_a_vertical_wall_adopts_its_first_draw_without_inliers(est):
    """tests/test_ransac_gpu.py, test_no_horizontal_plane_in_the_cloud: no draw is within 10 degrees of the z axis."""
    rng = np.random.default_rng(3)
    n = 5000
    wall = np.stack([np.full(n, 10.0), rng.uniform(-20, 20, n), rng.uniform(-2, 3, n), np.zeros(n)], axis=1).astype(np.float32)
    P = capi.params_c0()
    got = run(est, P, [wall], [1])[0]
    want = expected(P, wall, 1)
    assert want[2] == 0 and want[1].size == 0 and abs(abs(want[0][0]) - 1.0) < 1e-3
    check(got, want, n, "wall")
    assert got[2] == P.ransac_plane_max_iterations + 1  # every draw counted


@pytest.mark.parametrize("window", [False, True])
def test_two_calls_on_one_object_read_no_stale_scratch(est, window):
    """The second call has smaller clouds and other seeds."""
    P = capi.params_c0().replace(**WINDOW) if window else capi.params_c0()
    first = [window_cloud(20000, 7000, 1), window_cloud(7000, 297, 2), plane_cloud(6001, 3)]
    second = [window_cloud(300, 9, 4), window_cloud(1500, 100, 5), plane_cloud(65, 6, z0=-1.9)]
    rp = RansacPlanes(est, 3, 20000, parameters=P)
    for tag, clouds, seeds in (("first", first, [1, 2, 3]), ("second", second, [11, 12, 13])):
        got = run(est, P, clouds, seeds, rp=rp)
        check_all(P, clouds, seeds, got, f"reuse {window} {tag}")
    rp.close()


@pytest.mark.parametrize("n_seq", [1, 3, 13])
def test_object_sizes_with_an_empty_sequence_in_the_middle(est, n_seq):
    P = capi.params_c0().replace(ransac_plane_min_z=-2.2, ransac_plane_max_z=-0.9)
    sizes = [777, 0, 4100, 64, 9000, 3, 1024, 130, 6001, 2, 257, 5, 2049][:n_seq]
    if n_seq == 1:
        sizes = [777]
    clouds = [plane_cloud(n, 300 + n) for n in sizes]
    seeds = [60 + s for s in range(n_seq)]
    got = run(est, P, clouds, seeds, max_points=9000)
    check_all(P, clouds, seeds, got, f"n_seq {n_seq}")


@pytest.mark.parametrize("window", [False, True])
def test_equal_to_the_one_slot_path(window):
    """mld_estimate_ground_plane + mld_get_ground_plane_inliers on a slot against the batched call, same inputs."""
    import torch
    dev = torch.device("cuda:0")
    P = capi.params_c0().replace(ransac_plane_min_z=-2.2, ransac_plane_max_z=-0.9) if window else capi.params_c0()
    e = make_estimator(P, max_frames=1)
    clouds = [synth.make_cloud(synth.VLP16, seed=21, frame=1), plane_cloud(6001, 22), share_cloud(9000, 0.3, 23)]
    seeds = [5, 6, 7]
    got = run(e, P, clouds, seeds)
    for cloud, seed, g in zip(clouds, seeds, got):
        d_cloud = torch.from_numpy(cloud).to(dev)
        e.setInputCloud(d_cloud, None, plane_given=False)
        c_one, n_one = e.estimateGroundPlane(0, seed)
        inl = e.getGroundPlaneInliers()
        assert g[3] == 0 and g[1] == n_one == inl.size and n_one >= 3
        assert np.array_equal(bits(g[0]), bits(c_one))
        assert np.array_equal(g[5], mask_of(inl, cloud.shape[0])) and g[6]
    e.close()


def test_arguments_are_refused_by_name(est):
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    st = C.c_int(0)
    P = capi.params_c0()
    assert not lib.mld_ransac_planes_create(est._ctx, 2, 100, None, C.byref(st)) and st.value == capi.MLD_ERR_INVALID_ARG
    assert "params" in lib.mld_ransac_planes_last_error(None).decode()
    rp = lib.mld_ransac_planes_create(est._ctx, 2, 100, C.byref(P), C.byref(st))
    assert rp and st.value == capi.MLD_OK
    cloud = torch.zeros((101, 4), dtype=torch.float32, device=dev)
    mask = torch.full((4 + PAD,), GUARD, dtype=torch.int32, device=dev)
    res = torch.full((2, 8), -1, dtype=torch.int32, device=dev)
    tab = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())  # noqa: E731
    half = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)  # noqa: E731
    odd = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr() + 2)  # noqa: E731
    good = dict(pts=tab(cloud), n=(C.c_int64 * 2)(100, 100), stride=16, seeds=(C.c_uint32 * 2)(1, 2), res=res.data_ptr(),
                mask=tab(mask))

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.mld_ransac_planes_estimate_device(rp, a["pts"], a["n"], a["stride"], a["seeds"], a["res"], a["mask"])
        return rc, lib.mld_ransac_planes_last_error(rp).decode()

    torch.cuda.synchronize()
    for kw, word in ((dict(pts=None), "pts_dev"), (dict(n=None), "table n"), (dict(seeds=None), "seeds"),
                     (dict(res=None), "result_out_dev"), (dict(mask=None), "mask_out_dev"), (dict(stride=12), "stride_bytes"),
                     (dict(stride=64), "stride_bytes"), (dict(n=(C.c_int64 * 2)(100, -1)), "negative n"),
                     (dict(pts=half(cloud)), "pts_dev"), (dict(mask=half(mask)), "mask_out_dev"),
                     (dict(pts=odd(cloud)), "4-byte aligned"), (dict(mask=odd(mask)), "4-byte aligned")):
        rc, text = call(**kw)
        assert rc == capi.MLD_ERR_INVALID_ARG and word in text and "mld_ransac_planes_estimate_device" in text, (kw, text)
    rc, text = call(n=(C.c_int64 * 2)(100, 101))
    assert rc == capi.MLD_ERR_CAPACITY and "max_points" in text
    est.synchronize()
    assert (mask.cpu().numpy() == GUARD).all() and (res.cpu().numpy() == -1).all()  # nothing was launched
    # a sequence without points needs no arrays and gets its record only; a cloud of zeros has no model
    rc, text = call(n=(C.c_int64 * 2)(100, 0), pts=half(cloud), mask=half(mask))
    assert rc == capi.MLD_OK, text
    est.synchronize()
    r = res.cpu().numpy()
    assert (r[:, 6] == 1).all() and not r[:, :6].any() and r[:, 7].tolist() == [100, 0]
    m = mask.cpu().numpy()
    assert not m[:4].any() and (m[4:] == GUARD).all()
    lib.mld_ransac_planes_destroy(rp)


def test_tracklet_batch_with_its_own_ransac_planes_equals_the_oracle():
    """Three sequences of HDL-64 clouds, two frames (both banks): TrackletBatch.run with the planes of ransac_planes()
    against the per-sequence oracle with ITS estimated plane.  In the second frame one sequence has a cloud of two
    points: status 1, zero coefficients and an empty mask go to prepare(), and the oracle runs that frame without a
    plane (with two points no feature finds neighbours either way)."""
    import torch
    dev = torch.device("cuda:0")
    P, cam, S, NT = capi.params_c0(), kitti_camera(), 3, 300
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(23)
    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, NT)
    tb.attach_ransac_planes(synth.HDL64.rings * synth.HDL64.azimuth_steps)
    ref_last = [None] * S
    for f in range(2):
        host = [synth.make_cloud(synth.HDL64, seed=70 + s, frame=f) for s in range(S)]
        if f == 1:
            host[1] = np.ascontiguousarray(host[1][:2])
        seeds = [300 + 10 * f + s for s in range(S)]
        clouds = [to(c) for c in host]
        coeffs, masks, status, counts = tb.ransac_planes(clouds, seeds)
        assert coeffs.shape == (S, 4) and coeffs.dtype == np.float32 and counts.shape == (S, 3)
        uv = [synth.make_features_near_points(host[0] if c.shape[0] < 3 else c, NT, seed=80 + 3 * f + s) for s, c in enumerate(host)]
        u0 = [x[:, 0].astype(np.float32) for x in uv]
        v0 = [x[:, 1].astype(np.float32) for x in uv]
        u1 = [(x[:, 0] + rng.normal(0, 3, NT)).astype(np.float32) for x in uv]
        v1 = [(x[:, 1] + rng.normal(0, 2, NT)).astype(np.float32) for x in uv]
        is_new = [(rng.random(NT) < (1.0 if f == 0 else 0.3)) for _ in range(S)]
        d_cur = [torch.empty(NT, dtype=torch.float32, device=dev) for _ in range(S)]
        d_last = [torch.full((NT,), float("nan"), dtype=torch.float32, device=dev) for _ in range(S)]
        t_cur = [torch.empty(NT, dtype=torch.int32, device=dev) for _ in range(S)]
        t_last = [torch.zeros(NT, dtype=torch.int32, device=dev) for _ in range(S)]
        torch.cuda.synchronize()
        tb.run(tb.prepare(clouds, coeffs, masks, [to(a) for a in u0], [to(a) for a in v0], [to(a) for a in u1],
                          [to(a) for a in v1], [to(a.astype(np.uint8)) for a in is_new], d_cur, d_last, t_cur, t_last))
        tb.est.synchronize()
        for s in range(S):
            ref = make_oracle(P)
            ref.set_cloud(host[s])
            if host[s].shape[0] < 3:
                assert status[s] == 1 and not coeffs[s].any() and tuple(counts[s]) == (2, 0, 0)
                ref.set_ground_plane(None, None)
            else:
                c0, inl0 = ref.estimate_ground_plane(seeds[s])
                assert status[s] == 0 and np.array_equal(bits(coeffs[s]), bits(c0))
                assert np.array_equal(masks[s].cpu().numpy().view(np.uint32), mask_of(inl0, host[s].shape[0]))
                assert tuple(counts[s][:2]) == (host[s].shape[0], inl0.size) and counts[s][2] >= 1
            e_cur, e_last, et_cur, et_last = oracle.tracklets_depth(ref, ref_last[s], u0[s], v0[s], u1[s], v1[s], is_new[s],
                                                                    n_threads=8)
            assert_depth_parity(d_cur[s].cpu().numpy(), t_cur[s].cpu().numpy(), e_cur, et_cur, exact_main=False)
            nw = is_new[s]
            assert_depth_parity(d_last[s].cpu().numpy()[nw], t_last[s].cpu().numpy()[nw], e_last[nw], et_last[nw],
                                exact_main=False)
            ref_last[s] = ref
    tb.close()
