"""mld_plane_inliers_export_device (PlaneInliers, TrackletBatch.plane_inliers) against the NumPy restatement
(plane_inliers_restatement.py), against the one-slot getters and behind the two batch estimators: every comparison is of
integers or of raw float bits - the transform is the depth path's, operation for operation, and nothing is summed; there
is no tolerance.

Point counts and what they reach (a mask word takes 32 points, a wavefront's ballot 64, a block 1024):
  1, 31, 32, 33      a word not full / full / a second one
  63, 64, 65         a ballot not full / full / a second one
  1023, 1024, 1025   a second block
  2049, 4999         a third and a fifth block, the last one ending in the middle of a word
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import (CameraPinhole, PlaneInliers, ProjectedClouds, RansacPlanes, SemanticPlanes,
                                  TrackletBatch, capi, synth)

from helpers import kitti_camera, make_estimator
from plane_inliers_restatement import camera_cs, restate, words_of

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049, 4999)
MASKS = ("zero", "ones", "bit0", "last", "half", "sparse", "half_dirty")
GUARD = 0x5A5AA5A5
LEAD, PAD = 2, 4  # guard words before (8-byte alignment kept) and after every array
THR = 2.0

SMALL_CAM = CameraPinhole(64, 64, 64.0, 32.0, 32.0)
SMALL_T = np.eye(4)[:3].copy()  # x_cam = x_lidar, exactly


def params(use=False, thr=THR):
    return capi.params_c0().replace(ransac_plane_use_camx_treshold=1 if use else 0, ransac_plane_treshold_camx=thr)


def random_cloud(n, seed):
    """x_cam = -y_lidar under the KITTI transform: uniform in [-10, 10]."""
    rng = np.random.default_rng(seed)
    cl = np.zeros((n, 4), np.float32)
    cl[:, 0] = rng.uniform(-30, 60, n)
    cl[:, 1] = rng.uniform(-10, 10, n)
    cl[:, 2] = rng.uniform(-3, 3, n)
    cl[:, 3] = rng.uniform(0, 1, n)
    return cl


def make_mask(n, kind, seed=0):
    """The mask words of a cloud of n points."""
    rng = np.random.default_rng(9000 + 31 * n + seed)
    W = (n + 31) // 32
    if kind == "zero":
        return np.zeros(W, np.uint32)
    if kind == "ones":
        return np.full(W, 0xFFFFFFFF, np.uint32)  # (the bits beyond n as well)
    bits = np.zeros(n, bool)
    if kind == "bit0":
        bits[0] = True
    elif kind == "last":
        bits[n - 1] = True
    elif kind in ("half", "half_dirty"):
        bits = rng.random(n) < 0.5
    elif kind == "sparse":
        bits = rng.random(n) < 1.0 / 64
    else:
        raise KeyError(kind)
    words = words_of(bits)
    if kind == "half_dirty" and n & 31:
        words[-1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)
    return words


_CAM = {}


def cam_of(cloud, key, camera=None, T=None):
    """The oracle's camera-frame cloud; computed once per key and left unchanged."""
    if key not in _CAM:
        _CAM[key] = camera_cs(cloud, camera, T)
        _CAM[key].setflags(write=False)
    return _CAM[key]


def size_cloud(n):
    return random_cloud(n, 100 + n)


def want_size(n, kind, use, thr=THR):
    cloud = size_cloud(n)
    return restate(cloud, make_mask(n, kind), use, thr, cam=cam_of(cloud, ("sizes", n)))


@pytest.fixture(scope="module")
def est():
    e = make_estimator(capi.params_c0(), max_frames=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def small_est():
    e = make_estimator(capi.params_c0(), camera=SMALL_CAM, T=SMALL_T, max_frames=1)
    yield e
    e.close()


def device_cloud(cloud, stride, dev, offset=False):
    """The cloud on the device: 16- or 32-byte records, optionally one float behind a 16-byte boundary."""
    import torch
    if cloud is None or cloud.shape[0] == 0:
        return None
    n = cloud.shape[0]
    width = stride // 4
    host = np.full((n, width), np.nan, dtype=np.float32)  # (what lies behind x, y, z must not matter)
    host[:, :3] = cloud[:, :3]
    buf = torch.empty(n * width + 4, dtype=torch.float32, device=dev)
    view = buf[1:1 + n * width] if offset else buf[:n * width]
    view.copy_(torch.from_numpy(host.reshape(-1)).to(dev))
    return view.view(n, width)


def device_mask(words, dev, odd=False):
    """The mask on the device at 0 (mod 8) or, odd, at 4 (mod 8); exactly its words, guard words behind them."""
    import torch
    if words is None or words.size == 0:
        return None
    buf = torch.full((words.size + 3,), GUARD, dtype=torch.int32, device=dev)
    view = buf[1:1 + words.size] if odd else buf[:words.size]
    view.copy_(torch.from_numpy(words.view(np.int32)).to(dev))
    assert view.data_ptr() % 8 == (4 if odd else 0)
    return view


class Guarded:
    """`words` int32 words between guard words, all of them the guard pattern before the call."""

    def __init__(self, words, dev):
        import torch
        self.words = words
        self.buf = torch.full((LEAD + words + PAD,), GUARD, dtype=torch.int32, device=dev)

    def view(self, dtype):
        return self.buf[LEAD:LEAD + self.words].view(dtype)

    def read(self):
        """(payload as int32 words, guards before and after untouched)"""
        whole = self.buf.cpu().numpy()
        ok = bool((whole[:LEAD] == GUARD).all() and (whole[LEAD + self.words:] == GUARD).all())
        return whole[LEAD:LEAD + self.words].copy(), ok


def wanted(flag, s):
    """Is the optional output asked for for sequence s?  flag: False (null table), True, or a list of S booleans."""
    return bool(flag) if isinstance(flag, bool) else bool(flag[s])


def prepare(clouds, masks, caps=None, lidar=True, cam=True, stride=16, offset=False, odd=False):
    """The device buffers of one call: clouds, masks, guarded outputs, the argument list of export().  They are made by
    work on torch's stream, which nothing orders against the context's stream: torch.cuda.synchronize() before issue()."""
    import torch
    dev = torch.device("cuda:0")
    S = len(clouds)
    ns = [0 if c is None else c.shape[0] for c in clouds]
    caps = list(ns) if caps is None else list(caps)
    d_clouds = [device_cloud(c, stride, dev, offset) for c in clouds]
    d_masks = [device_mask(m, dev, odd) if n else None for m, n in zip(masks, ns)]
    counts = torch.full((S, 2), -7, dtype=torch.int64, device=dev)
    g = dict(index=[Guarded(k, dev) for k in caps],
             lidar=[Guarded(3 * k, dev) if wanted(lidar, s) else None for s, k in enumerate(caps)],
             cam=[Guarded(6 * k, dev) if wanted(cam, s) else None for s, k in enumerate(caps)])
    tab = lambda gs, dt, flag: None if flag is False else [x.view(dt) if x is not None else None for x in gs]  # noqa: E731
    args = (d_clouds, d_masks, caps, counts, tab(g["index"], torch.int32, True), tab(g["lidar"], torch.float32, lidar),
            tab(g["cam"], torch.float64, cam))
    return dict(ns=ns, caps=caps, counts=counts, g=g, args=args)


def issue(pi, q):
    """Queues the call on the context's stream.  No synchronisation."""
    pi.export(*q["args"])


def collect(q):
    """Per sequence a dict: the counts, the payload words of every array (None where not asked for), guards untouched."""
    cn = q["counts"].cpu().numpy()
    out = []
    for s in range(len(q["ns"])):
        r = dict(n_inliers=int(cn[s, 0]), n_cloud=int(cn[s, 1]), guards=True)
        for name, gs in q["g"].items():
            r[name] = None
            if gs[s] is not None:
                r[name], ok = gs[s].read()
                r["guards"] = r["guards"] and ok
        out.append(r)
    return out


def run(est, P, clouds, masks, max_points=None, pi=None, **kw):
    import torch
    q = prepare(clouds, masks, **kw)
    own = pi is None
    if own:
        pi = PlaneInliers(est, len(clouds), max_points or max(max(q["ns"]), 1), P)
    torch.cuda.synchronize()  # every buffer of the call is made before the context's stream touches one
    issue(pi, q)
    est.synchronize()
    if own:
        pi.close()
    return collect(q)


def check(got, want, cap, what=""):
    """One sequence against the restatement: counts complete, the first min(count, capacity) entries of every list equal
    - the inlier count for index and lidar, the cloud count for cam -, everything at and beyond them still the guard
    pattern."""
    assert got["guards"], what
    assert (got["n_inliers"], got["n_cloud"]) == (want["n_inliers"], want["n_cloud"]), (what, got["n_inliers"], got["n_cloud"])
    m = min(want["n_inliers"], cap)
    assert got["index"].size == cap
    assert np.array_equal(got["index"][:m], want["index"][:m]), what
    assert (got["index"][m:] == GUARD).all(), what
    if got["lidar"] is not None:
        assert np.array_equal(got["lidar"][:3 * m], want["lidar"][:m].view(np.int32).reshape(-1)), what
        assert (got["lidar"][3 * m:] == GUARD).all(), what
    if got["cam"] is not None:
        k = min(want["n_cloud"], cap)
        assert np.array_equal(got["cam"][:6 * k].view(np.int64), want["cam"][:k].view(np.int64).reshape(-1)), what
        assert (got["cam"][6 * k:] == GUARD).all(), what


def test_the_size_cases_keep_and_reject_inliers():
    """On the restatement alone, no GPU call: every size >= 64 at density 1/2 with the 2.0 filter has at least one inlier
    kept and one rejected, and the sparse masks of the larger sizes are not empty."""
    for n in SIZES:
        w = want_size(n, "half", True)
        if n >= 64:
            assert 0 < w["n_cloud"] < w["n_inliers"] < n, (n, w["n_cloud"], w["n_inliers"])
        assert want_size(n, "ones", False)["n_inliers"] == n == want_size(n, "ones", False)["n_cloud"]
        assert want_size(n, "half_dirty", True)["n_inliers"] == w["n_inliers"]
        if n >= 1023:
            assert want_size(n, "sparse", False)["n_inliers"] > 0


@pytest.mark.parametrize("stride", [16, 32])
@pytest.mark.parametrize("n", SIZES)
def test_single_sequences_equal_the_restatement(est, n, stride):
    """Every mask kind, filter off and on, one sequence per call."""
    cloud = size_cloud(n)
    for use in (False, True):
        pi = PlaneInliers(est, 1, n, params(use))
        for kind in MASKS:
            got = run(est, None, [cloud], [make_mask(n, kind)], pi=pi, stride=stride)[0]
            check(got, want_size(n, kind, use), n, f"n={n} stride={stride} {kind} filter={use}")
        pi.close()


@pytest.mark.parametrize("stride,shifted", [(16, False), (32, False), (16, True), (32, True)])
@pytest.mark.parametrize("use", [False, True])
def test_the_sizes_in_one_ragged_call_equal_the_restatement(est, stride, shifted, use):
    """Every boundary size in ONE call per mask kind; shifted: every cloud at 4 (mod 16), every mask at 4 (mod 8)."""
    clouds = [size_cloud(n) for n in SIZES]
    pi = PlaneInliers(est, len(SIZES), max(SIZES), params(use))
    for kind in MASKS:
        got = run(est, None, clouds, [make_mask(n, kind) for n in SIZES], pi=pi, stride=stride, offset=shifted, odd=shifted)
        for n, g in zip(SIZES, got):
            check(g, want_size(n, kind, use), n, f"ragged n={n} {kind} filter={use}")
    pi.close()


LONG = (65537, 262145, 1)  # 65 chunks: the scan's second wavefront; 257: its second round, the last chunk of one point


@pytest.mark.parametrize("use", [False, True])
def test_long_sequences_whose_chunk_counts_leave_the_first_wavefront_and_the_first_round_of_the_scan(est, use):
    """One call on an object of max_points 262 145: the prefixes over the chunk counts cross from wavefront 0 to wavefront
    1 (65 chunks) and carry into a second round of 256 chunks (257 chunks) - with the filter on, both of them."""
    clouds = [size_cloud(n) for n in LONG]
    got = run(est, params(use), clouds, [make_mask(n, "half") for n in LONG], max_points=262145)
    for n, g in zip(LONG, got):
        want = want_size(n, "half", use)
        if n > 1:
            assert 0 < want["n_cloud"] < n and (want["n_cloud"] < want["n_inliers"]) == use
        check(g, want, n, f"long n={n} filter={use}")


def filter_cloud():
    """Camera = lidar frame (SMALL_T): x_cam is the record's x.  Points at +0.0, -0.0, +-2, just beyond, NaN, inf."""
    xs = [0.0, -0.0, 2.0, -2.0, np.nextafter(np.float32(2.0), np.float32(3.0)), 1.5, -1.5, np.nan, np.inf, -np.inf, 9.0, 1e-30]
    rng = np.random.default_rng(4)
    cl = np.zeros((1100, 4), np.float32)
    cl[:, 0] = rng.uniform(-10, 10, 1100)
    cl[:, 1] = rng.uniform(-5, 5, 1100)
    cl[:, 2] = rng.uniform(1, 30, 1100)
    for k, x in enumerate(xs):  # in the first word, around a wavefront's end and in the second block
        for at in (k, 60 + k, 1030 + k):
            cl[at, 0] = x
    return cl, len(xs)


@pytest.mark.parametrize("use,thr", [(False, 2.0), (True, 2.0), (True, 0.0), (True, -1.0), (True, np.inf)],
                         ids=["off", "2.0", "0.0", "negative", "inf"])
def test_the_filter(small_est, use, thr):
    cloud, k = filter_cloud()
    n = cloud.shape[0]
    cam = cam_of(cloud, "filter", SMALL_CAM, SMALL_T)
    assert np.array_equal(cam[:k, 0], cloud[:k, 0].astype(np.float64), equal_nan=True)  # x_cam is x
    bits = np.random.default_rng(5).random(n) < 0.5
    for at in (0, 60, 1030):
        bits[at:at + k] = True  # the special records are inliers
    words = words_of(bits)
    want = restate(cloud, words, use, thr, cam=cam)
    got = run(small_est, params(use, thr), [cloud], [words])[0]
    check(got, want, n, f"filter {use} {thr}")
    kept = set(want["index"][want["keep"]].tolist())
    nan_at, zeros = 7, {0, 1}
    if not use or thr == np.inf:
        assert (nan_at in kept) == (not use) and {8, 9} <= kept  # NaN: in with the filter off, out with it on; inf <= inf
        assert want["n_cloud"] == want["n_inliers"] - (0 if not use else 3)
    elif thr < 0:
        assert got["n_cloud"] == 0 and got["n_inliers"] == want["n_inliers"] > 0
    elif thr == 0.0:
        assert got["n_cloud"] == 6 and {0, 1, 60, 61, 1030, 1031} == kept  # +0.0 and -0.0, nothing else
    else:
        assert zeros <= kept and {2, 3, 5, 6, 11} <= kept and not ({4, 7, 8, 9, 10} & kept)


CAPACITIES = {"0": lambda c: 0, "1": lambda c: 1, "count - 1": lambda c: c - 1, "count": lambda c: c, "count + 7": lambda c: c + 7}


@pytest.mark.parametrize("of", ["n_inliers", "n_cloud"])
@pytest.mark.parametrize("which", list(CAPACITIES))
def test_capacity(est, which, of):
    """Nothing at or beyond min(count, capacity) changes in any of the three outputs (the arrays are the guard pattern
    before the call, with guard words around them), the counts are complete; ONE capacity bounds index and lidar by the
    inlier rank and cam by the cloud rank, so with the filter on the lists end at different lengths."""
    ns, kinds = (4999, 65, 1025, 0), ("half", "ones", "sparse", "zero")
    clouds = [size_cloud(n) if n else None for n in ns]
    masks = [make_mask(n, k) if n else None for n, k in zip(ns, kinds)]
    wants = [want_size(n, k, True) if n else restate(np.empty((0, 4), np.float32), np.empty(0, np.uint32), True, THR) for n, k in zip(ns, kinds)]
    assert wants[0]["n_cloud"] < wants[0]["n_inliers"] - 7
    caps = [max(0, CAPACITIES[which](w[of])) for w in wants]
    got = run(est, params(True), clouds, masks, caps=caps, max_points=5000)
    for n, w, k, g in zip(ns, wants, caps, got):
        check(g, w, k, f"capacity {which} of {of} n={n}")
    if which in ("0", "1"):
        assert got[0]["n_inliers"] > caps[0] and got[0]["n_cloud"] > caps[0]  # truncated, and told so


@pytest.mark.parametrize("null_table", ["lidar", "cam", "neither"])
def test_optional_outputs_as_a_null_table_and_as_single_null_entries(est, null_table):
    """One ragged call: one of the two optional outputs is a null table, the other has null entries; a sequence without
    points sits in the middle with null arrays."""
    ns = (1025, 65, 0, 4999)
    clouds = [size_cloud(n) if n else None for n in ns]
    masks = [make_mask(n, "half") if n else None for n in ns]
    kw = dict(lidar=[True, False, False, True], cam=[False, True, False, True])
    if null_table != "neither":
        kw[null_table] = False
    got = run(est, params(True), clouds, masks, max_points=5000, **kw)
    for s, (n, g) in enumerate(zip(ns, got)):
        want = want_size(n, "half", True) if n else dict(n_inliers=0, n_cloud=0, index=np.empty(0, np.int32))
        check(g, want, n, f"optional {null_table} [{s}]")
        for name, flag in kw.items():
            assert (g[name] is not None) == wanted(flag, s)


def test_sequences_without_points_need_no_arrays(est):
    """n[s] == 0 with null cloud, mask and outputs inside a ragged call, and a call in which every sequence is empty."""
    got = run(est, params(True), [None, size_cloud(65), None], [None, make_mask(65, "ones"), None], max_points=100)
    assert [(g["n_inliers"], g["n_cloud"]) for g in got][::2] == [(0, 0), (0, 0)] and all(g["guards"] for g in got)
    check(got[1], want_size(65, "ones", True), 65, "between two empty sequences")
    got = run(est, params(False), [None, None], [None, None], max_points=100)
    assert [(g["n_inliers"], g["n_cloud"]) for g in got] == [(0, 0), (0, 0)]


def test_export_past_the_last_generation_of_the_descriptor_ring(est):
    """35 calls with different ragged tables and different masks are queued without a synchronisation in between (the
    ring has 16 generations); every call's outputs are checked afterwards."""
    import torch
    S, calls = 3, 35
    sizes = (0, 1, 33, 64, 65, 1023, 1025, 2049)
    pi = PlaneInliers(est, S, max(sizes), params(True))
    queued = []
    for k in range(calls):  # the buffers of ALL calls first ...
        ns = [sizes[(k + 3 * s) % len(sizes)] for s in range(S)]
        masks = [make_mask(n, ("half", "sparse", "ones")[(k + s) % 3], seed=k) if n else None for s, n in enumerate(ns)]
        caps = [n if (k + s) % 3 else n // 4 for s, n in enumerate(ns)]
        queued.append((ns, masks, caps, prepare([size_cloud(n) if n else None for n in ns], masks, caps=caps)))
    torch.cuda.synchronize()
    for *_, q in queued:  # ... then the calls back to back
        issue(pi, q)
    est.synchronize()
    pi.close()
    some = 0
    for k, (ns, masks, caps, q) in enumerate(queued):
        for s, g in enumerate(collect(q)):
            if ns[s] == 0:
                assert (g["n_inliers"], g["n_cloud"], g["guards"]) == (0, 0, True)
                continue
            cloud = size_cloud(ns[s])
            want = restate(cloud, masks[s], True, THR, cam=cam_of(cloud, ("sizes", ns[s])))
            check(g, want, caps[s], f"call {k} [{s}]")
            some += want["n_cloud"]
    assert some > 0


def test_equal_to_the_one_slot_getters():
    """A VLP16 and an HDL64 frame with the analytic ground plane on two slots of a context with the camx filter on:
    mld_set_clouds_planes_device, then mld_get_ground_plane_inliers / mld_get_ground_plane_cloud per slot, against ONE
    batched call and against the cam_out of ProjectedClouds gathered at the indices."""
    import torch
    dev = torch.device("cuda:0")
    P = params(True, 6.0)
    e = make_estimator(P, max_frames=2)
    hosts = [synth.make_cloud(synth.VLP16, seed=51, frame=1), synth.make_cloud(synth.HDL64_KITTI, seed=52, frame=1)]
    planes = [synth.make_ground_plane(c) for c in hosts]
    words = []
    for c, (_, inl) in zip(hosts, planes):
        bits = np.zeros(c.shape[0], bool)
        bits[inl] = True
        words.append(words_of(bits))
    got = run(e, P, hosts, words)
    d_clouds = [torch.from_numpy(c).to(dev) for c in hosts]
    d_masks = [torch.from_numpy(w.view(np.int32)).to(dev) for w in words]
    ns = [c.shape[0] for c in hosts]
    cams = [torch.empty((n, 3), dtype=torch.float64, device=dev) for n in ns]
    nvis = torch.empty(2, dtype=torch.int64, device=dev)
    pc = ProjectedClouds(e, 2, max(ns))
    torch.cuda.synchronize()
    pc.export(d_clouds, [0, 0], nvis, [None, None], [None, None], cam=cams)
    coeffs = np.ascontiguousarray(np.stack([p[0] for p in planes]), dtype=np.float32)
    e._check(e._lib.mld_set_clouds_planes_device(
        e._ctx, 2, (C.c_void_p * 2)(*[int(c.data_ptr()) for c in d_clouds]), (C.c_int64 * 2)(*ns), 16,
        coeffs.ctypes.data_as(C.POINTER(C.c_float)), (C.c_void_p * 2)(*[int(m.data_ptr()) for m in d_masks])))
    for s in range(2):
        inl = e.getGroundPlaneInliers(s)
        cloud = np.ascontiguousarray(e.getCloudRansacPlane(s).T)
        g = got[s]
        assert g["guards"] and g["n_inliers"] == inl.size == planes[s][1].size > 100
        assert 0 < g["n_cloud"] == cloud.shape[0] < g["n_inliers"]
        assert np.array_equal(g["index"][:inl.size], inl)
        assert np.array_equal(g["lidar"][:3 * inl.size], hosts[s][inl, :3].view(np.int32).reshape(-1))
        assert np.array_equal(g["cam"][:6 * cloud.shape[0]].view(np.int64), cloud.view(np.int64).reshape(-1))
        all_cam = cams[s].cpu().numpy()[inl]
        keep = np.abs(all_cam[:, 0]) <= 6.0
        assert np.array_equal(all_cam[keep].view(np.int64), cloud.view(np.int64))
    pc.close()
    e.close()


def test_behind_the_ransac_planes_without_a_host_round_trip():
    """RansacPlanes.estimate, then PlaneInliers.export on its masks, both queued before anything is read: n_inliers equals
    the record's, the indices equal mld_get_ground_plane_inliers after the one-slot estimation with the same seed, and a
    failed sequence (two points: status 1, a mask of zeros) gets counts 0 while the others are unaffected."""
    import torch
    dev = torch.device("cuda:0")
    P = params(True, 6.0)
    e = make_estimator(P, max_frames=1)
    hosts = [synth.make_cloud(synth.VLP16, seed=61, frame=1), random_cloud(2, 1), synth.make_cloud(synth.VLP16, seed=62, frame=2)]
    seeds = [11, 12, 13]
    S, ns = 3, [c.shape[0] for c in hosts]
    d_clouds = [torch.from_numpy(c).to(dev) for c in hosts]
    d_masks = [torch.full((RansacPlanes.mask_words(n) + 1,), GUARD, dtype=torch.int32, device=dev) for n in ns]
    res = torch.empty((S, 8), dtype=torch.int32, device=dev)
    q = prepare(hosts, [np.zeros((n + 31) // 32, np.uint32) for n in ns])
    args = list(q["args"])
    args[0], args[1] = d_clouds, d_masks
    rp, pi = RansacPlanes(e, S, max(ns), P), PlaneInliers(e, S, max(ns), P)
    torch.cuda.synchronize()
    rp.estimate(d_clouds, seeds, res, d_masks)
    pi.export(*args)
    e.synchronize()
    rec, got = res.cpu().numpy(), collect(q)
    assert rec[:, 6].tolist() == [0, 1, 0]  # status
    assert (got[1]["n_inliers"], got[1]["n_cloud"], got[1]["guards"]) == (0, 0, True) and (got[1]["index"] == GUARD).all()
    for s in (0, 2):
        e.setInputCloud(d_clouds[s], None, plane_given=False)
        _, n_one = e.estimateGroundPlane(0, seeds[s])
        inl = e.getGroundPlaneInliers()
        cloud = np.ascontiguousarray(e.getCloudRansacPlane().T)
        g = got[s]
        assert g["guards"] and g["n_inliers"] == rec[s, 4] == n_one == inl.size > 3
        assert np.array_equal(g["index"][:n_one], inl) and (g["index"][n_one:] == GUARD).all()
        assert g["n_cloud"] == cloud.shape[0] > 0
        assert np.array_equal(g["cam"][:6 * g["n_cloud"]].view(np.int64), cloud.view(np.int64).reshape(-1))
    rp.close()
    pi.close()
    e.close()


def test_behind_the_semantic_planes_without_a_host_round_trip():
    """SemanticPlanes.estimate, then PlaneInliers.export on its masks, likewise; the failed sequence has two points."""
    import torch
    dev = torch.device("cuda:0")
    P = params(False)
    e = make_estimator(P, max_frames=1)
    frames = [synth.make_cloud(synth.VLP16, seed=3, frame=1), synth.make_cloud(synth.VLP16, seed=4, frame=1)]
    imgs = [synth.make_label_image(c) for c in frames]
    hosts, imgs = [frames[0], np.ascontiguousarray(frames[1][:2]), frames[1]], [imgs[0], imgs[1], imgs[1]]
    S, ns, labels, thr = 3, [c.shape[0] for c in hosts], (6, 7, 8, 9), 0.1
    d_clouds = [torch.from_numpy(c).to(dev) for c in hosts]
    d_imgs = [torch.from_numpy(i).to(dev) for i in imgs]
    d_masks = [torch.full((SemanticPlanes.mask_words(n) + 1,), GUARD, dtype=torch.int32, device=dev) for n in ns]
    res = torch.empty((S, 8), dtype=torch.int32, device=dev)
    q = prepare(hosts, [np.zeros((n + 31) // 32, np.uint32) for n in ns])
    args = list(q["args"])
    args[0], args[1] = d_clouds, d_masks
    sp, pi = SemanticPlanes(e, S, max(ns)), PlaneInliers(e, S, max(ns), P)
    torch.cuda.synchronize()
    sp.estimate(d_clouds, d_imgs, labels, thr, res, d_masks)
    pi.export(*args)
    e.synchronize()
    rec, got = res.cpu().numpy(), collect(q)
    assert rec[:, 6].tolist() == [0, 1, 0]  # status
    assert (got[1]["n_inliers"], got[1]["n_cloud"], got[1]["guards"]) == (0, 0, True) and (got[1]["index"] == GUARD).all()
    for s in (0, 2):
        e.setInputCloud(d_clouds[s], None, plane_given=False)
        _, n_one = e.estimateSemanticPlane(d_imgs[s], labels, thr)
        inl = e.getGroundPlaneInliers()
        g = got[s]
        assert g["guards"] and g["n_inliers"] == g["n_cloud"] == rec[s, 5] == n_one == inl.size > 3
        assert np.array_equal(g["index"][:n_one], inl) and (g["index"][n_one:] == GUARD).all()
        assert np.array_equal(g["lidar"][:3 * n_one], hosts[s][inl, :3].view(np.int32).reshape(-1))
    sp.close()
    pi.close()
    e.close()


def test_tracklet_batch_plane_inliers_on_three_ragged_sequences():
    """The Python route, with the masks as ransac_planes() returns them: device tensors out."""
    import torch
    dev = torch.device("cuda:0")
    P = params(True, 6.0)
    hosts = [synth.make_cloud(synth.VLP16, seed=71, frame=1), np.ascontiguousarray(synth.make_cloud(synth.VLP16, seed=72, frame=1)[:7001]),
             random_cloud(2, 3)]
    tb = TrackletBatch(P, kitti_camera(), synth.T_CAM_LIDAR, 3, 16)
    with pytest.raises(Exception, match="attach_plane_inliers"):
        tb.plane_inliers([None] * 3, [None] * 3)
    tb.attach_ransac_planes(30000)
    assert tb.attach_plane_inliers(30000) is tb.attach_plane_inliers()
    clouds = [torch.from_numpy(c).to(dev) for c in hosts]
    coeffs, masks, status, counts = tb.ransac_planes(clouds, [21, 22, 23])
    assert status.tolist() == [0, 0, 1]
    out = tb.plane_inliers(clouds, masks, lidar=True, cam=True)
    cn = out["counts"].cpu().numpy()
    assert tuple(cn.shape) == (3, 2) and cn[:, 0].tolist() == counts[:, 1].tolist() and cn[2].tolist() == [0, 0]
    for s, c in enumerate(hosts):
        n = c.shape[0]
        want = restate(c, masks[s].cpu().numpy().view(np.uint32)[:(n + 31) // 32], True, 6.0)
        k, m = want["n_inliers"], want["n_cloud"]
        assert (k, m) == tuple(cn[s]) and tuple(out["index"][s].shape) == (n,) and tuple(out["cam"][s].shape) == (n, 3)
        assert np.array_equal(out["index"][s][:k].cpu().numpy(), want["index"])
        assert np.array_equal(out["lidar"][s][:k].cpu().numpy().view(np.int32), want["lidar"].view(np.int32))
        assert np.array_equal(out["cam"][s][:m].cpu().numpy().view(np.int64), want["cam"].view(np.int64))
    assert 0 < cn[0, 1] < cn[0, 0]
    few = tb.plane_inliers(clouds, masks, capacity=[10, 0, 1000])
    assert few["lidar"] is None and few["cam"] is None and np.array_equal(few["counts"].cpu().numpy(), cn)
    assert tuple(few["index"][0].shape) == (10,) and tuple(few["index"][1].shape) == (0,) and tuple(few["index"][2].shape) == (2,)
    assert np.array_equal(few["index"][0].cpu().numpy(), restate(hosts[0], masks[0].cpu().numpy().view(np.uint32), False)["index"][:10])
    tb.close()


def test_arguments_are_refused_by_name(est):
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    st = C.c_int(0)
    P = params(True)
    T = np.ascontiguousarray(np.asarray(synth.T_CAM_LIDAR, dtype=np.float64).reshape(-1)[:12])
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    assert not lib.mld_plane_inliers_create(est._ctx, 2, 100, None, Tp, C.byref(st)) and st.value == capi.MLD_ERR_INVALID_ARG
    assert "params" in lib.mld_plane_inliers_last_error(None).decode()
    assert not lib.mld_plane_inliers_create(est._ctx, 2, 100, C.byref(P), None, C.byref(st)) and st.value == capi.MLD_ERR_INVALID_ARG
    assert "T_cam_lidar" in lib.mld_plane_inliers_last_error(None).decode()
    pi = lib.mld_plane_inliers_create(est._ctx, 2, 100, C.byref(P), Tp, C.byref(st))
    assert pi and st.value == capi.MLD_OK
    cloud = torch.zeros((101, 4), dtype=torch.float32, device=dev)
    mask = torch.zeros(8, dtype=torch.int32, device=dev)
    index = torch.full((100 + PAD,), GUARD, dtype=torch.int32, device=dev)
    lidar = torch.full((300 + PAD,), GUARD, dtype=torch.int32, device=dev)
    cam = torch.full((600 + PAD,), GUARD, dtype=torch.int32, device=dev)
    counts = torch.full((2, 2), -7, dtype=torch.int64, device=dev)
    tab = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())  # noqa: E731
    half = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)  # noqa: E731
    odd = lambda t, by=2: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr() + by)  # noqa: E731
    i64 = lambda a, b: (C.c_int64 * 2)(a, b)  # noqa: E731
    good = dict(pts=tab(cloud), n=i64(100, 100), stride=16, mask=tab(mask), cap=i64(100, 100), counts=counts.data_ptr(),
                index=tab(index), lidar=tab(lidar), cam=tab(cam))

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.mld_plane_inliers_export_device(pi, a["pts"], a["n"], a["stride"], a["mask"], a["cap"], a["counts"], a["index"],
                                                 a["lidar"], a["cam"])
        return rc, lib.mld_plane_inliers_last_error(pi).decode()

    torch.cuda.synchronize()
    for kw, word in ((dict(pts=None), "null table pts_dev"), (dict(n=None), "null table n"), (dict(mask=None), "null table mask_dev"),
                     (dict(cap=None), "null table capacity"), (dict(index=None), "null table index_out"),
                     (dict(counts=None), "null array counts_out_dev"), (dict(pts=half(cloud)), "null array pts_dev"),
                     (dict(mask=half(mask)), "null array mask_dev"), (dict(index=half(index)), "null array index_out"),
                     (dict(n=i64(100, -1)), "negative n"), (dict(cap=i64(100, -1)), "negative capacity"),
                     (dict(stride=12), "stride_bytes"), (dict(stride=64), "stride_bytes"),
                     (dict(pts=odd(cloud)), "pts_dev must be 4-byte aligned"), (dict(mask=odd(mask)), "mask_dev must be 4-byte aligned"),
                     (dict(index=odd(index)), "index_out must be 4-byte aligned"),
                     (dict(lidar=odd(lidar)), "lidar_out must be 4-byte aligned"),
                     (dict(cam=odd(cam, 4)), "cam_out must be 8-byte aligned"),
                     (dict(counts=counts.data_ptr() + 4), "counts_out_dev must be 8-byte aligned")):
        rc, text = call(**kw)
        assert rc == capi.MLD_ERR_INVALID_ARG and word in text and "mld_plane_inliers_export_device" in text, (kw, text)
    assert lib.mld_plane_inliers_export_device(None, *[good[k] for k in ("pts", "n", "stride", "mask", "cap", "counts", "index",
                                                                         "lidar", "cam")]) == capi.MLD_ERR_INVALID_ARG
    assert "null object (pi)" in lib.mld_plane_inliers_last_error(None).decode()
    rc, text = call(n=i64(100, 101))
    assert rc == capi.MLD_ERR_CAPACITY and "max_points" in text
    est.synchronize()
    for t in (index, lidar, cam):
        assert (t.cpu().numpy() == GUARD).all()
    assert (counts.cpu().numpy() == -7).all()
    # a sequence without points, and one without capacity, need no arrays; a mask of zeros has no inlier
    for kw in (dict(n=i64(100, 0), pts=half(cloud), mask=half(mask), index=half(index), lidar=half(lidar), cam=half(cam)),
               dict(cap=i64(100, 0), index=half(index), lidar=None, cam=None)):
        rc, text = call(**kw)
        assert rc == capi.MLD_OK, text
        est.synchronize()
        assert counts.cpu().numpy().tolist() == [[0, 0], [0, 0]]
    for t in (index, lidar, cam):
        assert (t.cpu().numpy() == GUARD).all()
    lib.mld_plane_inliers_destroy(pi)
