"""mld_projected_clouds_export_device (ProjectedClouds, TrackletBatch.projected_clouds) against the oracle's
PointcloudData and against the one-slot getters: every comparison is for EQUALITY, f64 values as raw bits - transform and
projection are the depth path's, operation for operation, and nothing is summed; there is no tolerance.

Point counts and what they reach (a wavefront takes 64 points, a block 1024):
  0                  no arrays, n_visible 0, a map of -1
  1, 63, 64, 65      one mask word not full / full / a second one
  1023, 1024, 1025   a second block
  4097               a fifth block
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import NO_PLANE, CameraPinhole, ProjectedClouds, TrackletBatch, capi, synth

from helpers import kitti_camera, make_estimator, make_oracle

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097)
GUARD = 0x5A5AA5A5
LEAD, PAD = 2, 4  # guard words before (8-byte alignment kept) and after every array

SMALL_CAM = CameraPinhole(64, 64, 64.0, 32.0, 32.0)  # powers of two: the projections below are exact
SMALL_T = np.eye(4)[:3].copy()


def random_cloud(n, seed):
    """Points in front of, beside and behind the scanner (lidar frame: x forward): some project into the image, some
    beside it, and some of those behind the camera project into it as well."""
    rng = np.random.default_rng(seed)
    cl = np.zeros((n, 4), np.float32)
    cl[:, 0] = rng.uniform(-30, 60, n)
    cl[:, 1] = rng.uniform(-25, 25, n)
    cl[:, 2] = rng.uniform(-3, 3, n)
    cl[:, 3] = rng.uniform(0, 1, n)
    return cl


_WANT = {}


def expected(cloud, camera=None, T=None, key=None):
    """{nvis, uv [Nvis, 2], index, cam [n, 3], map [H, W]} from the oracle; computed once per key and left unchanged."""
    if key is not None and key in _WANT:
        return _WANT[key]
    cam = camera or kitti_camera()
    n = cloud.shape[0]
    if n == 0:
        want = dict(nvis=0, uv=np.empty((0, 2)), index=np.empty(0, np.int32), cam=np.empty((0, 3)),
                    map=np.full((cam.height, cam.width), -1, np.int32))
    else:
        ref = make_oracle(capi.params_c0(), camera, T)
        ref.set_cloud(cloud)
        want = dict(nvis=ref.nvis, uv=np.ascontiguousarray(ref.visible_image_points().T), index=ref.point_index().copy(),
                    cam=np.ascontiguousarray(ref.cloud_camera_cs().T), map=ref.pixel_map().copy())
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if key is not None:
        _WANT[key] = want
    return want


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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
    n = cloud.shape[0]
    if n == 0:
        return None
    width = stride // 4
    host = np.full((n, width), np.nan, dtype=np.float32)  # (what lies behind x, y, z must not matter)
    host[:, :3] = cloud[:, :3]
    buf = torch.empty(n * width + 4, dtype=torch.float32, device=dev)
    view = buf[1:1 + n * width] if offset else buf[:n * width]
    view.copy_(torch.from_numpy(host.reshape(-1)).to(dev))
    return view.view(n, width)


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


def prepare(cam, clouds, caps=None, depth=True, cam_out=True, pixel_map=True, stride=16, offset=False):
    """The device buffers of one call: clouds, guarded outputs, the argument list of export().  They are made by work on
    torch's stream, which nothing orders against the context's stream: torch.cuda.synchronize() before issue()."""
    import torch
    dev = torch.device("cuda:0")
    S = len(clouds)
    ns = [c.shape[0] for c in clouds]
    caps = list(ns) if caps is None else list(caps)
    d_clouds = [device_cloud(c, stride, dev, offset) for c in clouds]
    nvis = torch.full((S,), -7, dtype=torch.int64, device=dev)
    cells = cam.width * cam.height
    g = dict(uv=[Guarded(4 * k, dev) for k in caps], index=[Guarded(k, dev) for k in caps],
             depth=[Guarded(2 * k, dev) if wanted(depth, s) else None for s, k in enumerate(caps)],
             cam=[Guarded(6 * n, dev) if wanted(cam_out, s) else None for s, n in enumerate(ns)],
             map=[Guarded(cells, dev) if wanted(pixel_map, s) else None for s in range(S)])
    tab = lambda gs, dt, flag: None if flag is False else [x.view(dt) if x is not None else None for x in gs]  # noqa: E731
    args = (d_clouds, caps, nvis, tab(g["uv"], torch.float64, True), tab(g["index"], torch.int32, True),
            tab(g["depth"], torch.float64, depth), tab(g["cam"], torch.float64, cam_out), tab(g["map"], torch.int32, pixel_map))
    return dict(ns=ns, caps=caps, nvis=nvis, g=g, args=args)


def issue(pc, q):
    """Queues the call on the context's stream.  No synchronisation."""
    pc.export(*q["args"])


def collect(q):
    """Per sequence a dict: nvis, the payload words of every array (None where not asked for), guards untouched."""
    nv = q["nvis"].cpu().numpy()
    out = []
    for s in range(len(q["ns"])):
        r = dict(nvis=int(nv[s]), guards=True)
        for name, gs in q["g"].items():
            r[name] = None
            if gs[s] is not None:
                r[name], ok = gs[s].read()
                r["guards"] = r["guards"] and ok
        out.append(r)
    return out


def run(est, cam, clouds, max_points=None, **kw):
    import torch
    q = prepare(cam, clouds, **kw)
    pc = ProjectedClouds(est, len(clouds), max_points or max(max(c.shape[0] for c in clouds), 1))
    torch.cuda.synchronize()  # every buffer of the call is made before the context's stream touches one
    issue(pc, q)
    est.synchronize()
    pc.close()
    return collect(q)


def check(got, want, n, cap, what="", want_map=None):
    """One sequence against the oracle's record: the first min(Nvis, capacity) entries equal, everything at and beyond
    them still the guard pattern, the count complete, cam and map whole."""
    assert got["guards"], what
    nvis = want["nvis"]
    assert got["nvis"] == nvis, (what, got["nvis"], nvis)
    m = min(nvis, cap)
    uv = got["uv"]
    assert uv.size == 4 * cap
    assert np.array_equal(uv[:4 * m].view(np.uint64), bits(want["uv"][:m]).reshape(-1)), what
    assert (uv[4 * m:] == GUARD).all(), what
    assert np.array_equal(got["index"][:m], want["index"][:m]), what
    assert (got["index"][m:] == GUARD).all(), what
    if got["depth"] is not None:
        assert np.array_equal(got["depth"][:2 * m].view(np.uint64), bits(want["cam"][want["index"][:m], 2])), what
        assert (got["depth"][2 * m:] == GUARD).all(), what
    if got["cam"] is not None:
        assert np.array_equal(got["cam"].view(np.uint64), bits(want["cam"]).reshape(-1)), what
    if got["map"] is not None:
        assert np.array_equal(got["map"].reshape(want["map"].shape), want["map"] if want_map is None else want_map), what


def size_clouds():
    return [random_cloud(n, 100 + n) for n in SIZES]


def test_the_size_cases_have_visible_and_invisible_points():
    """On the CPU, through the oracle: neither none nor all of the points of a case are visible, and some visible points
    lie behind the camera (they are in the lists and not in the map)."""
    behind = 0
    for n, c in zip(SIZES, size_clouds()):
        want = expected(c, key=("sizes", n))
        if n >= 63:
            assert 0 < want["nvis"] < n, (n, want["nvis"])
        behind += int((want["cam"][want["index"], 2] < 0).sum())
    assert behind > 0


@pytest.mark.parametrize("stride", [16, 32])
@pytest.mark.parametrize("n", SIZES)
def test_single_sequences_equal_the_oracle(est, n, stride):
    cloud = random_cloud(n, 100 + n)
    got = run(est, kitti_camera(), [cloud], stride=stride)[0]
    check(got, expected(cloud, key=("sizes", n)), n, n, f"n={n} stride={stride}")


@pytest.mark.parametrize("stride,offset", [(16, False), (32, False), (16, True), (32, True)])
def test_the_sizes_in_one_ragged_call_equal_the_oracle(est, stride, offset):
    """Every boundary size in ONE call, stride 16 and 32, cloud bases at 0 and at 4 (mod 16)."""
    clouds = size_clouds()
    got = run(est, kitti_camera(), clouds, stride=stride, offset=offset)
    for n, c, g in zip(SIZES, clouds, got):
        check(g, expected(c, key=("sizes", n)), n, n, f"ragged n={n}")


LONG = (65537, 262145, 1)  # 65 chunks: the scan's second wavefront; 257: its second round, the last chunk of one point


def test_long_sequences_whose_chunk_counts_leave_the_first_wavefront_and_the_first_round_of_the_scan(est):
    """One call on an object of max_points 262 145: the prefix over the chunk counts crosses from wavefront 0 to
    wavefront 1 (65 chunks) and carries into a second round of 256 chunks (257 chunks)."""
    clouds = [random_cloud(n, 100 + n) for n in LONG]
    got = run(est, kitti_camera(), clouds, max_points=262145)
    for n, c, g in zip(LONG, clouds, got):
        want = expected(c, key=("sizes", n))
        assert n == 1 or 0 < want["nvis"] < n
        check(g, want, n, n, f"long n={n}")


def boundary_cloud():
    """Camera 64 x 64, f = 64, cu = cv = 32, identity transform: u = 64 x / z + 32, v = 64 y / z + 32, exactly."""
    nan, inf = np.nan, np.inf
    pts = [(0.0, 0.0, 2.0, True),      # (32, 32)
           (-1.0, 0.0, 2.0, False),    # u == 0
           (1.0, 0.0, 2.0, False),     # u == W
           (0.0, -1.0, 2.0, False),    # v == 0
           (0.0, 1.0, 2.0, False),     # v == H
           (0.5, 0.25, 2.0, True),     # (48, 40)
           (0.1, 0.1, 0.0, False),     # z == 0
           (0.0, 0.0, 0.0, False),     # 0 / 0
           (0.125, 0.125, -2.0, True),  # behind the camera, (28, 28): visible, absent from the map
           (nan, 0.0, 2.0, False), (0.0, nan, 2.0, False), (0.0, 0.0, nan, False),
           (inf, 0.0, 2.0, False), (0.0, -inf, 2.0, False), (0.0, 0.0, inf, False), (0.0, 0.0, -inf, False),
           (-0.96875, 0.0, 2.0, True),  # u == 1
           (0.96875, 0.0, 2.0, True),   # u == 63
           (-1.03125, 0.0, 2.0, False),  # u == -1
           (0.0, 1.03125, 2.0, False)]  # v == 65
    cl = np.zeros((len(pts), 4), np.float32)
    cl[:, :3] = [p[:3] for p in pts]
    return cl, np.array([p[3] for p in pts])


def test_the_boundaries_of_the_image(small_est):
    cloud, vis = boundary_cloud()
    want = expected(cloud, SMALL_CAM, SMALL_T)
    assert np.array_equal(want["index"], np.flatnonzero(vis))  # the oracle agrees with the list above
    got = run(small_est, SMALL_CAM, [cloud])[0]
    check(got, want, cloud.shape[0], cloud.shape[0], "boundaries")
    idx = got["index"][:got["nvis"]]
    assert np.array_equal(idx, np.flatnonzero(vis))
    uv = got["uv"][:4 * got["nvis"]].view(np.float64).reshape(-1, 2)
    assert uv[0].tolist() == [32.0, 32.0] and uv[1].tolist() == [48.0, 40.0] and uv[2].tolist() == [28.0, 28.0]
    m = got["map"].reshape(64, 64)
    behind = int(np.flatnonzero(idx == 8)[0])
    assert m[28, 28] == -1 and behind not in m  # visible, z < 0: in no cell
    assert m[32, 32] == 0 and m[40, 48] == 1 and m[32, 1] == int(np.flatnonzero(idx == 16)[0])
    assert (m >= 0).sum() == vis.sum() - 1


def test_the_first_point_of_a_cell_wins_across_blocks(small_est):
    """Points 5, 70, 1030 and 3000 (four blocks, two words of the first) share the cell (10, 10), all with z > 0: the map
    holds the visible index of point 5.  The first point of the cell (20, 20), 100, has z < 0 and a later one, 2000,
    z > 0: the later one wins."""
    rng = np.random.default_rng(5)
    n = 3100
    cl = np.zeros((n, 4), np.float32)
    z = rng.uniform(1, 4, n)
    u, v = rng.uniform(30, 70, n), rng.uniform(30, 70, n)  # cells right of / below (30, 30), some beside the image
    cl[:, 0], cl[:, 1], cl[:, 2] = (u - 32) * z / 64, (v - 32) * z / 64, z
    for i, frac in ((5, 0.5), (70, 0.25), (1030, 0.75), (3000, 0.125)):
        cl[i, :3] = ((10 + frac - 32) * 2 / 64, (10.5 - 32) * 2 / 64, 2.0)
    cl[100, :3] = ((20.5 - 32) * -2 / 64, (20.5 - 32) * -2 / 64, -2.0)
    cl[2000, :3] = ((20.5 - 32) * 2 / 64, (20.5 - 32) * 2 / 64, 2.0)
    want = expected(cl, SMALL_CAM, SMALL_T)
    assert 0 < want["nvis"] < n
    got = run(small_est, SMALL_CAM, [cl])[0]
    check(got, want, n, n, "first wins")
    m, idx = got["map"].reshape(64, 64), got["index"]
    assert idx[m[10, 10]] == 5 and idx[m[20, 20]] == 2000
    assert {5, 70, 100, 1030, 2000, 3000} <= set(idx[:got["nvis"]].tolist())


CAPACITIES = {"0": lambda nvis: 0, "1": lambda nvis: 1, "nvis - 1": lambda nvis: nvis - 1, "nvis": lambda nvis: nvis,
              "nvis + 3": lambda nvis: nvis + 3}


@pytest.mark.parametrize("which", list(CAPACITIES))
def test_capacity(est, which):
    """Nothing at or beyond min(Nvis, capacity) changes (the arrays are the guard pattern before the call, with guard
    words around them), n_visible is complete, the map is the untruncated one."""
    clouds = [random_cloud(4097, 100 + 4097), random_cloud(65, 100 + 65), random_cloud(0, 100)]
    wants = [expected(c, key=("sizes", c.shape[0])) for c in clouds]
    caps = [max(0, CAPACITIES[which](w["nvis"])) for w in wants]
    got = run(est, kitti_camera(), clouds, caps=caps)
    for c, w, k, g in zip(clouds, wants, caps, got):
        check(g, w, c.shape[0], k, f"capacity {which} n={c.shape[0]}")
        assert g["nvis"] == w["nvis"]
    if which in ("0", "1"):
        assert got[0]["nvis"] > caps[0] and got[0]["map"].max() > caps[0]  # truncated: the map keeps the complete ranks


@pytest.mark.parametrize("null_table", ["depth", "cam_out", "pixel_map"])
def test_optional_outputs_as_a_null_table_and_as_single_null_entries(est, null_table):
    """One ragged call: one of the three optional outputs is a null table, the other two have null entries."""
    clouds = [random_cloud(n, 100 + n) for n in (1025, 65, 0, 4097)]
    kw = dict(depth=[True, False, True, False], cam_out=[False, True, True, False], pixel_map=[True, False, False, True])
    kw[null_table] = False
    got = run(est, kitti_camera(), clouds, **kw)
    name = dict(depth="depth", cam_out="cam", pixel_map="map")
    for s, (c, g) in enumerate(zip(clouds, got)):
        n = c.shape[0]
        check(g, expected(c, key=("sizes", n)), n, n, f"optional {null_table} [{s}]")
        for k, flag in kw.items():
            assert (g[name[k]] is not None) == wanted(flag, s)


@pytest.mark.parametrize("scanner", ["VLP16", "HDL64_KITTI"])
def test_equal_to_the_one_slot_getters(scanner):
    """mld_set_cloud_device on a slot, then the debug getters, against the batched call on the same cloud."""
    import torch
    dev = torch.device("cuda:0")
    e = make_estimator(capi.params_c0(), max_frames=1)
    cloud = synth.make_cloud(getattr(synth, scanner), seed=41, frame=1)
    n = cloud.shape[0]
    got = run(e, kitti_camera(), [cloud])[0]
    e.setInputCloud(torch.from_numpy(cloud).to(dev), NO_PLANE)
    nvis = e.getVisibleCount()
    assert got["guards"] and got["nvis"] == nvis and 0 < nvis < n
    uv = np.ascontiguousarray(e.getPointsCloudImageCs().T)
    idx = e.getPointIndex()
    cam = np.ascontiguousarray(e.getCloudCameraCs(n).T)
    assert np.array_equal(got["uv"][:4 * nvis].view(np.uint64), bits(uv).reshape(-1))
    assert np.array_equal(got["index"][:nvis], idx)
    assert np.array_equal(got["cam"].view(np.uint64), bits(cam).reshape(-1))
    assert np.array_equal(got["map"].reshape(synth.KITTI_H, synth.KITTI_W), e.getPixelMap())
    assert np.array_equal(got["depth"][:2 * nvis].view(np.uint64), bits(cam[idx, 2]))
    for r in (0, nvis // 2, nvis - 1):
        assert bits(e.getPointDepthCamVisible(r))[0] == got["depth"][:2 * nvis].view(np.uint64)[r]
    e.close()


def test_export_past_the_last_generation_of_the_descriptor_ring(small_est):
    """35 calls with different ragged tables are queued without a synchronisation in between (the ring has 16
    generations); every call's outputs are checked afterwards."""
    import torch
    S, calls = 3, 35
    sizes = (0, 1, 63, 64, 65, 130, 257, 1023, 1024, 1025, 1500)
    pool = {n: random_cloud(n, 700 + n) for n in sizes}
    for cl in pool.values():  # lidar coordinates of random_cloud -> the small camera's: x right, y down, z forward
        cl[:, :3] = np.stack([-cl[:, 1], -cl[:, 2] * 8, cl[:, 0]], axis=1)
    pc = ProjectedClouds(small_est, S, max(sizes))
    queued = []
    for k in range(calls):  # the buffers of ALL calls first ...
        ns = [sizes[(k + 3 * s) % len(sizes)] for s in range(S)]
        caps = [n if (k + s) % 3 else n // 2 for s, n in enumerate(ns)]
        queued.append((ns, caps, prepare(SMALL_CAM, [pool[n] for n in ns], caps=caps, cam_out=False)))
    torch.cuda.synchronize()
    for _, _, q in queued:  # ... then the calls back to back
        issue(pc, q)
    small_est.synchronize()
    pc.close()
    some = 0
    for k, (ns, caps, q) in enumerate(queued):
        for s, g in enumerate(collect(q)):
            want = expected(pool[ns[s]], SMALL_CAM, SMALL_T, key=("ring", ns[s]))
            check(g, want, ns[s], caps[s], f"call {k} [{s}]")
            some += want["nvis"]
    assert some > 0


def test_arguments_are_refused_by_name(est):
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    st = C.c_int(0)
    cam = kitti_camera().as_struct()
    T = np.ascontiguousarray(np.asarray(synth.T_CAM_LIDAR, dtype=np.float64).reshape(-1)[:12])
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    assert not lib.mld_projected_clouds_create(est._ctx, 2, 100, None, Tp, C.byref(st)) and st.value == capi.MLD_ERR_INVALID_ARG
    assert "camera" in lib.mld_projected_clouds_last_error(None).decode()
    pc = lib.mld_projected_clouds_create(est._ctx, 2, 100, C.byref(cam), Tp, C.byref(st))
    assert pc and st.value == capi.MLD_OK
    cloud = torch.zeros((101, 4), dtype=torch.float32, device=dev)
    uv = torch.full((400 + PAD,), GUARD, dtype=torch.int32, device=dev)
    index = torch.full((100 + PAD,), GUARD, dtype=torch.int32, device=dev)
    nvis = torch.full((2,), -7, dtype=torch.int64, device=dev)
    tab = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())  # noqa: E731
    half = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)  # noqa: E731
    odd = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr() + 2)  # noqa: E731
    i64 = lambda a, b: (C.c_int64 * 2)(a, b)  # noqa: E731
    good = dict(pts=tab(cloud), n=i64(100, 100), stride=16, cap=i64(100, 100), nvis=nvis.data_ptr(), uv=tab(uv), index=tab(index))

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.mld_projected_clouds_export_device(pc, a["pts"], a["n"], a["stride"], a["cap"], a["nvis"], a["uv"], a["index"],
                                                    None, None, None)
        return rc, lib.mld_projected_clouds_last_error(pc).decode()

    torch.cuda.synchronize()
    for kw, word in ((dict(pts=None), "pts_dev"), (dict(n=None), "table n"), (dict(cap=None), "capacity"),
                     (dict(nvis=None), "n_visible_out_dev"), (dict(uv=None), "uv_out"), (dict(index=None), "index_out"),
                     (dict(stride=12), "stride_bytes"), (dict(stride=64), "stride_bytes"), (dict(n=i64(100, -1)), "negative n"),
                     (dict(cap=i64(100, -1)), "negative capacity"), (dict(pts=half(cloud)), "pts_dev"),
                     (dict(uv=half(uv)), "uv_out"), (dict(index=half(index)), "index_out"),
                     (dict(pts=odd(cloud)), "4-byte aligned")):
        rc, text = call(**kw)
        assert rc == capi.MLD_ERR_INVALID_ARG and word in text and "mld_projected_clouds_export_device" in text, (kw, text)
    rc, text = call(n=i64(100, 101))
    assert rc == capi.MLD_ERR_CAPACITY and "max_points" in text
    est.synchronize()
    assert (uv.cpu().numpy() == GUARD).all() and (index.cpu().numpy() == GUARD).all() and (nvis.cpu().numpy() == -7).all()
    # a sequence without points, and one without capacity, need no arrays; a cloud of zeros has no visible point
    for kw in (dict(n=i64(100, 0), pts=half(cloud), uv=half(uv), index=half(index)),
               dict(cap=i64(100, 0), uv=half(uv), index=half(index))):
        rc, text = call(**kw)
        assert rc == capi.MLD_OK, text
        est.synchronize()
        assert nvis.cpu().numpy().tolist() == [0, 0]
    assert (uv.cpu().numpy() == GUARD).all() and (index.cpu().numpy() == GUARD).all()
    lib.mld_projected_clouds_destroy(pc)


def test_tracklet_batch_projected_clouds_on_three_ragged_sequences():
    """The Python route: device tensors out, consumed by torch without a host synchronisation of the caller's."""
    import torch
    dev = torch.device("cuda:0")
    host = [random_cloud(1025, 100 + 1025), None, random_cloud(65, 100 + 65)]
    tb = TrackletBatch(capi.params_c0(), kitti_camera(), synth.T_CAM_LIDAR, 3, 16)
    with pytest.raises(Exception, match="attach_projected_clouds"):
        tb.projected_clouds([None] * 3)
    tb.attach_projected_clouds(2000)
    clouds = [torch.from_numpy(c).to(dev) if c is not None else None for c in host]
    out = tb.projected_clouds(clouds, depth=True, cam=True, pixel_map=True)
    nv = out["n_visible"].cpu().numpy()
    for s, c in enumerate(host):
        n = 0 if c is None else c.shape[0]
        want = expected(c if c is not None else np.empty((0, 4), np.float32), key=("sizes", n))
        m = want["nvis"]
        assert nv[s] == m
        assert tuple(out["uv"][s].shape) == (n, 2) and tuple(out["cam"][s].shape) == (n, 3)
        assert np.array_equal(bits(out["uv"][s][:m].cpu().numpy()), bits(want["uv"]))
        assert np.array_equal(out["index"][s][:m].cpu().numpy(), want["index"])
        assert np.array_equal(bits(out["depth"][s][:m].cpu().numpy()), bits(want["cam"][want["index"], 2]))
        assert np.array_equal(bits(out["cam"][s].cpu().numpy()), bits(want["cam"]))
        assert np.array_equal(out["pixel_map"][s].cpu().numpy(), want["map"])
    few = tb.projected_clouds(clouds, capacity=[10, 0, 1000])
    assert few["depth"] is None and few["cam"] is None and few["pixel_map"] is None
    assert np.array_equal(few["n_visible"].cpu().numpy(), nv)
    assert tuple(few["uv"][0].shape) == (10, 2) and tuple(few["index"][2].shape) == (65,)
    assert np.array_equal(few["index"][0].cpu().numpy(), expected(host[0], key=("sizes", 1025))["index"][:10])
    none = tb.projected_clouds([None] * 3, pixel_map=True)  # a frame in which every sequence is empty
    assert none["n_visible"].cpu().numpy().tolist() == [0, 0, 0]
    assert all(int(t.numel()) == 0 for t in none["uv"] + none["index"])
    assert all(bool((m == -1).all()) for m in none["pixel_map"])
    tb.close()
