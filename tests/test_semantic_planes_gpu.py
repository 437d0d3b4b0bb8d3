"""mld_semantic_planes_estimate_device (SemanticPlanes, TrackletBatch.semantic_planes) against the oracle's
estimate_semantic_plane and against the one-slot path mld_estimate_semantic_plane_device: coefficients as raw bits,
counts, status and every mask word must be EQUAL - the association of the float sums is fixed, there is no tolerance.

Point counts and what they reach (a wavefront reduces a GROUP of 64 points, a block of the streaming kernels takes
1024 points = 16 groups, the fit adds group g into partial g % 256):
  3                  three candidates: the dummy prior (0, 0, 1, 0) as first plane, status 0 (by construction the one
                     success case without 4 candidates)
  63, 64, 65         one group, not full / full / a second group of one point (and a second mask word pair)
  255, 256, 257      the wavefronts of a block; 1023, 1024, 1025: a second block
  16 384             exactly 256 groups: every partial once;  16 385 + 64: partials 0 and 1 twice
  28 800             the whole VLP-16 cloud
Sub-clouds are seeded random subsets of a VLP-16 frame in which a third of the points (at most all there are) are
ground candidates.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import SemanticPlanes, TrackletBatch, capi, synth
from oracle import np_restatement

from helpers import kitti_camera, make_estimator, make_oracle

pytestmark = pytest.mark.gpu

LABELS = (6, 7, 8, 9)  # tracklet_depth_module.cpp:280
THR = 0.1
SIZES = (3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16384, 16385 + 64, 28800)
GUARD = 0x5A5AA5A5
PAD = 3


def candidates_of(cloud, img, labels=LABELS):
    """Indices of the points whose projection hits a ground label (RansacPlane.cpp:198-221), as
    np_restatement.semantic_plane finds them - which raises below three and so cannot count those."""
    T = synth.T_CAM_LIDAR
    x, y, z = (cloud[:, k].astype(np.float64) for k in range(3))
    pc = [(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32).astype(np.float64) for r in range(3)]
    with np.errstate(all="ignore"):
        p0 = synth.KITTI_F * pc[0] + (0.0 * pc[1] + synth.KITTI_CU * pc[2])
        p1 = 0.0 * pc[0] + (synth.KITTI_F * pc[1] + synth.KITTI_CV * pc[2])
        p2 = 0.0 * pc[0] + (0.0 * pc[1] + 1.0 * pc[2])
        u, v = p0 / p2, p1 / p2
        ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 2147483648.0) & (np.abs(v) < 2147483648.0)
        ix = np.where(ok, np.trunc(np.where(ok, u, 0.0)), -1).astype(np.int64)
        iy = np.where(ok, np.trunc(np.where(ok, v, 0.0)), -1).astype(np.int64)
    ok &= (ix >= 0) & (ix < img.shape[1]) & (iy >= 0) & (iy < img.shape[0])
    lab = np.full(cloud.shape[0], -1, dtype=np.int64)
    lab[ok] = img[iy[ok], ix[ok]]
    cand = np.nonzero(np.isin(lab, np.asarray(labels)))[0].astype(np.int32)
    if cand.size >= 3:
        assert np.array_equal(cand, np_restatement.semantic_plane(cloud, T, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, img,
                                                                  labels, THR)[0])
    return cand


def frame(seed, frame_no=1):
    cloud = synth.make_cloud(synth.VLP16, seed=seed, frame=frame_no)
    return cloud, synth.make_label_image(cloud)


def sub_cloud(cloud, cand, n, seed):
    """n points of the cloud in random order, max(4, n / 3) of them candidates that are ground returns (3 of 3; the
    candidate set also holds returns behind the camera whose mirrored projection hits a ground pixel: left out here, so
    that the first plane is the ground and the selection finds inliers)."""
    if n == cloud.shape[0]:
        return cloud
    rng = np.random.default_rng(seed)
    ground = cand[np.abs(cloud[cand, 2] - synth.GROUND_Z) < 0.05]
    k = min(n, ground.size, max(4, n // 3)) if n > 3 else n
    other = np.setdiff1d(np.arange(cloud.shape[0]), cand)
    idx = np.concatenate([rng.choice(ground, k, replace=False), rng.choice(other, n - k, replace=False)])
    return np.ascontiguousarray(cloud[rng.permutation(idx)])


def expected(cloud, img, thr=THR, labels=LABELS):
    """(coeffs float32[4], n_candidates, n_inliers, status, mask words uint32) from the oracle."""
    n = cloud.shape[0]
    words = (n + 31) // 32
    n_cand = int(candidates_of(cloud, img, labels).size) if n else 0
    if n < 3 or n_cand < 3:
        return np.zeros(4, np.float32), n_cand, 0, 1, np.zeros(words, np.uint32)
    ref = make_oracle(capi.params_c0())
    ref.set_cloud(cloud)
    coeffs, inl = ref.estimate_semantic_plane(img, labels, thr)
    m = np.zeros(words, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, np.uint32(1) << (inl & 31).astype(np.uint32))
    return coeffs, n_cand, int(inl.size), 0, m


_CASES = {}


def case(n):
    """The sub-cloud of n points, its image and the oracle's answer; made once."""
    if n not in _CASES:
        cloud, img = frame(5)
        sub = sub_cloud(cloud, candidates_of(cloud, img), n, 1000 + n)
        want = expected(sub, img)
        assert want[3] == 0 and want[1] >= min(n, 4) and (n == 3 or want[2] >= 4), (n, want[1:4])  # not a fallback
        _CASES[n] = (sub, img, want)
    return _CASES[n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def est():
    e = make_estimator(capi.params_c0(), max_frames=1)
    yield e
    e.close()


def device_cloud(cloud, stride, dev):
    import torch
    if stride == 32:
        wide = np.full((cloud.shape[0], 8), np.nan, dtype=np.float32)  # (what lies behind x, y, z must not matter)
        wide[:, :3] = cloud[:, :3]
        cloud = wide
    return torch.from_numpy(np.ascontiguousarray(cloud)).to(dev)


def mask_buffers(ns, dev, misalign=False):
    """Per sequence a guarded buffer and the view handed to the call: `words` entries, then PAD guard words."""
    import torch
    bufs, views = [], []
    for n in ns:
        w = (n + 31) // 32
        b = torch.full((1 + w + PAD,), GUARD, dtype=torch.int32, device=dev)
        v = b[1:] if misalign else b[:-1]
        if misalign:
            assert v.data_ptr() % 8 == 4
        bufs.append(b)
        views.append(v)
    return bufs, views


def run(est, clouds, imgs, stride=16, thr=THR, labels=LABELS, misalign=False, d_imgs=None):
    """One call for the given sequences; returns [(coeffs, n_candidates, n_inliers, status, mask words, guard ok)]."""
    import torch
    dev = torch.device("cuda:0")
    S = len(clouds)
    ns = [c.shape[0] for c in clouds]
    d_clouds = [device_cloud(c, stride, dev) for c in clouds]
    if d_imgs is None:
        d_imgs = [torch.from_numpy(np.ascontiguousarray(im)).to(dev) for im in imgs]
    res = torch.full((S, 8), -1, dtype=torch.int32, device=dev)
    bufs, views = mask_buffers(ns, dev, misalign)
    torch.cuda.synchronize()
    sp = SemanticPlanes(est, S, max(max(ns), 1))
    sp.estimate(d_clouds, d_imgs, labels, thr, res, views)
    est.synchronize()
    sp.close()
    r = res.cpu().numpy()
    out = []
    for s, n in enumerate(ns):
        w = (n + 31) // 32
        v = views[s].cpu().numpy().view(np.uint32)
        whole = bufs[s].cpu().numpy()
        outside = whole[1 + w:] if misalign else whole[w:]
        guard_ok = bool((outside == GUARD).all()) and (not misalign or whole[0] == GUARD)
        assert r[s, 7] == 0
        out.append((r[s, :4].copy().view(np.float32), int(r[s, 4]), int(r[s, 5]), int(r[s, 6]), v[:w].copy(), guard_ok))
    return out


def check(got, want, what=""):
    coeffs, n_cand, n_inl, status, mask, guard_ok = got
    assert status == want[3], what
    assert n_cand == want[1], (what, n_cand, want[1])
    assert n_inl == want[2], (what, n_inl, want[2])
    assert np.array_equal(bits(coeffs), bits(want[0])), (what, coeffs, want[0])
    assert np.array_equal(mask, want[4]), (what, np.flatnonzero(mask != want[4])[:8])
    assert guard_ok, what


@pytest.mark.parametrize("stride", [16, 32])
def test_mixed_sizes_in_one_call_equal_the_oracle(est, stride):
    cs = [case(n) for n in SIZES]
    got = run(est, [c[0] for c in cs], [c[1] for c in cs], stride=stride)
    for n, g, c in zip(SIZES, got, cs):
        check(g, c[2], f"n={n}")
    assert bits(cs[0][2][0]).tolist() == bits([0, 0, 1, 0]).tolist() and cs[0][2][1] == 3  # the dummy prior, unrefined


@pytest.mark.parametrize("n_seq", [1, 2, 5])
def test_sizes_one_at_a_time_equal_the_oracle(est, n_seq):
    """Every size alone (n_seq 1), or with copies of itself and of its neighbours in the list (n_seq 2, 5)."""
    for k, n in enumerate(SIZES):
        pick = [SIZES[(k + j) % len(SIZES)] for j in range(n_seq)]
        cs = [case(m) for m in pick]
        got = run(est, [c[0] for c in cs], [c[1] for c in cs], stride=16 if k % 2 == 0 else 32)
        for m, g, c in zip(pick, got, cs):
            check(g, c[2], f"n={m} in {pick}")


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_equal_to_the_one_slot_path(seed):
    """mld_estimate_semantic_plane_device on a slot of a one-slot estimator against the batched call, same inputs."""
    import torch
    dev = torch.device("cuda:0")
    cloud, img = frame(seed)
    thr = (0.1, 0.3, 0.05)[seed - 3]
    e = make_estimator(capi.params_c0(), max_frames=1)
    d_cloud = torch.from_numpy(cloud).to(dev)
    d_img = torch.from_numpy(img).to(dev)
    e.setInputCloud(d_cloud, None, plane_given=False)
    c_one, n_one = e.estimateSemanticPlane(d_img, LABELS, thr)
    inl = e.getGroundPlaneInliers()
    got = run(e, [cloud], [img], thr=thr)[0]
    e.close()
    m = np.zeros((cloud.shape[0] + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, np.uint32(1) << (inl & 31).astype(np.uint32))
    assert n_one >= 4 and got[1] >= 4 and got[3] == 0 and got[2] == n_one  # (no fallback: 143, 888, 91 inliers)
    assert np.array_equal(bits(got[0]), bits(c_one)) and np.array_equal(got[4], m) and got[5]
    check(got, expected(cloud, img, thr), f"seed {seed}")


def test_a_mask_that_is_not_8_byte_aligned_and_its_neighbours(est):
    """Masks at 4 (mod 8); the words before and after each mask keep their guard value.  Odd word counts (65 points = 3
    words) end in the middle of a wavefront's ballot."""
    sizes = (65, 255, 1025, 28800)
    cs = [case(n) for n in sizes]
    got = run(est, [c[0] for c in cs], [c[1] for c in cs], misalign=True)
    for n, g, c in zip(sizes, got, cs):
        check(g, c[2], f"n={n}")


def test_strided_rows_a_small_image_and_an_image_per_sequence(est):
    import torch
    dev = torch.device("cuda:0")
    # (a) row_stride_bytes > cols, odd base address
    sub, img, want = case(28800)
    rows, cols = img.shape
    buf = torch.zeros(rows * (cols + 37) + 64, dtype=torch.uint8, device=dev)
    view = buf[3:3 + rows * (cols + 37)].view(rows, cols + 37)[:, :cols]
    view.copy_(torch.from_numpy(img).to(dev))
    buf[3:3 + rows * (cols + 37)].view(rows, cols + 37)[:, cols:] = 7  # (a ground label in the padding: never read)
    check(run(est, [sub], None, d_imgs=[view])[0], want, "strided rows")
    # (b) an image smaller than the camera: projections beyond it are no candidates; odd label sets
    cloud, full = frame(11)
    small = np.ascontiguousarray(full[:330, :1000])  # (top left corner: the pixel coordinates stay)
    labels = (7, 8, -3, 300, 7)
    want_small = expected(cloud, small, 0.2, labels)
    assert want_small[3] == 0 and 4 <= want_small[1] < candidates_of(cloud, full).size
    check(run(est, [cloud], [small], thr=0.2, labels=labels)[0], want_small, "small image")
    # (c) three sequences, each with the image of its own frame
    frames = [frame(20 + s, s) for s in range(3)]
    wants = [expected(c, im) for c, im in frames]
    assert all(w[3] == 0 and w[2] >= 4 for w in wants) and len({w[1] for w in wants}) == 3
    got = run(est, [f[0] for f in frames], [f[1] for f in frames])
    for s in range(3):
        check(got[s], wants[s], f"sequence {s}")


@pytest.mark.parametrize("bad", ["no ground label", "n = 0", "n = 2"])
def test_a_failed_sequence_among_good_ones(est, bad):
    """Status 1, zero coefficients, zero mask for the failed sequence; its neighbours as if it were not there."""
    a, b = case(1025), case(257)
    if bad == "no ground label":
        cloud, img = a[0], np.full_like(a[1], 23)
    else:
        cloud, img = a[0][:int(bad[-1])], a[1]
    want = expected(cloud, img)
    assert want[3] == 1 and not want[0].any() and want[2] == 0
    got = run(est, [a[0], cloud, b[0]], [a[1], img, b[1]])
    check(got[0], a[2], "before")
    check(got[1], want, bad)
    check(got[2], b[2], "after")
    alone = run(est, [a[0]], [a[1]])[0]
    assert np.array_equal(bits(alone[0]), bits(got[0][0])) and np.array_equal(alone[4], got[0][4])


def test_three_candidates_give_the_dummy_prior_and_no_failure(est):
    """An image with exactly three ground pixels, each hit by a cloud point: the first fit needs more than 3 members
    and returns (0, 0, 1, 0); the selection and the refit run against that plane."""
    cloud, img = frame(7)
    xyz = cloud[:, :3].astype(np.float64)
    cam = xyz @ synth.T_CAM_LIDAR[:, :3].T + synth.T_CAM_LIDAR[:, 3]
    z = cam[:, 2]
    with np.errstate(all="ignore"):
        u = np.trunc(cam[:, 0] / z * synth.KITTI_F + synth.KITTI_CU)
        v = np.trunc(cam[:, 1] / z * synth.KITTI_F + synth.KITTI_CV)
    ok = np.nonzero((z > 1) & (u >= 0) & (u < synth.KITTI_W) & (v >= 0) & (v < synth.KITTI_H))[0]
    img3 = np.zeros_like(img)
    for i in ok:
        img3[int(v[i]), int(u[i])] = 7
        if int((img3 == 7).sum()) == 3:
            break
    want = expected(cloud, img3)
    assert want[3] == 0 and want[1] >= 3
    got = run(est, [cloud], [img3])[0]
    check(got, want, "three ground pixels")
    if want[1] == 3:  # (several points may share the three pixels)
        # selection against z = 0: the inliers are the points with |z| < thr, the refit is theirs (or the prior again)
        sel = np.abs(cloud[:, 2].astype(np.float32)).astype(np.float64) < THR
        assert got[2] == int(sel.sum())


def test_arguments_are_refused_by_name(est):
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    st = C.c_int(0)
    cam = kitti_camera().as_struct()
    T = np.ascontiguousarray(synth.T_CAM_LIDAR.reshape(-1)[:12])
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    assert not lib.mld_semantic_planes_create(est._ctx, 2, 100, None, Tp, C.byref(st)) and st.value == capi.MLD_ERR_INVALID_ARG
    assert "camera" in lib.mld_semantic_planes_last_error(None).decode()
    assert not lib.mld_semantic_planes_create(est._ctx, 2, 100, C.byref(cam), None, C.byref(st))
    assert "T_cam_lidar" in lib.mld_semantic_planes_last_error(None).decode()
    sp = lib.mld_semantic_planes_create(est._ctx, 2, 100, C.byref(cam), Tp, C.byref(st))
    assert sp and st.value == capi.MLD_OK
    cloud = torch.zeros((100, 4), dtype=torch.float32, device=dev)
    img = torch.zeros((4, 8), dtype=torch.uint8, device=dev)
    mask = torch.full((4 + PAD,), GUARD, dtype=torch.int32, device=dev)
    res = torch.full((2, 8), -1, dtype=torch.int32, device=dev)
    lab = (C.c_int32 * 4)(*LABELS)
    tab = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())  # noqa: E731
    half = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)  # noqa: E731
    good = dict(pts=tab(cloud), n=(C.c_int64 * 2)(100, 100), stride=16, img=tab(img), rows=4, cols=8, row_stride=8,
                labels=C.addressof(lab), n_labels=4, thr=0.1, res=res.data_ptr(), mask=tab(mask))

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.mld_semantic_planes_estimate_device(sp, a["pts"], a["n"], a["stride"], a["img"], a["rows"], a["cols"],
                                                     a["row_stride"], a["labels"], a["n_labels"], a["thr"], a["res"], a["mask"])
        return rc, lib.mld_semantic_planes_last_error(sp).decode()

    torch.cuda.synchronize()
    for kw, word in ((dict(pts=None), "pts_dev"), (dict(n=None), "table n"), (dict(img=None), "label_image_dev"),
                     (dict(res=None), "result_out_dev"), (dict(mask=None), "mask_out_dev"), (dict(rows=0), "rows"),
                     (dict(cols=-2), "cols"), (dict(row_stride=7), "row_stride_bytes"), (dict(stride=12), "stride_bytes"),
                     (dict(stride=64), "stride_bytes"), (dict(n_labels=-1), "n_labels"), (dict(labels=None), "ground_labels"),
                     (dict(n=(C.c_int64 * 2)(100, -1)), "negative n"), (dict(pts=half(cloud)), "pts_dev"),
                     (dict(img=half(img)), "label_image_dev"), (dict(mask=half(mask)), "mask_out_dev")):
        rc, text = call(**kw)
        assert rc == capi.MLD_ERR_INVALID_ARG and word in text and "mld_semantic_planes_estimate_device" in text, (kw, text)
    rc, text = call(n=(C.c_int64 * 2)(100, 101))
    assert rc == capi.MLD_ERR_CAPACITY and "max_points" in text
    est.synchronize()
    assert (mask.cpu().numpy() == GUARD).all() and (res.cpu().numpy() == -1).all()  # nothing was launched
    # a sequence without points needs no arrays; labels may be absent with n_labels == 0 (no candidates then)
    rc, text = call(n=(C.c_int64 * 2)(100, 0), pts=half(cloud), img=half(img), mask=half(mask), labels=None, n_labels=0)
    assert rc == capi.MLD_OK, text
    est.synchronize()
    r = res.cpu().numpy()
    assert (r[:, 6] == 1).all() and not r[:, :6].any() and not r[:, 7].any()
    m = mask.cpu().numpy()
    assert not m[:4].any() and (m[4:] == GUARD).all()
    lib.mld_semantic_planes_destroy(sp)


def test_two_calls_queued_through_one_set_of_host_tables(est):
    """Two calls back to back through ONE set of host tables, rewritten in between, one synchronisation at the end."""
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    S = 2
    picks = [(1025, 257), (65, 16384)]
    sp = SemanticPlanes(est, S, 16384)
    t_pts, t_img, t_mask = ((C.c_void_p * S)() for _ in range(3))
    t_n = (C.c_int64 * S)()
    lab = (C.c_int32 * 4)(*LABELS)
    keep = []
    for pick in picks:
        cs = [case(n) for n in pick]
        d_clouds = [torch.from_numpy(c[0]).to(dev) for c in cs]
        d_imgs = [torch.from_numpy(c[1]).to(dev) for c in cs]
        bufs, views = mask_buffers(pick, dev)
        res = torch.full((S, 8), -1, dtype=torch.int32, device=dev)
        keep.append((cs, d_clouds, d_imgs, bufs, views, res))
    torch.cuda.synchronize()
    for cs, d_clouds, d_imgs, bufs, views, res in keep:
        for s in range(S):
            t_pts[s], t_img[s], t_mask[s], t_n[s] = d_clouds[s].data_ptr(), d_imgs[s].data_ptr(), views[s].data_ptr(), d_clouds[s].shape[0]
        rc = lib.mld_semantic_planes_estimate_device(sp._sp, t_pts, t_n, 16, t_img, synth.KITTI_H, synth.KITTI_W, synth.KITTI_W,
                                                     C.addressof(lab), 4, THR, res.data_ptr(), t_mask)
        assert rc == capi.MLD_OK, lib.mld_semantic_planes_last_error(sp._sp).decode()
        for s in range(S):  # (what a caller that reuses its tables does next; the values must not matter any more)
            t_pts[s] = t_img[s] = t_mask[s] = None
            t_n[s] = 0
    est.synchronize()
    for cs, d_clouds, d_imgs, bufs, views, res in keep:
        r = res.cpu().numpy()
        for s in range(S):
            w = (cs[s][0].shape[0] + 31) // 32
            whole = bufs[s].cpu().numpy()
            got = (r[s, :4].copy().view(np.float32), int(r[s, 4]), int(r[s, 5]), int(r[s, 6]), whole[:w].view(np.uint32),
                   bool((whole[w:] == GUARD).all()))
            check(got, cs[s][2], f"n={cs[s][0].shape[0]}")
    sp.close()


def test_calls_queued_past_the_last_generation_of_the_descriptor_ring(est):
    """35 calls (twice the 16 pinned generations of the descriptor ring and three more) with no synchronisation in
    between, through ONE set of host tables rewritten after every call, each call with its own result tensor and
    guarded masks: every generation's event is waited for and recorded again, and every call equals the oracle."""
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    S, calls, sizes = 2, 2 * 16 + 3, (3, 63, 64, 65, 255, 257)
    sp = SemanticPlanes(est, S, 257)
    t_pts, t_img, t_mask = ((C.c_void_p * S)() for _ in range(3))
    t_n = (C.c_int64 * S)()
    lab = (C.c_int32 * 4)(*LABELS)
    d_cloud = {n: torch.from_numpy(case(n)[0]).to(dev) for n in sizes}
    d_img = torch.from_numpy(case(sizes[0])[1]).to(dev)  # (every case is a sub-cloud of one frame: one image)
    assert all(np.array_equal(case(n)[1], case(sizes[0])[1]) for n in sizes)
    keep = []
    for k in range(calls):
        pick = (sizes[k % 6], sizes[(k + 1) % 6])
        bufs, views = mask_buffers(pick, dev)
        keep.append((pick, bufs, views, torch.full((S, 8), -1, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for pick, bufs, views, res in keep:
        for s in range(S):
            t_pts[s], t_img[s], t_mask[s], t_n[s] = d_cloud[pick[s]].data_ptr(), d_img.data_ptr(), views[s].data_ptr(), pick[s]
        rc = lib.mld_semantic_planes_estimate_device(sp._sp, t_pts, t_n, 16, t_img, synth.KITTI_H, synth.KITTI_W, synth.KITTI_W,
                                                     C.addressof(lab), 4, THR, res.data_ptr(), t_mask)
        assert rc == capi.MLD_OK, lib.mld_semantic_planes_last_error(sp._sp).decode()
        for s in range(S):
            t_pts[s] = t_img[s] = t_mask[s] = None
            t_n[s] = 0
    est.synchronize()
    for k, (pick, bufs, views, res) in enumerate(keep):
        r = res.cpu().numpy()
        for s in range(S):
            w = (pick[s] + 31) // 32
            whole = bufs[s].cpu().numpy()
            got = (r[s, :4].copy().view(np.float32), int(r[s, 4]), int(r[s, 5]), int(r[s, 6]), whole[:w].view(np.uint32),
                   bool((whole[w:] == GUARD).all()))
            check(got, case(pick[s])[2], f"call {k}, n={pick[s]}")
    sp.close()


def test_tracklet_batch_with_its_own_planes_equals_the_oracle_fed_batch():
    """Two sequences, two frames: TrackletBatch.run with the planes of semantic_planes() against a second batch fed the
    oracle's coefficients and inlier masks - depths and types identical, and the road fallback did answer features.
    The clouds are the front halves of VLP-16 frames (x > 0.5 m): the returns behind the camera, whose mirrored
    projection hits ground pixels too, would tilt the plane away from the road.  On these sparse clouds few features
    end on the road fallback (the oracle alone gives 8 SuccessRoad among the 4 x 300 newest features)."""
    import torch
    dev = torch.device("cuda:0")
    P, cam, S, NT = capi.params_c0(), kitti_camera(), 2, 300
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(17)
    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, NT)
    tb_ref = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, NT)
    tb.attach_planes(synth.VLP16.rings * synth.VLP16.azimuth_steps)
    road = 0
    for f in range(2):
        frames = [frame(40 + s, f) for s in range(S)]
        frames = [(np.ascontiguousarray(c[c[:, 0] > 0.5]), im) for c, im in frames]
        clouds = [to(c) for c, _ in frames]
        d_imgs = [to(im) for _, im in frames]
        thr = 0.2
        wants = [expected(c, im, thr) for c, im in frames]
        assert all(w[3] == 0 and w[2] >= 4 for w in wants)
        coeffs, masks, status, counts = tb.semantic_planes(clouds, d_imgs, LABELS, thr)
        assert coeffs.shape == (S, 4) and coeffs.dtype == np.float32 and not status.any()
        for s in range(S):
            assert np.array_equal(bits(coeffs[s]), bits(wants[s][0])) and tuple(counts[s]) == wants[s][1:3]
            assert np.array_equal(masks[s].cpu().numpy().view(np.uint32), wants[s][4])
        uv = [synth.make_features_near_points(c, NT, seed=50 + 2 * f + s) for s, (c, _) in enumerate(frames)]
        u0 = [to(x[:, 0].astype(np.float32)) for x in uv]
        v0 = [to(x[:, 1].astype(np.float32)) for x in uv]
        u1 = [to((x[:, 0] + rng.normal(0, 3, NT)).astype(np.float32)) for x in uv]
        v1 = [to((x[:, 1] + rng.normal(0, 2, NT)).astype(np.float32)) for x in uv]
        is_new = [to((rng.random(NT) < (1.0 if f == 0 else 0.3)).astype(np.uint8)) for _ in range(S)]

        def outputs():
            return ([torch.empty(NT, dtype=torch.float32, device=dev) for _ in range(S)],
                    [torch.full((NT,), float("nan"), dtype=torch.float32, device=dev) for _ in range(S)],
                    [torch.empty(NT, dtype=torch.int32, device=dev) for _ in range(S)],
                    [torch.zeros(NT, dtype=torch.int32, device=dev) for _ in range(S)])
        o, o_ref = outputs(), outputs()
        ref_masks = [to(w[4].view(np.int32)) for w in wants]
        torch.cuda.synchronize()
        tb.run(tb.prepare(clouds, coeffs, masks, u0, v0, u1, v1, is_new, *o))
        tb_ref.run(tb_ref.prepare(clouds, np.stack([w[0] for w in wants]), ref_masks, u0, v0, u1, v1, is_new, *o_ref))
        tb.est.synchronize()
        tb_ref.est.synchronize()
        for s in range(S):
            for a, b in zip(o, o_ref):
                x, y = a[s].cpu().numpy(), b[s].cpu().numpy()
                assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y), (f, s)
            road += int((o_ref[2][s].cpu().numpy() == 16).sum())
    assert road >= 4, road  # SuccessRoad: the planes were used
    tb.close()
    tb_ref.close()
