"""mld_labels_assign_device (SemanticLabels, TrackletBatch.labels) against tests/label_restatement.py: every label and,
where requested, every vote pair must be EQUAL - the answer is an integer count, there is no tolerance.

The implementation has two kernel shapes and switches between them on the NOMINAL window 2*(w/2) x 2*(h/2):
  * at most 16 pixels -> one 16-lane row per track (k_labels_row); more -> one wavefront per track (k_labels_wave).
    (4, 4) and (5, 5) are 16 pixels, (6, 4) is 24, (2, 8) / (8, 2) are 16 and (2, 10) is 20: windows on both sides.
    A nominal area of 0 ((0, 0), (1, 1)) takes the row shape with no pixel in any window.
  * inside the row shape the lane -> pixel map divides by the nominal width 2, 4, 6 or 8: (2, 2), (4, 4), (6, 2), (8, 2).
  * inside the wavefront shape: a clipped window of at most 64 pixels is one pass, a larger one several ((8, 8) is
    exactly 64); a clipped window narrower than 64 columns advances rows every pass, a wider one does not (the 1 x 200
    image with (200, 2) and (1000, 1000)); 64 equal labels take one histogram update, mixed ones one per lane (the
    alphabet of 2 against the alphabet of 256).
  * a block answers 256 tracks in the row shape (sequences of 256 and 257 tracks) and 32 in the other.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import SemanticLabels, TrackletBatch, capi, synth

from helpers import kitti_camera, make_estimator
from label_restatement import NO_LABEL, assign_labels

pytestmark = pytest.mark.gpu

WINDOWS = [(0, 0), (1, 1), (2, 2), (3, 2), (4, 4), (5, 5), (6, 4), (8, 8), (9, 9), (10, 8), (50, 50), (2, 200), (200, 2),
           (1000, 1000), (6, 2), (8, 2), (2, 8), (2, 10)]
# (rows, cols, row stride in bytes, number of label values)
IMAGES = [(37, 53, 53, 5), (37, 53, 61, 2), (37, 53, 61, 256), (1, 1, 1, 5), (1, 200, 200, 2), (1, 200, 203, 5)]
BATCHES = [(0, 1, 600), (257, 0, 0, 256, 3)]
UNWRITTEN_LABEL, UNWRITTEN_VOTE, PAD = 12345, -77777, 7


def make_image(rng, rows, cols, n_values):
    """Blocks of a few pixels of one label with single-pixel noise: windows with a clear winner, windows on an edge
    between two labels (ties) and windows of one label all occur."""
    values = rng.choice(256, n_values, replace=False).astype(np.uint8) if n_values < 256 else np.arange(256, dtype=np.uint8)
    coarse = rng.integers(0, n_values, ((rows + 2) // 3, (cols + 3) // 4))
    img = np.repeat(np.repeat(coarse, 3, axis=0), 4, axis=1)[:rows, :cols]
    noise = rng.random((rows, cols)) < 0.15
    img = np.where(noise, rng.integers(0, n_values, (rows, cols)), img)
    return values[img]


def special_features(rows, cols):
    """(u, v) pairs with defined answers at and beyond every edge of the image and of the float -> int conversion."""
    w, h = float(cols), float(rows)
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    out = []
    # exactly on every border and corner
    out += [(0, cy), (w - 1, cy), (cx, 0), (cx, h - 1), (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    # up to 3 px outside every border (and the corners)
    for d in (1, 2, 3):
        out += [(-d, cy), (w - 1 + d, cy), (cx, -d), (cx, h - 1 + d), (-d, -d), (w - 1 + d, h - 1 + d)]
    # fractional negatives in (-1, 0): truncation gives pixel 0, not -1
    out += [(-0.7, cy), (cx, -0.7), (-0.001, -0.999), (-0.5, h - 0.5)]
    # fractional values just inside the last pixel
    out += [(w - 0.01, cy), (cx, h - 0.01)]
    # far outside, inside and beyond the range of int
    for far in (1e6, -1e6, 3e9, -3e9, 2147483648.0, -2147483648.0, 2147483520.0):
        out += [(far, cy), (cx, far), (far, far)]
    # not finite: in u, in v, in both
    for bad in (float("nan"), float("inf"), float("-inf")):
        out += [(bad, cy), (cx, bad), (bad, bad)]
    out += [(float("nan"), float("inf")), (float("-inf"), float("nan"))]
    return np.array(out, dtype=np.float32)


def make_features(rng, rows, cols, n, rotate):
    sp = special_features(rows, cols)
    if n < len(sp):
        return np.roll(sp, -rotate * 5, axis=0)[:n].copy()
    uni = np.stack([rng.uniform(0, cols, n - len(sp)), rng.uniform(0, rows, n - len(sp))], axis=1).astype(np.float32)
    return rng.permutation(np.concatenate([sp, uni]))  # (the special ones land in every block)


def device_image(img, stride, dev):
    """The image as a [rows, cols] view with the given row stride into a byte buffer, starting at an odd address."""
    import torch
    rows, cols = img.shape
    buf = torch.zeros(rows * stride + 64, dtype=torch.uint8, device=dev)
    view = buf[3:3 + rows * stride].view(rows, stride)[:, :cols]
    view.copy_(torch.from_numpy(img).to(dev))
    assert view.data_ptr() % 2 == 1 and (rows == 1 or view.stride(0) == stride)
    return view


@pytest.fixture(scope="module")
def est():
    e = make_estimator(capi.params_c0(), max_frames=1)
    yield e
    e.close()


def outputs(ns, dev):
    import torch
    lab = [torch.full((n + PAD,), UNWRITTEN_LABEL, dtype=torch.int16, device=dev) for n in ns]
    vot = [torch.full((n + PAD, 2), UNWRITTEN_VOTE, dtype=torch.int32, device=dev) for n in ns]
    return lab, vot


def check(ns, want, lab, vot, vote_mode):
    """Every entry of n_tracks[s] written and equal to the restatement, nothing beyond it touched."""
    for s, n in enumerate(ns):
        got = lab[s].cpu().numpy()
        assert np.array_equal(got[:n], want[s][0]), (s, np.flatnonzero(got[:n] != want[s][0])[:8])
        assert (got[n:] == UNWRITTEN_LABEL).all(), s
        gv = vot[s].cpu().numpy()
        written = vote_mode == "all" or (vote_mode == "not_last" and s != len(ns) - 1)
        if written:
            assert np.array_equal(gv[:n], want[s][1]), (s, np.flatnonzero((gv[:n] != want[s][1]).any(axis=1))[:8])
            assert (gv[n:] == UNWRITTEN_VOTE).all(), s
        else:
            assert (gv == UNWRITTEN_VOTE).all(), s


@pytest.mark.parametrize("ns", BATCHES, ids=lambda b: "n" + "-".join(map(str, b)))
@pytest.mark.parametrize("rows,cols,stride,n_values", IMAGES, ids=lambda x: str(x))
def test_assign_equals_the_restatement(est, rows, cols, stride, n_values, ns):
    """Every window of WINDOWS on one image geometry and one batch; votes_out present, NULL for the last sequence, and
    NULL as a table."""
    import torch
    dev = torch.device("cuda:0")
    S = len(ns)
    rng = np.random.default_rng(1000 * rows + cols + stride + 7 * n_values + S)
    imgs = [make_image(rng, rows, cols, n_values) for _ in range(S)]
    feats = [make_features(rng, rows, cols, n, s) for s, n in enumerate(ns)]
    d_imgs = [device_image(im, stride, dev) for im in imgs]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_u, d_v = [to(f[:, 0]) for f in feats], [to(f[:, 1]) for f in feats]
    sl = SemanticLabels(est, S)
    ties = nonempty = 0
    for roi in WINDOWS:
        want = [assign_labels(imgs[s], roi, feats[s][:, 0], feats[s][:, 1]) for s in range(S)]
        ties += sum(int(w[2].sum()) for w in want)
        nonempty += sum(int((w[0] != NO_LABEL).sum()) for w in want)
        runs = []
        for vote_mode in ("all", "not_last", "none"):
            lab, vot = outputs(ns, dev)
            torch.cuda.synchronize()
            votes = {"all": vot, "not_last": vot[:-1] + [None], "none": None}[vote_mode]
            sl.assign(d_imgs, roi, d_u, d_v, [t[:n] for t, n in zip(lab, ns)],
                      [t[:n] if t is not None else None for t, n in zip(votes, ns)] if votes is not None else None)
            runs.append((lab, vot, vote_mode))
        est.synchronize()
        for lab, vot, vote_mode in runs:
            check(ns, want, lab, vot, vote_mode)
        if roi[0] < 2 or roi[1] < 2:
            assert all((w[0] == NO_LABEL).all() and not w[1].any() for w in want)
    sl.close()
    assert nonempty > 0
    # the tie rule is this project's: the small alphabets must exercise it (a 1 x 1 image cannot tie)
    if n_values <= 5 and rows * cols > 1:
        assert ties > 20, ties


def test_arguments_are_refused_by_name(est):
    """Every refusal of mld_labels_assign_device happens on the host, before anything is launched."""
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    st = C.c_int(0)
    lb = lib.mld_labels_create(est._ctx, 2, C.byref(st))
    assert lb and st.value == capi.MLD_OK
    img = torch.zeros((4, 8), dtype=torch.uint8, device=dev)
    uv = torch.zeros(3, dtype=torch.float32, device=dev)
    out = torch.zeros(3, dtype=torch.int16, device=dev)
    tab = lambda t: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())  # noqa: E731
    n = (C.c_int64 * 2)(3, 3)
    good = dict(img=tab(img), rows=4, cols=8, stride=8, w=5, h=5, u=tab(uv), v=tab(uv), n=n, out=tab(out), votes=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.mld_labels_assign_device(lb, a["img"], a["rows"], a["cols"], a["stride"], a["w"], a["h"], a["u"], a["v"],
                                          a["n"], a["out"], a["votes"])
        return rc, lib.mld_labels_last_error(lb).decode()

    for kw, word in ((dict(img=None), "label_image_dev"), (dict(u=None), "u"), (dict(v=None), "v"), (dict(n=None), "n_tracks"),
                     (dict(out=None), "label_out"), (dict(w=-1), "roi_width"), (dict(h=-5), "roi_height"),
                     (dict(stride=7), "row_stride_bytes"), (dict(rows=0), "rows"), (dict(cols=-2), "cols"),
                     (dict(n=(C.c_int64 * 2)(3, -1)), "n_tracks"), (dict(out=(C.c_void_p * 2)(out.data_ptr(), None)), "label_out")):
        rc, text = call(**kw)
        assert rc == capi.MLD_ERR_INVALID_ARG and word in text and "mld_labels_assign_device" in text, (kw, text)
    rc, text = call()
    assert rc == capi.MLD_OK, text
    est.synchronize()
    assert (out.cpu().numpy() == 0).all()  # (an image of zeros)
    # a sequence without tracks needs no arrays
    rc, text = call(n=(C.c_int64 * 2)(3, 0), img=(C.c_void_p * 2)(img.data_ptr(), None), u=(C.c_void_p * 2)(uv.data_ptr(), None),
                    v=(C.c_void_p * 2)(uv.data_ptr(), None), out=(C.c_void_p * 2)(out.data_ptr(), None))
    assert rc == capi.MLD_OK, text
    est.synchronize()
    lib.mld_labels_destroy(lb)


def test_calls_queued_through_one_set_of_host_tables(est):
    """Three calls back to back through ONE set of host pointer tables that is rewritten between the calls, each with
    its own images, features and outputs, one synchronisation at the end: the tables are consumed before a call returns."""
    import torch
    dev = torch.device("cuda:0")
    S, ns, rows, cols = 3, (300, 0, 77), 37, 53
    rng = np.random.default_rng(77)
    lib = capi.load()
    sl = SemanticLabels(est, S)
    t_img, t_u, t_v, t_lab, t_vot = ((C.c_void_p * S)() for _ in range(5))
    t_n = (C.c_int64 * S)()
    keep, want = [], []
    rois = [(5, 5), (50, 50), (6, 4)]
    for call in range(3):
        imgs = [make_image(rng, rows, cols, 5) for _ in range(S)]
        feats = [make_features(rng, rows, cols, n, call) for n in ns]
        d_imgs = [device_image(im, 53, dev) for im in imgs]
        d_u = [torch.from_numpy(np.ascontiguousarray(f[:, 0])).to(dev) for f in feats]
        d_v = [torch.from_numpy(np.ascontiguousarray(f[:, 1])).to(dev) for f in feats]
        lab, vot = outputs(ns, dev)
        keep.append((d_imgs, d_u, d_v, lab, vot))
        want.append([assign_labels(imgs[s], rois[call], feats[s][:, 0], feats[s][:, 1]) for s in range(S)])
    torch.cuda.synchronize()
    for call in range(3):
        d_imgs, d_u, d_v, lab, vot = keep[call]
        for s in range(S):
            t_img[s], t_u[s], t_v[s] = d_imgs[s].data_ptr(), d_u[s].data_ptr(), d_v[s].data_ptr()
            t_lab[s], t_vot[s], t_n[s] = lab[s].data_ptr(), vot[s].data_ptr(), ns[s]
        rc = lib.mld_labels_assign_device(sl._lb, t_img, rows, cols, 53, rois[call][0], rois[call][1], t_u, t_v, t_n, t_lab, t_vot)
        assert rc == capi.MLD_OK, lib.mld_labels_last_error(sl._lb).decode()
        for s in range(S):  # (what a caller that reuses its tables does next; the values must not matter any more)
            t_img[s] = t_u[s] = t_v[s] = t_lab[s] = t_vot[s] = None
            t_n[s] = 0
    est.synchronize()
    for call in range(3):
        check(ns, want[call], keep[call][3], keep[call][4], "all")
    sl.close()


def test_calls_queued_past_the_last_generation_of_the_descriptor_ring(est):
    """35 calls (twice the 16 pinned generations of the descriptor ring and three more) with no synchronisation in
    between, through ONE set of host pointer tables rewritten after every call: every generation's event is waited for
    and recorded again, and every call's labels and votes equal the restatement.  33 tracks cross a wavefront, one
    sequence is empty; (5, 5) takes the row kernel, (6, 4) the wavefront kernel, (0, 0) has no pixel in any window."""
    import torch
    dev = torch.device("cuda:0")
    S, ns, rows, cols, calls = 3, (33, 0, 2), 9, 11, 2 * 16 + 3
    rois = [(5, 5), (6, 4), (0, 0)]
    rng = np.random.default_rng(1635)
    lib = capi.load()
    sl = SemanticLabels(est, S)
    t_img, t_u, t_v, t_lab, t_vot = ((C.c_void_p * S)() for _ in range(5))
    t_n = (C.c_int64 * S)()
    keep, want = [], []
    for call in range(calls):
        imgs = [make_image(rng, rows, cols, 5) for _ in range(S)]
        feats = [make_features(rng, rows, cols, n, call) for n in ns]
        d_imgs = [device_image(im, 11, dev) for im in imgs]
        d_u = [torch.from_numpy(np.ascontiguousarray(f[:, 0])).to(dev) for f in feats]
        d_v = [torch.from_numpy(np.ascontiguousarray(f[:, 1])).to(dev) for f in feats]
        lab, vot = outputs(ns, dev)
        keep.append((d_imgs, d_u, d_v, lab, vot))
        want.append([assign_labels(imgs[s], rois[call % 3], feats[s][:, 0], feats[s][:, 1]) for s in range(S)])
    torch.cuda.synchronize()
    for call in range(calls):
        d_imgs, d_u, d_v, lab, vot = keep[call]
        roi = rois[call % 3]
        for s in range(S):
            t_img[s], t_u[s], t_v[s] = d_imgs[s].data_ptr(), d_u[s].data_ptr(), d_v[s].data_ptr()
            t_lab[s], t_vot[s], t_n[s] = lab[s].data_ptr(), vot[s].data_ptr(), ns[s]
        rc = lib.mld_labels_assign_device(sl._lb, t_img, rows, cols, 11, roi[0], roi[1], t_u, t_v, t_n, t_lab, t_vot)
        assert rc == capi.MLD_OK, lib.mld_labels_last_error(sl._lb).decode()
        for s in range(S):
            t_img[s] = t_u[s] = t_v[s] = t_lab[s] = t_vot[s] = None
            t_n[s] = 0
    est.synchronize()
    for call in range(calls):
        check(ns, want[call], keep[call][3], keep[call][4], "all")
    assert sum(int((w[0] != NO_LABEL).sum()) for per in want for w in per) > 100
    sl.close()


SCANNERS =(synth.Scanner(64, 1024, 2.0, -24.9), synth.VLP16)  # the first two of tests/test_tracklets_step_gpu.py
N_TRACKS = (500, 257)
H = 6


def _mask_of(inl, n, dev):
    import torch
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return torch.from_numpy(m.view(np.int32)).to(dev)


def test_labels_behind_the_tracklet_step():
    """Two frames of two sequences through TrackletBatch.step with a store, TrackletBatch.labels queued behind each step:
    (a) equal to the restatement on the raw u_new / v_new, (b) equal to SemanticLabels.assign on entry 0 of the exported
    histories (the store keeps (float)(int)u: the same pixel), and the step's depths, types and histories bit-equal
    to a second batch that makes no label call."""
    import torch
    from test_track_store_gpu import bits, churn
    dev = torch.device("cuda:0")
    P, cam, S = capi.params_c0(), kitti_camera(), len(SCANNERS)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(43)
    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, max(N_TRACKS))
    tb_plain = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, max(N_TRACKS))
    store, store_plain = tb.attach_store(H), tb_plain.attach_store(H)
    tb.attach_labels()
    again = SemanticLabels(tb.est, S)
    roi = (5, 5)
    prev, next_id = [np.zeros(0, np.int32)] * S, [0] * S
    for f in range(2):
        per, imgs = [], []
        for s in range(S):
            cloud = synth.make_cloud(SCANNERS[s], seed=90 + s, frame=2 * f)
            coeffs, inl = synth.make_ground_plane(cloud)
            n = N_TRACKS[s] - f
            ids, next_id[s] = churn(rng, prev[s], n, 0.3, next_id[s])
            u0 = rng.uniform(-2, cam.width + 2, n).astype(np.float32)
            v0 = rng.uniform(100, cam.height + 2, n).astype(np.float32)
            u1 = (u0 + rng.normal(0, 3, n)).astype(np.float32)
            v1 = (v0 + rng.normal(0, 2, n)).astype(np.float32)
            per.append((cloud, coeffs, inl, ids, u0, v0, u1, v1))
            prev[s] = ids
            imgs.append(make_image(rng, cam.height, cam.width, 5))
        ns = [len(p[3]) for p in per]
        clouds = [to(p[0]) for p in per]
        masks = [_mask_of(p[2], p[0].shape[0], dev) for p in per]
        coeffs = np.stack([p[1] for p in per])
        feats = [[to(p[k]) for p in per] for k in (4, 5, 6, 7)]
        ids = [to(p[3]) for p in per]
        d_imgs = [to(im) for im in imgs]

        def step_outputs():
            return ([torch.empty(n, dtype=torch.float32, device=dev) for n in ns],
                    [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in ns],
                    [torch.empty(n, dtype=torch.int32, device=dev) for n in ns],
                    [torch.zeros(n, dtype=torch.int32, device=dev) for n in ns])
        o, o_plain = step_outputs(), step_outputs()
        table = tb.prepare_step(clouds, coeffs, masks, ids, *feats, *o)
        table_plain = tb_plain.prepare_step(clouds, coeffs, masks, ids, *feats, *o_plain)
        lab, vot = outputs(ns, dev)
        lab2, vot2 = outputs(ns, dev)
        fp, fp_plain = ([torch.full((n, H, 3), -54321.0, dtype=torch.float32, device=dev) for n in ns] for _ in range(2))
        ln, ln_plain = ([torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns] for _ in range(2))
        torch.cuda.synchronize()
        tb.step(table)
        tb.labels(table, d_imgs, roi, [t[:n] for t, n in zip(lab, ns)], [t[:n] for t, n in zip(vot, ns)])
        store.export(fp, ln)
        tb_plain.step(table_plain)
        store_plain.export(fp_plain, ln_plain)
        tb.est.synchronize()
        tb_plain.est.synchronize()
        newest = [(fp[s][:, 0, 0].contiguous(), fp[s][:, 0, 1].contiguous()) for s in range(S)]
        torch.cuda.synchronize()
        again.assign(d_imgs, roi, [x[0] for x in newest], [x[1] for x in newest], [t[:n] for t, n in zip(lab2, ns)],
                     [t[:n] for t, n in zip(vot2, ns)])
        tb.est.synchronize()
        want = [assign_labels(imgs[s], roi, per[s][4], per[s][5]) for s in range(S)]
        check(ns, want, lab, vot, "all")   # (a)
        check(ns, want, lab2, vot2, "all")  # (b)
        assert sum(int((w[0] != NO_LABEL).sum()) for w in want) > 300
        for s in range(S):
            for a, b in zip(o, o_plain):
                x, y = a[s].cpu().numpy(), b[s].cpu().numpy()
                assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y), s
            assert np.array_equal(ln[s].cpu().numpy(), ln_plain[s].cpu().numpy()), s
            assert np.array_equal(bits(fp[s].cpu().numpy()), bits(fp_plain[s].cpu().numpy())), s
        assert (o[0][0].cpu().numpy() > 0).sum() > 20  # (the step did find depths)
    again.close()
    tb.close()
    tb_plain.close()
