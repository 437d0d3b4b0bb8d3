"""Lanes of a TrackletBatch that start, restart and resume independently (mld_tracklets_step_lanes_device,
mld_tracklets_depths_lanes_device, TrackletBatch.step / run with `restart`, set_previous, TrackletStore.import_packed).

Scanners, camera and track counts as in test_tracklets_step_gpu.py (clouds of 28 800 points and more, at most 500
tracks, max_history 6).  The oracle is the product's existing path: every recording alone through a TrackletBatch of ONE
sequence with the scalar step (its histories checked against the dict-of-lists restatement); a lane that runs the
recording inside a batch - after another recording, after frames without tracks, or resumed on another context from a
packed export - must give the same bits: depths, d_last, both type arrays, exports and counts.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import TrackletBatch, capi, synth

from helpers import kitti_camera
from test_track_store_gpu import SENTINEL, Restatement, bits, churn
from test_tracklets_step_gpu import H, SCANNERS, _mask_of

pytestmark = pytest.mark.gpu

# name: (scanner, tracks, frames, first id, cloud seed).  B's ids overlap A's.
RECORDINGS = {"R": (SCANNERS[0], 500, 6, 0, 70), "A": (SCANNERS[1], 257, 5, 0, 71), "B": (SCANNERS[2], 64, 3, 100, 72),
              "C": (SCANNERS[1], 300, 4, 5000, 73)}
KEYS = ("d_cur", "d_last", "t_cur", "t_last", "fp", "len", "counts")


def _empty(frame):
    """The frame's cloud and plane without tracks."""
    z = np.zeros(0, np.float32)
    return frame[:3] + (np.zeros(0, np.int32), z, z, z, z)


@pytest.fixture(scope="module")
def recordings():
    """Every recording on the host, made once: per frame (cloud, coeffs, inliers, ids, u_new, v_new, u_old, v_old)."""
    cam = kitti_camera()
    rng = np.random.default_rng(43)
    out = {}
    for name, (scanner, n, frames, first_id, seed) in RECORDINGS.items():
        prev, next_id, rec = np.zeros(0, np.int32), first_id, []
        for f in range(frames):
            cloud = synth.make_cloud(scanner, seed=seed, frame=2 * f)
            coeffs, inl = synth.make_ground_plane(cloud)
            ids, next_id = churn(rng, prev, n - f, 0.3, next_id)  # (a count that changes from frame to frame)
            u0 = rng.uniform(-2, cam.width + 2, len(ids)).astype(np.float32)
            v0 = rng.uniform(100, cam.height + 2, len(ids)).astype(np.float32)
            u1 = (u0 + rng.normal(0, 3, len(ids))).astype(np.float32)
            v1 = (v0 + rng.normal(0, 2, len(ids))).astype(np.float32)
            rec.append((cloud, coeffs, inl, ids, u0, v0, u1, v1))
            prev = ids
        out[name] = rec
    assert set(out["A"][2][3].tolist()) & set(out["B"][0][3].tolist())
    return out


def _batch(n_seq, store=True):
    tb = TrackletBatch(capi.params_c0(), kitti_camera(), synth.T_CAM_LIDAR, n_seq, 500)
    if store:
        tb.attach_store(H)
    return tb


def _frame(tb, per, restart=None, is_new=None, call=None):
    """One frame of every lane: step() (is_new None) or run() with the host-made masks `is_new`; `call`: a function that
    makes the tracklet call itself in place of step().  Returns per lane the outputs and, with a store, export and
    counts."""
    import torch
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ns = [len(p[3]) for p in per]
    clouds = [to(p[0]) for p in per]
    masks = [_mask_of(p[2], p[0].shape[0], dev) for p in per]
    coeffs = np.stack([p[1] for p in per])
    feats = [[to(p[k]) for p in per] for k in (4, 5, 6, 7)]
    outs = ([torch.empty(n, dtype=torch.float32, device=dev) for n in ns],
            [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in ns],
            [torch.empty(n, dtype=torch.int32, device=dev) for n in ns],
            [torch.zeros(n, dtype=torch.int32, device=dev) for n in ns])
    if is_new is None:
        f = tb.prepare_step(clouds, coeffs, masks, [to(p[3]) for p in per], *feats, *outs)
    else:
        f = tb.prepare(clouds, coeffs, masks, *feats, [to(m) for m in is_new], *outs)
    torch.cuda.synchronize()
    if call is not None:
        call(tb, f)
    elif is_new is None:
        tb.step(f, restart=restart)
    else:
        tb.run(f, restart=restart)
    res = [dict(zip(KEYS, (t[s] for t in outs))) for s in range(tb.S)]
    if tb.store is not None:
        fp = [torch.full((n, H, 3), float(SENTINEL), dtype=torch.float32, device=dev) for n in ns]
        ln = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
        torch.cuda.synchronize()
        tb.store.export(fp, ln)
        counts = tb.store.counts()
        for s in range(tb.S):
            res[s].update(fp=fp[s], len=ln[s], counts=counts[s])
    tb.est.synchronize()
    return [{k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()} for r in res]


def _same(got, want, what, keys=KEYS):
    for k in keys:
        a, b = got[k], want[k]
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b), (what, k)


@pytest.fixture(scope="module")
def solo(recordings):
    """Every recording alone: a TrackletBatch of one sequence, the scalar step; histories and counts are checked against
    the restatement fed the depths of the run."""
    out = {}
    for name, rec in recordings.items():
        tb, ref, frames = _batch(1), Restatement(H), []
        for p in rec:
            r = _frame(tb, [p])[0]
            ref.commit(p[3], p[4], p[5], p[6], p[7], r["d_cur"], r["d_last"])
            e_len, e_fp = ref.export()
            assert np.array_equal(r["len"], e_len) and np.array_equal(bits(r["fp"]), bits(e_fp)), name
            assert r["counts"].tolist() == ref.counts, name
            frames.append(r)
        tb.close()
        assert (frames[0]["d_last"] == -1).all()  # no previous cloud yet (tracklet_depth_module.cpp:93-96)
        if name == "R":  # later frames found depths on the previous cloud (500 tracks on 65 536 points)
            assert (frames[1]["d_last"] > 0).sum() > 5
        out[name] = frames
    return out


def _schedule(recordings):
    """Six frames of three lanes: lane 0 runs R throughout; lane 1 runs A for frames 0-2 and starts B at frame 3; lane 2
    carries no tracks for frames 0-1 and starts C at frame 2.  Per frame: (frames of the lanes, restart flags, what
    each lane shows: (recording, frame) or None)."""
    R, A, B, Cr = (recordings[k] for k in "RABC")
    plan = []
    for f in range(6):
        lane1 = (A[f], ("A", f)) if f < 3 else (B[f - 3], ("B", f - 3))
        lane2 = (_empty(Cr[0]), None) if f < 2 else (Cr[f - 2], ("C", f - 2))
        plan.append(([R[f], lane1[0], lane2[0]], [0, int(f == 3), int(f == 2)], [("R", f), lane1[1], lane2[1]]))
    return plan


@pytest.fixture(scope="module")
def restarted(recordings):
    """The schedule through step() with `restart`, run once."""
    tb, out = _batch(3), []
    for per, restart, _ in _schedule(recordings):
        out.append(_frame(tb, per, restart=restart if any(restart) else None))
    assert tb.lane_has_last == [True] * 3
    tb.close()
    return out


def test_lanes_restart_independently(recordings, solo, restarted):
    """Every recording in its lane equals its solo run bit for bit, whatever the lane held before."""
    for (per, restart, shows), lanes in zip(_schedule(recordings), restarted):
        for s, show in enumerate(shows):
            if show is None:
                assert lanes[s]["counts"].tolist() == [0] * 6
                continue
            _same(lanes[s], solo[show[0]][show[1]], (show, s))
    b0 = restarted[3][1]  # B's first frame, in the lane A ran in a frame ago: every id is new, no previous frame is used
    assert b0["counts"][1] == len(b0["d_last"]) and (b0["d_last"] == -1).all() and (b0["fp"][:, 1, 2] == -1).all()
    assert (b0["t_last"] == restarted[0][0]["t_last"][0]).all()  # (MLD_Unspecified, as on a batch's first frame)
    c0 = restarted[2][2]
    assert (c0["d_last"] == -1).all() and (c0["len"] == 2).all()


def test_run_with_a_host_mask_and_restart_equals_step(recordings, restarted):
    """run() with masks made on the host (the caller keeps the maps, and forgets a lane's on its restart) and the same
    `restart` gives step()'s depths and types."""
    tb = _batch(3, store=False)
    known = [set() for _ in range(3)]
    for (per, restart, _), want in zip(_schedule(recordings), restarted):
        for s in range(3):
            if restart[s]:
                known[s] = set()
        is_new = [np.array([int(i) not in known[s] for i in per[s][3]], dtype=np.uint8) for s in range(3)]
        got = _frame(tb, per, restart=restart if any(restart) else None, is_new=is_new)
        for s in range(3):
            _same(got[s], want[s], s, keys=KEYS[:4])
            known[s] = set(int(i) for i in per[s][3])
    tb.close()


def test_resume_on_another_context(recordings, solo):
    """A runs frames 0-2 in one batch, is exported (packed export + ids) and imported into lane 0 of a NEW two-lane batch;
    set_previous gives that lane frame 2's cloud and plane.  Frames 3-4 equal the uninterrupted solo run; lane 1 starts B
    with `restart` beside it."""
    import torch
    dev = torch.device("cuda:0")
    A, B = recordings["A"], recordings["B"]
    first = _batch(1)
    for p in A[:3]:
        _frame(first, [p])
    n = len(A[2][3])
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    fp = torch.zeros((first.store.packed_capacity(n), 3), dtype=torch.float32, device=dev)
    ids = torch.from_numpy(A[2][3]).to(dev)
    torch.cuda.synchronize()
    first.store.export_packed([fp], [off])
    first.est.synchronize()
    total = int(off[-1])
    tb = _batch(2)
    tb.store.import_packed([ids, None], [off, None], [fp[:total], None], select=[1, 0])
    tb.set_previous(0, torch.from_numpy(A[2][0]).to(dev), A[2][1], _mask_of(A[2][2], A[2][0].shape[0], dev))
    assert tb.lane_has_last == [True, False] and not tb.have_last
    first.close()  # (the source and its context are gone before the resumed lane steps)
    for k in range(2):
        got = _frame(tb, [A[3 + k], B[k]], restart=[0, 1] if k == 0 else None)
        _same(got[0], solo["A"][3 + k], ("A", 3 + k))
        _same(got[1], solo["B"][k], ("B", k))
    assert got[0]["len"].max() == 6
    tb.close()


def test_the_scalar_call_and_the_lanes_call_with_equal_flags_agree(recordings):
    """mld_tracklets_step_device and mld_tracklets_step_lanes_device with a uniform have_last and restart = NULL on the
    same four frames, through the C entries."""
    lib = capi.load()

    def lanes_call(tb, f):
        S, est = tb.S, tb.est
        est._check(lib.mld_set_clouds_planes_range_device(est._ctx, tb.bank * S, S, f["clouds"], f["n"], 16,
                                                          f["coeffs"].ctypes.data_as(C.POINTER(C.c_float)), f["masks"]))
        flags = (C.c_uint8 * S)(*[1 if tb.have_last else 0] * S)
        tb.store._check(lib.mld_tracklets_step_lanes_device(est._ctx, tb.store._tr, tb.bank, flags, None, f["ids"], f["u_new"],
                                                            f["v_new"], f["u_old"], f["v_old"], f["nt"], f["d_cur"],
                                                            f["d_last"], f["t_cur"], f["t_last"]))
        tb._keep = (tb._keep[1] if tb._keep else None, f)
        tb.bank = 1 - tb.bank
        tb.have_last = True

    scalar, lanes = _batch(3), _batch(3)
    for f in range(4):
        per = [recordings["R"][f], recordings["A"][f], recordings["C"][f]]
        want = _frame(scalar, per)
        got = _frame(lanes, per, call=lanes_call)
        for s in range(3):
            _same(got[s], want[s], (f, s))
    scalar.close()
    lanes.close()
