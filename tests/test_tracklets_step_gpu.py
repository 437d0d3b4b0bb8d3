"""mld_tracklets_step_device end to end (TrackletBatch.step): ids + features in, depths + histories out.

Three sequences with scanners of different size, four frames, at most 500 tracks, 30 % new per frame.  The depths and
result types must be bit-equal to TrackletBatch.run on a second context that is fed the same frames with a HOST-made
new-track mask (the path the step call wraps), and the exported histories equal to the dict-of-lists restatement of
tracklet_depth_module.cpp:23-61, :119-193, :209-259 (tests/test_track_store_gpu.py) fed those depths.
"""
import numpy as np
import pytest

from mono_lidar_depth_amd import TrackletBatch, capi, synth

from helpers import kitti_camera
from test_track_store_gpu import SENTINEL, Restatement, bits, churn

pytestmark = pytest.mark.gpu

SCANNERS = (synth.Scanner(64, 1024, 2.0, -24.9), synth.VLP16, synth.HDL64_KITTI)  # 65 536 / 28 800 / 120 000 points
N_TRACKS = (500, 257, 64)
H = 6


def _mask_of(inl, n, dev):
    import torch
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return torch.from_numpy(m.view(np.int32)).to(dev)


@pytest.fixture(scope="module")
def frames():
    """Four frames of every sequence on the host, made once: cloud, plane, ids, features."""
    cam = kitti_camera()
    rng = np.random.default_rng(41)
    S = len(SCANNERS)
    prev, next_id, out = [np.zeros(0, np.int32)] * S, [0] * S, []
    for f in range(4):
        per = []
        for s in range(S):
            cloud = synth.make_cloud(SCANNERS[s], seed=90 + s, frame=2 * f)
            assert cloud.shape[0] > 4096
            coeffs, inl = synth.make_ground_plane(cloud)
            n = N_TRACKS[s] - (f if s == 1 else 0)  # (a ragged count that changes from frame to frame)
            ids, next_id[s] = churn(rng, prev[s], n, 0.3, next_id[s])
            u0 = rng.uniform(-2, cam.width + 2, n).astype(np.float32)
            v0 = rng.uniform(100, cam.height + 2, n).astype(np.float32)
            u1 = (u0 + rng.normal(0, 3, n)).astype(np.float32)
            v1 = (v0 + rng.normal(0, 2, n)).astype(np.float32)
            per.append((cloud, coeffs, inl, ids, u0, v0, u1, v1))
            prev[s] = ids
        out.append(per)
    return out


def _run_both(frames, first_frame_has_last):
    """The frames through step() on one context and through run() with a host-made mask on another.  With
    `first_frame_has_last` the sequence starts one frame earlier on both (a warm-up frame without tracks), so that the
    first frame with tracks already has a previous cloud."""
    import torch
    dev = torch.device("cuda:0")
    P, cam, S = capi.params_c0(), kitti_camera(), len(SCANNERS)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tb_step = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, max(N_TRACKS))
    tb_run = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, max(N_TRACKS))
    store = tb_step.attach_store(H)
    ref = [Restatement(H) for _ in range(S)]
    known = [set() for _ in range(S)]
    results = []
    seq = list(frames)
    if first_frame_has_last:
        empty = np.zeros(0, np.float32)
        seq.insert(0, [(c, co, inl, np.zeros(0, np.int32), empty, empty, empty, empty) for c, co, inl, *_ in frames[-1]])
    for per in seq:
        ns = [len(p[3]) for p in per]
        clouds = [to(p[0]) for p in per]
        masks = [_mask_of(p[2], p[0].shape[0], dev) for p in per]
        coeffs = np.stack([p[1] for p in per])
        feats = [[to(p[k]) for p in per] for k in (4, 5, 6, 7)]
        ids = [to(p[3]) for p in per]
        is_new_host = [np.array([int(i) not in known[s] for i in per[s][3]], dtype=np.uint8) for s in range(S)]

        def outputs():
            return ([torch.empty(n, dtype=torch.float32, device=dev) for n in ns],
                    [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in ns],
                    [torch.empty(n, dtype=torch.int32, device=dev) for n in ns],
                    [torch.zeros(n, dtype=torch.int32, device=dev) for n in ns])
        o_step, o_run = outputs(), outputs()
        f_step = tb_step.prepare_step(clouds, coeffs, masks, ids, *feats, *o_step)
        f_run = tb_run.prepare(clouds, coeffs, masks, *feats, [to(m) for m in is_new_host], *o_run)
        torch.cuda.synchronize()
        tb_step.step(f_step)
        tb_run.run(f_run)
        fp = [torch.full((n, H, 3), float(SENTINEL), dtype=torch.float32, device=dev) for n in ns]
        ln = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
        torch.cuda.synchronize()
        store.export(fp, ln)
        counts = store.counts()
        tb_run.est.synchronize()
        frame_res = []
        for s in range(S):
            got = [t[s].cpu().numpy() for t in o_step]
            want = [t[s].cpu().numpy() for t in o_run]
            new = is_new_host[s].astype(bool)
            # bit-equal depths and types; d_last / type_last are written only where the track is new
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[2], want[2]), s
            assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[3], want[3]), s
            assert np.isnan(got[1][~new]).all() and not np.isnan(got[1][new]).any()
            p = per[s]
            ref[s].commit(p[3], p[4], p[5], p[6], p[7], want[0], want[1])
            e_len, e_fp = ref[s].export()
            assert np.array_equal(ln[s].cpu().numpy(), e_len), s
            assert np.array_equal(bits(fp[s].cpu().numpy()), bits(e_fp)), s
            assert counts[s].tolist() == ref[s].counts, s
            assert counts[s, 1] == new.sum()
            known[s] = set(int(i) for i in p[3])
            frame_res.append((got, new, fp[s].cpu().numpy(), ln[s].cpu().numpy()))
        results.append(frame_res)
    tb_step.close()
    tb_run.close()
    return results


@pytest.fixture(scope="module")
def four_frames(frames):
    """The four frames through both paths, compared frame by frame inside _run_both; run once for the module."""
    return _run_both(frames, first_frame_has_last=False)


def test_step_equals_run_with_a_host_mask_and_keeps_the_histories(four_frames):
    # (every comparison with run() and with the restatement happened in _run_both)  later frames: 30 % new, depths were
    # found on both frames, the histories grew by one entry per frame
    for got, new, fp, ln in four_frames[3]:
        assert 0 < new.sum() < len(new)
        assert ln.max() == min(5, H) and ln.min() == 2
    got, new = four_frames[3][0][0], four_frames[3][0][1]
    assert (got[0] > 0).sum() > 50 and (got[1][new] > 0).sum() > 5


def test_first_frame_without_a_previous_cloud_stores_minus_one(four_frames):
    """have_last == 0 on the first frame: every track is new, and its second entry - the previous feature, for which
    there is no cloud yet - holds depth -1 (tracklet_depth_module.cpp:93-96)."""
    for got, new, fp, ln in four_frames[0]:
        assert new.all() and (ln == 2).all()
        assert (got[1] == -1).all() and (fp[:, 1, 2] == -1).all()
        assert not (fp[:, 0, 2] == SENTINEL).any()


def test_step_with_a_previous_cloud_on_the_first_tracks(frames):
    """The same sequences one frame later in their life: a frame without tracks came first, so the first frame WITH
    tracks has have_last == 1 and the new tracks' second entries are real depths of the previous cloud, not -1."""
    results = _run_both(frames[:2], first_frame_has_last=True)
    assert all(len(r[3]) == 0 for r in results[0])
    found = 0
    for got, new, fp, ln in results[1]:
        assert new.all() and (ln == 2).all()
        assert np.array_equal(bits(fp[:, 1, 2]), bits(got[1]))
        found += int((got[1] > 0).sum())
    assert found > 20
