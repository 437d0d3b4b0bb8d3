"""The GPU-resident tracklet store (mld_tracks_*) alone, with synthetic depths: after every frame the new-track masks,
the exported histories (lengths, and every entry below the length bit for bit; nothing written beyond it) and the
counters are compared with `Restatement`, a dict-of-lists restatement of tracklet_depth_module.cpp:23-61
(ExractNewTrackletFrames), :119-193 (SaveFeatureDepths, TidyUpTracklets) and :209-259
(convert_tracklets_to_matches_msg) plus the store's one deviation, the `max_history` cap.

The shapes are the smallest at which each thing can go wrong: more than one 256-thread block per sequence, ragged
counts with empty and one-track sequences, a sequence count that is no multiple of anything, a full table.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimator, TrackletStore, capi, synth

from helpers import kitti_camera

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-54321.0)  # what the export buffers hold before the call


class Restatement:
    """`_trackletMap` of ONE sequence: id -> list of (u, v, d), newest first."""

    def __init__(self, max_history):
        self.H = int(max_history)
        self.map = {}
        self.order = []     # the ids of the last committed frame, message order
        self.counts = [0] * 6

    def begin(self, ids):
        return np.array([int(i) not in self.map for i in ids], dtype=np.uint8)  # `_trackletMap.count(id)`, :31

    def commit(self, ids, u_new, v_new, u_old, v_old, d_cur, d_last):
        trunc = lambda a: np.asarray(a, dtype=np.float32).astype(np.int32).astype(np.float32)  # noqa: E731  pair<int,int>, :237
        un, vn, uo, vo = trunc(u_new), trunc(v_new), trunc(u_old), trunc(v_old)
        updated, n_new, n_old, n_dup = {}, 0, 0, 0
        for i, tid in enumerate(int(t) for t in ids):
            if tid in updated:   # a repeated id: removed (the store keeps one occurrence, unspecified which)
                n_dup += 1
                continue
            hist = self.map.get(tid)
            if hist is None:     # :134-151
                hist = [(uo[i], vo[i], np.float32(d_last[i]))]
                n_new += 1
            else:
                n_old += 1
            hist.insert(0, (un[i], vn[i], np.float32(d_cur[i])))  # :154-160
            del hist[self.H:]    # the store's cap; the reference's deque is unbounded
            updated[tid] = hist
        self.map = updated       # TidyUpTracklets: tracks without an update are erased (:171-193)
        self.order = [int(t) for t in ids]
        ok = sum(1 for h in updated.values() for e in h if e[2] >= 0)      # :235
        total = sum(len(h) for h in updated.values())
        self.counts = [len(updated), n_new, n_old, ok, total - ok, n_dup]

    def export(self):
        """(lengths [n], entries [n, H, 3] with SENTINEL beyond the length) in the order of the last frame."""
        n = len(self.order)
        lens = np.zeros(n, dtype=np.int32)
        fp = np.full((n, self.H, 3), SENTINEL, dtype=np.float32)
        for i, tid in enumerate(self.order):
            h = self.map[tid]
            lens[i] = len(h)
            fp[i, :len(h)] = np.array(h, dtype=np.float32).reshape(len(h), 3)
        return lens, fp


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Harness:
    """A store of S sequences beside S restatements; frame() runs one frame through both and compares everything."""

    def __init__(self, n_seq, max_tracks, max_history, seed=0):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.est = DepthEstimator(device=0, max_frames=1)
        self.est.InitConfig(capi.params_c0())
        self.est.Initialize(kitti_camera(), synth.T_CAM_LIDAR)
        self.S, self.M, self.H = n_seq, max_tracks, max_history
        self.store = TrackletStore(self.est, n_seq, max_tracks, max_history)
        self.ref = [Restatement(max_history) for _ in range(n_seq)]
        self.rng = np.random.default_rng(seed)
        self.hold = []

    def close(self):
        self.est.synchronize()
        self.store.close()
        self.est.close()

    def features(self, n):
        """Pixel coordinates with fractions (negative ones too: truncation is toward zero) and depths of which a fifth
        failed (-1) and a few are NaN."""
        rng = self.rng
        u_new, u_old = rng.uniform(-3, 1245, n).astype(np.float32), rng.uniform(-3, 1245, n).astype(np.float32)
        v_new, v_old = rng.uniform(-3, 378, n).astype(np.float32), rng.uniform(-3, 378, n).astype(np.float32)
        d_cur, d_last = rng.uniform(0, 80, n).astype(np.float32), rng.uniform(0, 80, n).astype(np.float32)
        for d in (d_cur, d_last):
            d[rng.random(n) < 0.2] = -1.0
            d[rng.random(n) < 0.02] = np.nan
        return u_new, v_new, u_old, v_old, d_cur, d_last

    def to(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def upload(self, ids):
        """Device tensors of one frame: (ids, is_new, six feature arrays) per sequence, and the host copies."""
        torch = self.torch
        host = [self.features(len(i)) for i in ids]
        t_ids = [self.to(np.asarray(i, dtype=np.int32)) for i in ids]
        t_new = [torch.full((len(i),), 7, dtype=torch.uint8, device=self.dev) for i in ids]
        t_feat = [[self.to(h[k]) for h in host] for k in range(6)]
        torch.cuda.synchronize()
        return host, t_ids, t_new, t_feat

    def check_export_and_counts(self, skip_ids=()):
        torch = self.torch
        ns = [len(r.order) for r in self.ref]
        fp = [torch.full((n, self.H, 3), float(SENTINEL), dtype=torch.float32, device=self.dev) for n in ns]
        ln = [torch.full((n,), -9, dtype=torch.int32, device=self.dev) for n in ns]
        torch.cuda.synchronize()
        self.store.export(fp, ln)
        counts = self.store.counts()  # (synchronises)
        for s, r in enumerate(self.ref):
            e_len, e_fp = r.export()
            g_len, g_fp = ln[s].cpu().numpy(), fp[s].cpu().numpy()
            keep = np.array([t not in skip_ids for t in r.order], dtype=bool)
            assert np.array_equal(g_len[keep], e_len[keep]), f"sequence {s}: lengths differ"
            # entries below the length bit-equal, entries at or beyond it untouched (the restatement holds SENTINEL there)
            assert np.array_equal(bits(g_fp[keep]), bits(e_fp[keep])), f"sequence {s}: histories differ"
            if not skip_ids:
                assert counts[s].tolist() == r.counts, f"sequence {s}: counts {counts[s].tolist()} != {r.counts}"
        return counts

    def frame(self, ids, skip_ids=(), check=True):
        """ids: S arrays of int32 ids.  Returns the store's counts of the frame."""
        host, t_ids, t_new, t_feat = self.upload(ids)
        self.store.begin(t_ids, t_new)
        self.store.commit(*t_feat)
        self.hold = (t_ids, t_new, t_feat)
        exp_new = [r.begin(i) for r, i in zip(self.ref, ids)]
        for r, i, h in zip(self.ref, ids, host):
            r.commit(i, *h)
        self.est.synchronize()  # (the frame's tensors may be dropped by the next frame from here on)
        if not check:
            return None
        for s in range(self.S):
            got = t_new[s].cpu().numpy()
            keep = np.array([int(t) not in skip_ids for t in ids[s]], dtype=bool)
            assert np.array_equal(got[keep], exp_new[s][keep]), f"sequence {s}: is_new differs"
        return self.check_export_and_counts(skip_ids)


def churn(rng, prev, n, new_frac, next_id):
    """n ids: (1 - new_frac) of them survivors of `prev` (as many as there are), the rest fresh; shuffled."""
    n_keep = min(len(prev), n - int(round(n * new_frac)))
    ids = np.concatenate([rng.choice(prev, n_keep, replace=False) if n_keep else np.zeros(0, np.int64),
                          np.arange(next_id, next_id + n - n_keep)]).astype(np.int64)
    rng.shuffle(ids)
    return ids.astype(np.int32), next_id + n - n_keep


@pytest.mark.parametrize("n_seq", [1, 13])
def test_basic_churn(n_seq):
    """Ragged track counts in 0 .. 600 (always a sequence with no track and one with a single track when there are
    several), 12 frames, 30 % new per frame."""
    h = Harness(n_seq, 600, 8, seed=n_seq)
    rng = np.random.default_rng(100 + n_seq)
    prev = [np.zeros(0, np.int32)] * n_seq
    next_id = [1000 * s for s in range(n_seq)]  # (the same id in two sequences means two tracks)
    for frame in range(12):
        ids = []
        for s in range(n_seq):
            n = int(rng.integers(0, 601))
            if n_seq > 1:
                n = {(frame + 2) % n_seq: 0, (frame + 5) % n_seq: 1, 3: 600}.get(s, n)
            else:
                n = (600, 257, 0, 1, 300, 600)[frame % 6]
            i, next_id[s] = churn(rng, prev[s], n, 0.3, next_id[s])
            ids.append(i)
        counts = h.frame(ids)
        assert counts[:, 5].sum() == 0
        prev = ids
    h.close()


def test_history_wraps_at_max_history():
    """max_history 4, tracks alive for 11 frames: the length saturates at 4 and the newest four are kept in order; a
    track that joins later has length 2 with d_last second."""
    import torch
    h = Harness(2, 300, 4, seed=5)
    ids = [np.arange(300, dtype=np.int32), np.arange(7, 7 + 261, dtype=np.int32)]
    for frame in range(11):
        if frame == 10:  # one late joiner per sequence
            ids = [np.concatenate([i[:-1], np.array([9999], np.int32)]) for i in ids]
        h.frame(ids)
        lens, fp = h.ref[0].export()
        assert (lens[:-1] == min(frame + 2, 4)).all()
    lens, fp = h.ref[1].export()
    assert lens[-1] == 2 and (lens[:-1] == 4).all()
    # the restatement is what the store was compared with; pin its own meaning on the device data once more
    out = [torch.zeros((len(i), 4, 3), dtype=torch.float32, device=h.dev) for i in ids]
    ln = [torch.zeros(len(i), dtype=torch.int32, device=h.dev) for i in ids]
    torch.cuda.synchronize()
    h.store.export(out, ln)
    h.est.synchronize()
    t_feat = h.hold[2]
    newest = out[1][:, 0, :].cpu().numpy()
    assert np.array_equal(newest[:, 0], np.trunc(t_feat[0][1].cpu().numpy()))      # (int)u_new
    assert np.array_equal(bits(newest[:, 2]), bits(t_feat[4][1].cpu().numpy()))    # d_cur
    second = out[1][-1, 1, :].cpu().numpy()
    assert second[1] == np.trunc(t_feat[3][1][-1].item())                          # (int)v_old of the joiner
    assert np.array_equal(bits(second[2:3]), bits(t_feat[5][1][-1:].cpu().numpy()))  # d_last
    h.close()


def test_extremes_of_churn():
    """First frame (all new), a frame where every track survives (reordered), a frame where none does."""
    h = Harness(3, 520, 6, seed=9)
    rng = np.random.default_rng(9)
    a = [np.arange(0, 520, dtype=np.int32), np.arange(0, 300, dtype=np.int32), np.arange(50, 51, dtype=np.int32)]
    c = h.frame(a)
    assert c[:, 1].tolist() == [520, 300, 1] and c[:, 2].tolist() == [0, 0, 0]
    b = [rng.permutation(i).astype(np.int32) for i in a]
    c = h.frame(b)
    assert c[:, 1].tolist() == [0, 0, 0] and c[:, 2].tolist() == [520, 300, 1]
    d = [i + 100000 for i in b]
    c = h.frame(d)
    assert c[:, 1].tolist() == [520, 300, 1] and c[:, 0].tolist() == [520, 300, 1]
    c = h.frame([np.zeros(0, np.int32)] * 3)  # and a frame without tracks: everything is erased
    assert c.sum() == 0
    c = h.frame(a)
    assert c[:, 1].tolist() == [520, 300, 1]
    h.close()


def test_pool_does_not_leak():
    """n_tracks == max_tracks = 257 with every track replaced every frame for 40 frames (a pool that lost one row per
    frame, or handed rows out before it took the ended tracks' back, would run dry), then 5 frames without churn."""
    h = Harness(2, 257, 4, seed=11)
    for frame in range(40):
        base = 1000 * frame
        ids = [np.arange(base, base + 257, dtype=np.int32), np.arange(base + 5, base + 262, dtype=np.int32)[::-1].copy()]
        c = h.frame(ids, check=frame % 8 == 7 or frame == 39)
        if c is not None:
            assert c[:, 0].tolist() == [257, 257] and c[:, 1].tolist() == [257, 257]
    for frame in range(5):
        c = h.frame(ids)
        assert c[:, 2].tolist() == [257, 257] and c[:, 1].tolist() == [0, 0]
    h.close()


def id_sets(rng):
    wrap = lambda a: (np.asarray(a, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # noqa: E731
    return {"shift16": wrap(np.arange(600) << 16), "shift20": wrap(np.arange(600) << 20),
            "consecutive": np.arange(-300, 300, dtype=np.int32),
            "random": rng.choice(np.arange(-2**31, 2**31, 2**20), 600, replace=False).astype(np.int64).astype(np.int32)
            + rng.integers(0, 2**20, 600).astype(np.int32)}


def test_every_int32_is_an_id():
    """0, -1, INT32_MIN and INT32_MAX in one frame, found again in the next and told apart."""
    h = Harness(1, 8, 4, seed=13)
    special = np.array([0, -1, -2**31, 2**31 - 1], dtype=np.int32)
    c = h.frame([special])
    assert c[0, 1] == 4
    c = h.frame([special[::-1].copy()])
    assert c[0, 2] == 4 and c[0, 1] == 0
    c = h.frame([np.array([0, 2**31 - 1, 1, -2], dtype=np.int32)])
    assert c[0, 2] == 2 and c[0, 1] == 2
    h.close()


def test_probe_chains():
    """600 ids i << 16, 600 ids i << 20 (wrapped to int32), 600 consecutive, 600 random: whatever the hash, some of
    these share table positions.  One set per sequence, three frames with half of each set replaced by ids of the
    same pattern."""
    sets = id_sets(np.random.default_rng(17))
    names = list(sets)
    h = Harness(len(names), 700, 4, seed=17)
    for k in range(len(names)):
        assert len(set(sets[names[k]].tolist())) == 600
    h.frame([sets[n] for n in names])
    rng = np.random.default_rng(18)
    for frame in range(3):
        ids = []
        for n in names:
            cur = sets[n]
            keep = rng.choice(cur, 300, replace=False)
            step = {"shift16": 1 << 16, "shift20": 1 << 20}.get(n, 1)
            pool = np.setdiff1d(((np.arange(-3000, 3000, dtype=np.int64) * step + 2**31) % 2**32 - 2**31).astype(np.int32), cur)
            sets[n] = np.concatenate([keep, rng.choice(pool, 300, replace=False)]).astype(np.int32)
            rng.shuffle(sets[n])
            ids.append(sets[n])
        c = h.frame(ids)
        assert c[:, 2].tolist() == [300] * 4 and c[:, 1].tolist() == [300] * 4
    h.close()


def test_table_full():
    """n_tracks == max_tracks with every id set: the tables hold as many ids as they are built for."""
    sets = id_sets(np.random.default_rng(19))
    names = list(sets)
    h = Harness(len(names), 600, 4, seed=19)
    c = h.frame([sets[n] for n in names])
    assert c[:, 0].tolist() == [600] * 4
    c = h.frame([sets[n][::-1].copy() for n in names])
    assert c[:, 2].tolist() == [600] * 4
    c = h.frame([sets[names[(k + 1) % 4]] for k in range(4)])  # every sequence takes its neighbour's set
    assert c[:, 0].tolist() == [600] * 4
    h.close()


def test_duplicate_ids_are_counted_and_harmless():
    """One id twice in a frame: one duplicate counted, the live count as without the repeat, every other id exact in
    that frame and the next (which occurrence of the repeated id is stored is unspecified: it is not compared)."""
    h = Harness(2, 400, 4, seed=23)
    rng = np.random.default_rng(23)
    first = [np.arange(0, 300, dtype=np.int32), np.arange(0, 300, dtype=np.int32)]
    h.frame(first)
    # sequence 0 repeats a known id (42), sequence 1 repeats a new one (777), far apart in the frame
    others = np.setdiff1d(np.arange(0, 298, dtype=np.int32), [42])
    ids0 = np.concatenate([[42], rng.permutation(others), [42]]).astype(np.int32)
    ids1 = np.concatenate([[777], np.arange(100, 398, dtype=np.int32), [777]]).astype(np.int32)
    h.frame([ids0, ids1], skip_ids=(42, 777))
    counts = h.store.counts()
    assert counts[:, 5].tolist() == [1, 1]
    assert counts[:, 0].tolist() == [h.ref[0].counts[0], h.ref[1].counts[0]] == [298, 299]
    assert counts[0, 1:3].tolist() == h.ref[0].counts[1:3] and counts[1, 1:3].tolist() == h.ref[1].counts[1:3]
    # the next frame: both repeated ids are known tracks now; everything else is exact, and no row was lost - the
    # sequences fill up to max_tracks afterwards
    nxt = [np.concatenate([[42], np.arange(100, 250, dtype=np.int32)]).astype(np.int32),
           np.concatenate([[777], np.arange(300, 398, dtype=np.int32)]).astype(np.int32)]
    h.frame(nxt, skip_ids=(42, 777))
    counts = h.store.counts()
    assert counts[:, 5].tolist() == [0, 0] and counts[:, 1].tolist() == [0, 0]
    assert counts[:, 2].tolist() == [151, 99]
    full = [np.arange(5000, 5400, dtype=np.int32)] * 2
    c = h.frame(full)
    assert c[:, 0].tolist() == [400, 400]
    c = h.frame([i + 1000 for i in full])
    assert c[:, 1].tolist() == [400, 400]
    h.close()


def test_frames_enqueued_ahead_equal_frames_run_one_by_one():
    """Six frames begun and committed without any synchronisation through ONE set of host tables that is overwritten
    after every call, then one export - equal to the same frames with a synchronise after each."""
    import torch
    S, M, H, frames = 3, 500, 5, 6
    rng = np.random.default_rng(29)
    feeder = Harness(S, M, H, seed=29)  # (its store stays unused: it only makes and uploads the frames)
    plan, prev, next_id = [], [np.zeros(0, np.int32)] * S, [0, 0, 0]
    for f in range(frames):
        ids = []
        for s in range(S):
            i, next_id[s] = churn(rng, prev[s], (500, 300 + 37 * f, 1 + f)[s], 0.3, next_id[s])
            ids.append(i)
        plan.append((ids,) + feeder.upload(ids))
        prev = ids
    lib = capi.load()

    def run(wait):
        h = Harness(S, M, H, seed=1)
        tr = h.store._tr
        tab = [(C.c_void_p * S)() for _ in range(8)]
        nt = (C.c_int64 * S)()
        for ids, host, t_ids, t_new, t_feat in plan:
            for s in range(S):
                tab[0][s], tab[1][s], nt[s] = t_ids[s].data_ptr(), t_new[s].data_ptr(), len(ids[s])
                for k in range(6):
                    tab[2 + k][s] = t_feat[k][s].data_ptr()
            assert lib.mld_tracks_begin_device(tr, tab[0], nt, tab[1]) == 0
            for s in range(S):  # the host tables are consumed when the call returns
                tab[0][s], tab[1][s], nt[s] = None, None, 0
            assert lib.mld_tracks_commit_device(tr, *tab[2:8]) == 0
            for k in range(6):
                for s in range(S):
                    tab[2 + k][s] = None
            if wait:
                h.est.synchronize()
        ns = [len(i) for i in plan[-1][0]]
        fp = [torch.full((n, H, 3), float(SENTINEL), dtype=torch.float32, device=h.dev) for n in ns]
        ln = [torch.full((n,), -9, dtype=torch.int32, device=h.dev) for n in ns]
        torch.cuda.synchronize()
        h.store.export(fp, ln)
        counts = h.store.counts()
        res = ([t.cpu().numpy() for t in fp], [t.cpu().numpy() for t in ln], counts, [t.cpu().numpy() for t in plan[-1][3]])
        h.close()
        return res

    ahead, stepwise = run(False), run(True)
    for s in range(S):
        assert np.array_equal(bits(ahead[0][s]), bits(stepwise[0][s])) and np.array_equal(ahead[1][s], stepwise[1][s])
        assert np.array_equal(ahead[3][s], stepwise[3][s])
    assert np.array_equal(ahead[2], stepwise[2])
    # and both are right: the restatement over the same frames
    ref = [Restatement(H) for _ in range(S)]
    for ids, host, *_ in plan:
        for s in range(S):
            ref[s].commit(ids[s], *host[s])
    for s in range(S):
        e_len, e_fp = ref[s].export()
        assert np.array_equal(ahead[1][s], e_len) and np.array_equal(bits(ahead[0][s]), bits(e_fp))
        assert ahead[2][s].tolist() == ref[s].counts
    feeder.close()


def test_frames_enqueued_past_the_last_generation_of_the_descriptor_ring():
    """20 frames begun and committed (40 descriptor uploads: twice the 16 pinned generations of the ring and more) with
    no synchronisation, through ONE set of host tables overwritten after every call, then one export and the counts:
    every generation's event is waited for and recorded again, and the masks of every frame, the histories and the
    counts equal the restatement.  33 tracks cross a wavefront; the second sequence is empty on every third frame."""
    import torch
    S, M, H, frames = 3, 40, 4, 20
    rng = np.random.default_rng(41)
    h = Harness(S, M, H, seed=41)
    plan, prev, next_id = [], [np.zeros(0, np.int32)] * S, [0, 0, 0]
    for f in range(frames):
        ids = []
        for s in range(S):
            i, next_id[s] = churn(rng, prev[s], (33, 7 * (f % 3), 1 + f % 2)[s], 0.3, next_id[s])
            ids.append(i)
        plan.append((ids,) + h.upload(ids))
        prev = ids
    lib = capi.load()
    tr = h.store._tr
    tab = [(C.c_void_p * S)() for _ in range(8)]
    nt = (C.c_int64 * S)()
    for ids, host, t_ids, t_new, t_feat in plan:
        for s in range(S):
            tab[0][s], tab[1][s], nt[s] = t_ids[s].data_ptr(), t_new[s].data_ptr(), len(ids[s])
            for k in range(6):
                tab[2 + k][s] = t_feat[k][s].data_ptr()
        assert lib.mld_tracks_begin_device(tr, tab[0], nt, tab[1]) == 0
        for s in range(S):  # the host tables are consumed when the call returns
            tab[0][s], tab[1][s], nt[s] = None, None, 0
        assert lib.mld_tracks_commit_device(tr, *tab[2:8]) == 0
        for k in range(6):
            for s in range(S):
                tab[2 + k][s] = None
    ns = [len(i) for i in plan[-1][0]]
    fp = [torch.full((n, H, 3), float(SENTINEL), dtype=torch.float32, device=h.dev) for n in ns]
    ln = [torch.full((n,), -9, dtype=torch.int32, device=h.dev) for n in ns]
    torch.cuda.synchronize()
    h.store.export(fp, ln)
    counts = h.store.counts()  # (synchronises)
    ref = [Restatement(H) for _ in range(S)]
    for ids, host, t_ids, t_new, t_feat in plan:
        for s in range(S):
            assert np.array_equal(t_new[s].cpu().numpy(), ref[s].begin(ids[s])), s
            ref[s].commit(ids[s], *host[s])
    for s in range(S):
        e_len, e_fp = ref[s].export()
        assert np.array_equal(ln[s].cpu().numpy(), e_len) and np.array_equal(bits(fp[s].cpu().numpy()), bits(e_fp)), s
        assert counts[s].tolist() == ref[s].counts, s
    h.close()


def test_capacity_and_call_order_are_checked():
    import torch
    from mono_lidar_depth_amd import DepthEstimatorError
    h = Harness(1, 16, 2, seed=31)
    ids = [torch.arange(17, dtype=torch.int32, device=h.dev)]
    with pytest.raises(DepthEstimatorError) as e:
        h.store.begin(ids)
    assert e.value.code == capi.MLD_ERR_CAPACITY
    f = [[torch.zeros(16, dtype=torch.float32, device=h.dev)] for _ in range(6)]
    with pytest.raises(DepthEstimatorError) as e:
        h.store.commit(*f)
    assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED
    c = h.frame([np.arange(16, dtype=np.int32)])  # the refused calls left the store usable
    assert c[0].tolist()[:3] == [16, 16, 0]
    h.close()
