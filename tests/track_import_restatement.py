"""The dict-of-lists restatement of the tracklet store (tests/test_track_store_gpu.py: `_trackletMap` of one sequence) with
what mld_tracks_import_packed_device and mld_tracks_reset_device add: load(ids, offsets, fp) replaces the map by given
tracks, reset() by none, packed() writes the map as mld_tracks_export_packed_device does.  The rules are the header's:
entries bit for bit, the newest `max_history` entries of a longer history, offsets clamped to the entries fp holds, a
decreasing pair of offsets a track without entries, one occurrence of a repeated id stored and the others counted,
counts = [stored, stored, 0, entries with d >= 0, the other entries, repeated ids].

self_test(): load() of the restatement's own packed export reproduces it (tests/test_track_import_cpu.py runs it).
"""
import numpy as np

from test_track_store_gpu import SENTINEL, Restatement, churn


class ImportRestatement(Restatement):
    def packed(self):
        """(offsets int64 [n + 1], entries float32 [total, 3]) of the last committed frame, message order; a repeated
        id exports the stored history at every occurrence."""
        lens = [len(self.map[t]) for t in self.order]
        offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lens)
        rows = [e for t in self.order for e in self.map[t]]
        fp = np.array(rows, dtype=np.float32).reshape(len(rows), 3)
        return offsets, fp

    def load(self, ids, offsets, fp, n_entries=None):
        """n_entries: the entries fp counts as holding (default: all).  Of a repeated id the first occurrence is stored
        here; the store leaves unspecified which one it keeps."""
        fp = np.asarray(fp, dtype=np.float32).reshape(-1, 3)
        E = fp.shape[0] if n_entries is None else int(n_entries)
        off = np.clip(np.asarray(offsets, dtype=np.int64), 0, E)
        loaded, n_dup = {}, 0
        for i, tid in enumerate(int(t) for t in ids):
            hist = [tuple(fp[e]) for e in range(off[i], max(off[i], off[i + 1]))][:self.H]
            if tid in loaded:
                n_dup += 1
                continue
            loaded[tid] = hist
        self.map = loaded
        self.order = [int(t) for t in ids]
        ok = sum(1 for h in loaded.values() for e in h if e[2] >= 0)
        total = sum(len(h) for h in loaded.values())
        self.counts = [len(loaded), len(loaded), 0, ok, total - ok, n_dup]

    def reset(self):
        self.load(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros((0, 3), np.float32))

    def export(self):
        """As Restatement.export(), for maps that may hold tracks without entries."""
        n = len(self.order)
        lens = np.zeros(n, dtype=np.int32)
        fp = np.full((n, self.H, 3), SENTINEL, dtype=np.float32)
        for i, tid in enumerate(self.order):
            h = self.map[tid]
            lens[i] = len(h)
            if h:
                fp[i, :len(h)] = np.array(h, dtype=np.float32).reshape(len(h), 3)
        return lens, fp


def synthetic_features(rng, n):
    """The features of test_track_store_gpu.Harness.features: fractions, a fifth of the depths -1, a few NaN."""
    u_new, u_old = rng.uniform(-3, 1245, n).astype(np.float32), rng.uniform(-3, 1245, n).astype(np.float32)
    v_new, v_old = rng.uniform(-3, 378, n).astype(np.float32), rng.uniform(-3, 378, n).astype(np.float32)
    d_cur, d_last = rng.uniform(0, 80, n).astype(np.float32), rng.uniform(0, 80, n).astype(np.float32)
    for d in (d_cur, d_last):
        d[rng.random(n) < 0.2] = -1.0
        d[rng.random(n) < 0.02] = np.nan
    return u_new, v_new, u_old, v_old, d_cur, d_last


def self_test():
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)  # noqa: E731
    rng = np.random.default_rng(3)
    src = ImportRestatement(6)
    prev, next_id = np.zeros(0, np.int32), 0
    for _ in range(4):
        ids, next_id = churn(rng, prev, 70, 0.3, next_id)
        src.commit(ids, *synthetic_features(rng, 70))
        prev = ids
    offsets, fp = src.packed()
    assert offsets[-1] == fp.shape[0] and set(np.diff(offsets).tolist()) == {2, 3, 4, 5}
    # the same cap: the copy is the source, counts but for (new, old) included; the next frame keeps them equal
    dst = ImportRestatement(6)
    dst.load(prev, offsets, fp)
    for a, b in zip(src.export(), dst.export()):
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
    po, pf = dst.packed()
    assert np.array_equal(po, offsets) and np.array_equal(bits(pf), bits(fp))
    assert dst.counts[0] == src.counts[0] == dst.counts[1] and dst.counts[2] == 0 and dst.counts[3:5] == src.counts[3:5]
    ids, next_id = churn(rng, prev, 64, 0.3, next_id)
    feats = synthetic_features(rng, 64)
    assert np.array_equal(src.begin(ids), dst.begin(ids))
    src.commit(ids, *feats)
    dst.commit(ids, *feats)
    assert src.counts == dst.counts and np.array_equal(bits(src.export()[1]), bits(dst.export()[1]))
    # a smaller cap keeps the newest entries; clamped and decreasing offsets; a repeated id; reset
    small = ImportRestatement(3)
    small.load(prev, offsets, fp)
    lens, hist = small.export()
    assert np.array_equal(lens, np.minimum(np.diff(offsets), 3))
    assert all(np.array_equal(bits(hist[i, :lens[i]]), bits(fp[offsets[i]:offsets[i] + lens[i]])) for i in range(len(prev)))
    cut = ImportRestatement(6)
    bad = offsets.copy()
    bad[5] = bad[4] - 1
    cut.load(prev, bad, fp, n_entries=int(offsets[40]))
    lens = cut.export()[0]
    assert lens[4] == 0 and (lens[40:] == 0).all() and lens[5] == min(6, offsets[6] - bad[5])
    twice = ImportRestatement(6)
    twice.load(np.concatenate([prev[:10], prev[:2]]), offsets[:13], fp)
    assert twice.counts[0] == 10 and twice.counts[5] == 2
    twice.reset()
    assert twice.counts == [0] * 6 and twice.begin(prev).all()
