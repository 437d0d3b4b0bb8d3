"""mld_tracks_import_packed_device / mld_tracks_reset_device on the store alone, with the harness of
test_track_store_gpu.py (synthetic depths, -1 and NaN among them) and the restatement of track_import_restatement.py.

S = 5 sequences of (600, 0, 1, 257, 300) tracks in a store of max_tracks 600 and max_history 6: more than two blocks of
256 tracks, none, one, one past a block, and n == max_tracks.  Three frames with 30 % churn come first, so that the
histories hold 2 .. 4 entries and the ring heads are not 0.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimatorError, capi

from test_track_store_gpu import SENTINEL, Harness, bits, churn
from track_import_restatement import ImportRestatement, synthetic_features

pytestmark = pytest.mark.gpu

S, M, H = 5, 600, 6
COUNTS = (600, 0, 1, 257, 300)
TAIL = np.float32(777.25)  # what fp holds beyond n_entries in the bounds test


def harness(max_tracks=M, max_history=H, n_seq=S, seed=0):
    h = Harness(n_seq, max_tracks, max_history, seed=seed)
    h.ref = [ImportRestatement(max_history) for _ in range(n_seq)]
    return h


def entries(rng, n):
    """n (u, v, d) entries as an export holds them - here with fractions, which an import must keep bit for bit."""
    f = synthetic_features(rng, n)
    return np.ascontiguousarray(np.stack([f[0], f[1], f[4]], axis=1))


class Plan:
    """Frames made once on the host: ids with 30 % churn and the six feature arrays per sequence."""

    def __init__(self, seed, counts=COUNTS):
        self.rng = np.random.default_rng(seed)
        self.counts = list(counts)
        self.prev = [np.zeros(0, np.int32)] * len(counts)
        self.next_id = [1000 * s for s in range(len(counts))]

    def frame(self):
        ids = []
        for s, n in enumerate(self.counts):
            i, self.next_id[s] = churn(self.rng, self.prev[s], n, 0.3, self.next_id[s])
            ids.append(i)
        self.prev = ids
        return ids, [synthetic_features(self.rng, len(i)) for i in ids]


def run_frame(h, ids, host, skip_ids=()):
    """One planned frame through a store and its restatements; masks, exports (fixed stride and packed) and counts are
    compared with the restatement.  Returns (masks, state) for comparisons between stores."""
    torch = h.torch
    t_ids = [h.to(np.asarray(i, dtype=np.int32)) for i in ids]
    t_new = [torch.full((len(i),), 7, dtype=torch.uint8, device=h.dev) for i in ids]
    t_feat = [[h.to(f[k]) for f in host] for k in range(6)]
    torch.cuda.synchronize()
    h.store.begin(t_ids, t_new)
    h.store.commit(*t_feat)
    h.hold = (t_ids, t_new, t_feat)
    exp_new = [r.begin(i) for r, i in zip(h.ref, ids)]
    for r, i, f in zip(h.ref, ids, host):
        r.commit(i, *f)
    h.est.synchronize()
    masks = [t.cpu().numpy() for t in t_new]
    for s in range(h.S):
        assert np.array_equal(masks[s], exp_new[s]), f"sequence {s}: is_new differs"
    return masks, state(h, skip_ids)


def state(h, skip_ids=()):
    """Fixed-stride export, packed export and counts of a store, each compared with its restatements."""
    torch = h.torch
    counts = h.check_export_and_counts(skip_ids)
    ns = [len(r.order) for r in h.ref]
    fp = [torch.full((n, h.H, 3), float(SENTINEL), dtype=torch.float32, device=h.dev) for n in ns]
    ln = [torch.full((n,), -9, dtype=torch.int32, device=h.dev) for n in ns]
    off = [torch.full((n + 1,), -9, dtype=torch.int64, device=h.dev) for n in ns]
    pk = [torch.full((h.store.packed_capacity(n), 3), float(SENTINEL), dtype=torch.float32, device=h.dev) for n in ns]
    torch.cuda.synchronize()
    h.store.export(fp, ln)
    h.store.export_packed(pk, off)
    h.est.synchronize()
    out = {"fp": [t.cpu().numpy() for t in fp], "len": [t.cpu().numpy() for t in ln], "off": [t.cpu().numpy() for t in off],
           "pk": [t.cpu().numpy() for t in pk], "counts": counts, "dev": (off, pk)}
    if not skip_ids:
        for s, r in enumerate(h.ref):
            e_off, e_pk = r.packed()
            if ns[s]:
                assert np.array_equal(out["off"][s], e_off), f"sequence {s}: offsets differ"
            assert np.array_equal(bits(out["pk"][s][:len(e_pk)]), bits(e_pk)), f"sequence {s}: packed entries differ"
            assert (out["pk"][s][len(e_pk):] == SENTINEL).all(), f"sequence {s}: written beyond the total"
    return out


def same(a, b, seqs, counts_columns=slice(None)):
    for s in seqs:
        for k in ("fp", "len", "off", "pk"):
            x, y = a[k][s], b[k][s]
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y), (k, s)
        assert np.array_equal(a["counts"][s, counts_columns], b["counts"][s, counts_columns]), s


def import_state(dst, ids, st, select=None):
    """The packed export `st` of a store (device tensors) with the ids of its frame into `dst` and its restatements."""
    off, pk = st["dev"]
    t_ids = [dst.to(np.asarray(i, dtype=np.int32)) for i in ids]
    dst.torch.cuda.synchronize()
    totals = [int(st["off"][s][-1]) if len(ids[s]) else 0 for s in range(dst.S)]
    fps = [pk[s][:totals[s]] for s in range(dst.S)]
    dst.store.import_packed(t_ids, off, fps, select)
    for s in range(dst.S):
        if select is None or select[s]:
            dst.ref[s].load(ids[s], st["off"][s] if len(ids[s]) else np.zeros(1, np.int64), st["pk"][s][:totals[s]])
    dst.est.synchronize()


@pytest.fixture(scope="module")
def source():
    """The source store after three frames, and its plan (a test that runs further frames through it advances store and
    plan together; a test that needs the state takes it afresh)."""
    h = harness(seed=1)
    plan = Plan(7)
    for _ in range(3):
        ids, host = plan.frame()
        _, st = run_frame(h, ids, host)
    lens = np.concatenate(st["len"])
    assert lens.min() == 2 and lens.max() == 4
    yield h, plan
    h.close()


def test_round_trip_into_a_larger_store(source):
    """Packed export + ids into a store of max_tracks 700: both exports and the counts equal the source's and the
    restatement's (counts [1] / [2] are the import's: stored, 0), and two further frames through both stores agree."""
    src, plan = source
    st = state(src)
    dst = harness(max_tracks=700, seed=2)
    import_state(dst, plan.prev, st)
    got = state(dst)
    same(got, st, range(S), counts_columns=[0, 3, 4, 5])
    assert got["counts"][:, 1].tolist() == list(COUNTS) and got["counts"][:, 2].tolist() == [0] * S
    for _ in range(2):
        ids, host = plan.frame()
        m_src, st_src = run_frame(src, ids, host)
        m_dst, st_dst = run_frame(dst, ids, host)
        same(st_src, st_dst, range(S))
        assert all(np.array_equal(a, b) for a, b in zip(m_src, m_dst))
    assert np.concatenate(st_src["len"]).max() == 6
    dst.close()


def test_import_into_a_smaller_history(source):
    """max_history 3: the newest three entries of every track, and the frames that follow equal the restatement with
    cap 3 (run_frame compares)."""
    src, plan = source
    st = state(src)
    ids = plan.prev
    dst = harness(max_history=3, seed=3)
    import_state(dst, ids, st)
    got = state(dst)
    for s in range(S):
        keep = np.minimum(st["len"][s], 3)
        assert np.array_equal(got["len"][s], keep)
        for i in np.flatnonzero(st["len"][s] > 3)[:20]:
            assert np.array_equal(bits(got["fp"][s][i]), bits(st["fp"][s][i, :3]))
    follow = Plan(11)
    follow.prev, follow.next_id = list(ids), [50000 + 1000 * s for s in range(S)]
    for _ in range(2):
        run_frame(dst, *follow.frame())
    dst.close()


def test_select_leaves_the_other_sequences_alone():
    """Mid-run, sequences {1, 3} of one of two twin stores are imported into (3: no tracks).  Sequences 0, 2 and 4 stay
    bit-equal to the twin over the next two frames; every id of sequence 3 is new on the next frame, those it held
    before the import included."""
    a, b = harness(seed=4), harness(seed=5)
    plan = Plan(13)
    for _ in range(3):
        ids, host = plan.frame()
        run_frame(a, ids, host)
        _, st_b = run_frame(b, ids, host)
    held = plan.prev[3]
    # sequence 1 receives the 300 tracks of the twin's sequence 4; the tables of the others are NULL
    select = [0, 1, 0, 1, 0]
    ids_in = [None, plan.prev[4], None, np.zeros(0, np.int32), None]
    off, pk = st_b["dev"]
    total = int(st_b["off"][4][-1])
    a.store.import_packed([None, a.to(ids_in[1]), None, None, None], [None, off[4], None, None, None],
                          [None, pk[4][:total], None, None, None], select)
    a.ref[1].load(ids_in[1], st_b["off"][4], st_b["pk"][4][:total])
    a.ref[3].reset()
    got = state(a)
    same(got, st_b, (0, 2, 4))
    assert got["counts"][1].tolist()[:3] == [300, 300, 0] and got["counts"][3].tolist() == [0] * 6
    plan.counts[1], plan.prev[1] = 200, ids_in[1]
    for k in range(2):
        ids, host = plan.frame()
        m_a, st_a = run_frame(a, ids, host)
        m_b, st_b = run_frame(b, ids, host)
        same(st_a, st_b, (0, 2, 4))
        assert all(np.array_equal(m_a[s], m_b[s]) for s in (0, 2, 4))
        if k == 0:
            assert np.isin(ids[3], held).sum() > 100 and m_a[3].all() and not m_b[3].all()
            assert st_a["counts"][3, 1] == 257 and 0 < st_a["counts"][1, 2] <= 140
    a.close()
    b.close()


def test_the_pool_keeps_every_row():
    """600 tracks, 20 of them repeated ids, into the sequence with n == max_tracks; then three frames of 600 entirely new
    ids: 600 live tracks on every frame, every history the restatement's (a leaked or doubly freed row shows up as a
    smaller count or a foreign history)."""
    h = harness(seed=6)
    warm = Plan(17)
    for _ in range(2):  # (the import meets a pool and a table in use)
        run_frame(h, *warm.frame())
    rng = np.random.default_rng(19)
    ids0 = np.concatenate([np.arange(7000, 7580), rng.choice(np.arange(7000, 7580), 20, replace=False)]).astype(np.int32)
    lens = rng.integers(0, 7, 600)
    off0 = np.zeros(601, dtype=np.int64)
    off0[1:] = np.cumsum(lens)
    fp0 = entries(rng, int(off0[-1]))
    none = [None] * 4
    h.store.import_packed([h.to(ids0)] + none, [h.to(off0)] + none, [h.to(fp0)] + none, [1, 0, 0, 0, 0])
    h.ref[0].load(ids0, off0, fp0)
    repeated = set(ids0[580:].tolist())
    c = h.check_export_and_counts(skip_ids=repeated)
    assert c[0, [0, 1, 2, 5]].tolist() == [580, 580, 0, 20] == [h.ref[0].counts[k] for k in (0, 1, 2, 5)]
    for k in range(3):
        ids = [np.arange(9000 + 600 * k, 9600 + 600 * k, dtype=np.int32)] + [np.zeros(0, np.int32)] * 4
        _, got = run_frame(h, ids, [synthetic_features(rng, len(i)) for i in ids])
        assert got["counts"][0].tolist()[:3] == [600, 600, 0] and got["counts"][0, 5] == 0
    h.close()


def test_offsets_are_clamped_to_n_entries():
    """n_entries smaller than the last offset, a negative first offset and one decreasing pair; fp is of the full size and
    holds a distinctive value beyond n_entries, which appears in no export.  Lengths as the clamping rule gives."""
    h = harness(max_tracks=300, n_seq=1, seed=8)
    rng = np.random.default_rng(23)
    n = 300
    ids = np.arange(100, 100 + n, dtype=np.int32)
    lens = rng.integers(1, 7, n)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total, n_entries = int(off[-1]), int(off[260]) + 1  # (track 260 keeps one entry, the tracks behind it none)
    off[0] = -5
    off[51] = off[50] - 2  # track 50: no entries; track 51: from two entries in front of track 50's to its own end
    fp = entries(rng, total)
    fp[n_entries:] = TAIL
    t_fp = h.to(fp)
    h.store.import_packed([h.to(ids)], [h.to(off)], [t_fp[:n_entries]])
    h.ref[0].load(ids, off, fp, n_entries=n_entries)
    got = state(h)
    want = np.minimum(lens, H)
    want[50], want[51], want[260], want[261:] = 0, min(H, lens[50] + lens[51] + 2), 1, 0
    assert np.array_equal(got["len"][0], want)
    assert not (got["fp"][0] == TAIL).any() and not (got["pk"][0] == TAIL).any()
    assert got["counts"][0].tolist() == h.ref[0].counts
    # a track stored with length 0 takes the next commit's push like any other
    follow = Plan(29, counts=(n,))
    follow.prev, follow.next_id = [ids], [5000]
    _, got = run_frame(h, *follow.frame())
    assert got["len"][0].min() == 1
    h.close()


def test_repeated_ids_abandoned_frames_and_refusals():
    torch_ids = lambda h, a: h.to(np.asarray(a, dtype=np.int32))  # noqa: E731
    h = harness(max_tracks=300, n_seq=2, seed=9)
    rng = np.random.default_rng(31)
    # repeated ids: 42 twice in sequence 0, far apart and with different histories
    ids = [np.concatenate([[42], np.arange(1000, 1270), [42]]).astype(np.int32), np.arange(10, dtype=np.int32)]
    offs, fps = [], []
    for i in ids:
        lens = rng.integers(1, 7, len(i))
        offs.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        fps.append(entries(rng, int(offs[-1][-1])))
    h.store.import_packed([h.to(i) for i in ids], [h.to(o) for o in offs], [h.to(f) for f in fps])
    for s in range(2):
        h.ref[s].load(ids[s], offs[s], fps[s])
    c = h.check_export_and_counts(skip_ids=(42,))
    assert c[0, [0, 1, 2, 5]].tolist() == [271, 271, 0, 1] == [h.ref[0].counts[k] for k in (0, 1, 2, 5)]
    assert c[1].tolist() == h.ref[1].counts
    st = state(h, skip_ids=(42,))
    first, last = st["fp"][0][0], st["fp"][0][-1]
    assert st["len"][0][0] == st["len"][0][-1] and np.array_equal(bits(first), bits(last))  # both export the stored one
    stored = first[:st["len"][0][0]]
    occurrences = [fps[0][offs[0][i]:offs[0][i + 1]] for i in (0, len(ids[0]) - 1)]
    assert any(o.shape == stored.shape and np.array_equal(bits(o), bits(stored)) for o in occurrences)
    # a begun frame is abandoned by an import: the commit is refused
    feats = [[h.to(a) for a in (synthetic_features(rng, len(i))[k] for i in ids)] for k in range(6)]
    h.store.begin([h.to(i) for i in ids])
    three = [None, h.to(ids[1][:3])], [None, h.to(offs[1][:4])], [None, h.to(fps[1][:int(offs[1][3])])]
    h.store.import_packed(*three, select=[0, 1])  # (an import that carries tracks, into sequence 1 only)
    h.ref[1].load(ids[1][:3], offs[1][:4], fps[1])
    with pytest.raises(DepthEstimatorError) as e:
        h.store.commit(*feats)
    assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED
    state(h, skip_ids=(42,))
    h.store.begin([h.to(i) for i in ids])   # and by a reset, the import of no tracks
    h.store.reset([0, 1])
    h.ref[1].reset()
    with pytest.raises(DepthEstimatorError) as e:
        h.store.commit(*feats)
    assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED
    before = state(h, skip_ids=(42,))
    assert before["counts"][1].tolist() == [0] * 6
    # refusals, through the C entry; the store is unchanged afterwards
    lib, tr = capi.load(), h.store._tr
    t_ids, t_off, t_fp = h.to(ids[1]), h.to(offs[1]), h.to(fps[1])
    h.torch.cuda.synchronize()
    tab = lambda t: (C.c_void_p * 2)(None, t.data_ptr())  # noqa: E731
    cnt = lambda a, b: (C.c_int64 * 2)(a, b)  # noqa: E731
    sel = (C.c_uint8 * 2)(0, 1)
    ne = int(offs[1][-1])
    good = (sel, tab(t_ids), cnt(0, 10), tab(t_off), tab(t_fp), cnt(0, ne))
    call = lambda **kw: lib.mld_tracks_import_packed_device(tr, *[kw.get(k, g) for k, g in zip("sinofe", good)])  # noqa: E731
    assert call(n=cnt(0, 301)) == capi.MLD_ERR_CAPACITY
    assert call(n=cnt(0, -1)) == capi.MLD_ERR_INVALID_ARG
    assert call(e=cnt(0, -1)) == capi.MLD_ERR_INVALID_ARG
    assert call(i=None) == capi.MLD_ERR_INVALID_ARG and call(o=None) == capi.MLD_ERR_INVALID_ARG
    assert call(f=None) == capi.MLD_ERR_INVALID_ARG and call(e=None) == capi.MLD_ERR_INVALID_ARG
    assert call(n=None) == capi.MLD_ERR_INVALID_ARG
    nulls = (C.c_void_p * 2)(None, None)
    assert call(i=nulls) == capi.MLD_ERR_INVALID_ARG and call(o=nulls) == capi.MLD_ERR_INVALID_ARG
    assert call(f=nulls) == capi.MLD_ERR_INVALID_ARG
    assert call(s=None, n=cnt(5, 10)) == capi.MLD_ERR_INVALID_ARG  # (sequence 0 is selected now and has no arrays)
    after = state(h, skip_ids=(42,))
    same(before, after, range(2))
    assert call() == capi.MLD_OK  # the refused calls left the store usable
    h.ref[1].load(ids[1], offs[1], fps[1])
    state(h, skip_ids=(42,))
    h.close()
