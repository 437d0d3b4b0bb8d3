"""mld_tracks_export_leaving_device / mld_tracks_set_leaving_sink (TrackletStore.export_leaving, set_leaving_sink,
TrackletBatch.step(leaving=...)): the tracks a commit erases and the entries it overwrites.

The store alone is driven with synthetic depths (test_track_store_gpu.Harness: a fifth -1, a few NaN); only the last
tests run the step on a synthetic cloud.  After every begin the export is compared with the capped model of
track_leaving_restatement.py, over a run TrackArchive is compared with the unbounded model, and every ended track's
entries are compared with what export_packed gave for the same track one call earlier.  Everything is compared on bit
patterns; nothing here is arithmetic.  Every output buffer is longer than it is said to be and holds a sentinel behind
its capacity.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimatorError, TrackArchive, TrackletBatch, TrackletStore, capi, synth

from helpers import kitti_camera
from test_track_store_gpu import SENTINEL, Harness, bits, churn
from test_tracklets_step_gpu import _mask_of
from track_leaving_restatement import CappedStore, UnboundedMap, as_frame

pytestmark = pytest.mark.gpu

PAD = 5          # guard elements behind every capacity
GUARD_I = -9     # what the integer buffers hold before a call
SIZES = (1, 255, 256, 257, 600)  # a block of the kernels takes 256 tracks


class Buffers:
    """Output buffers of one leaving export with given capacities per sequence (None: what never truncates for
    `ns` committed tracks); every tensor is PAD elements longer than the store is told and pre-filled."""

    def __init__(self, h, ns, tcap=None, ecap=None, scap=None):
        torch = h.torch
        self.h, self.S = h, len(ns)
        self.tcap = [int(n) for n in ns] if tcap is None else list(tcap)
        self.ecap = [int(n) * h.H for n in ns] if ecap is None else list(ecap)
        self.scap = [int(n) for n in ns] if scap is None else list(scap)
        ints = lambda n, dt: torch.full((n + PAD,), GUARD_I, dtype=dt, device=h.dev)  # noqa: E731
        flts = lambda n: torch.full((n + PAD, 3), float(SENTINEL), dtype=torch.float32, device=h.dev)  # noqa: E731
        self.full = {"ids": [ints(c, torch.int32) for c in self.tcap], "offsets": [ints(c + 1, torch.int64) for c in self.tcap],
                     "fp": [flts(c) for c in self.ecap], "spill_ids": [ints(c, torch.int32) for c in self.scap],
                     "spill_fp": [flts(c) for c in self.scap]}
        self.record = torch.full((self.S, 4), GUARD_I, dtype=torch.int64, device=h.dev)

    def args(self):
        """The tensors the store sees: their sizes are the capacities."""
        f = self.full
        return {"ids": [t[:c] for t, c in zip(f["ids"], self.tcap)], "offsets": [t[:c + 1] for t, c in zip(f["offsets"], self.tcap)],
                "fp": [t[:c] for t, c in zip(f["fp"], self.ecap)], "spill_ids": [t[:c] for t, c in zip(f["spill_ids"], self.scap)],
                "spill_fp": [t[:c] for t, c in zip(f["spill_fp"], self.scap)], "record": self.record}

    def host(self):
        return TrackletStore.leaving_host(self.args())

    def untouched(self, s):
        return all((t[s].cpu().numpy() == GUARD_I).all() for t in (self.full["ids"], self.full["offsets"], self.full["spill_ids"])) and \
            all((bits(t[s].cpu().numpy()) == bits(SENTINEL)).all() for t in (self.full["fp"], self.full["spill_fp"]))

    def check(self, want, what, skip_ids=(), written=None):
        """want: per sequence the model's frame (as_frame), complete.  Compares the records, everything below the
        capacities and the guards at and beyond them.  skip_ids: ids whose place and entries are not compared (their
        presence and length are).  written: per sequence False where nothing at all may have been written."""
        rec = self.record.cpu().numpy()
        for s, w in enumerate(want):
            if written is not None and not written[s]:
                assert (rec[s] == GUARD_I).all() and self.untouched(s), f"{what}: sequence {s} was written"
                continue
            assert rec[s].tolist() == w["record"].tolist(), f"{what}: sequence {s}: record {rec[s].tolist()} != {w['record'].tolist()}"
            g = {k: t[s].cpu().numpy() for k, t in self.full.items()}
            n_t, n_e, n_p = (int(x) for x in w["record"][:3])
            t, e, p = min(n_t, self.tcap[s]), min(n_e, self.ecap[s]), min(n_p, self.scap[s])
            # (offsets[0 .. t] with a capacity > 0; a sequence without committed tracks gets nothing but its record)
            n_off = t + 1 if self.tcap[s] > 0 and len(self.h_order[s]) > 0 else 0
            if skip_ids:
                assert t == n_t and e == n_e and p == n_p  # (the tests that skip ids do not truncate)
                _same_but(g, w, skip_ids, f"{what}: sequence {s}")
            else:
                assert np.array_equal(g["ids"][:t], w["ids"][:t]), f"{what}: sequence {s}: ids differ"
                assert np.array_equal(g["offsets"][:n_off], w["offsets"][:n_off]), f"{what}: sequence {s}: offsets differ"
                assert np.array_equal(bits(g["fp"][:e]), bits(w["fp"][:e])), f"{what}: sequence {s}: entries differ"
                assert np.array_equal(g["spill_ids"][:p], w["spill_ids"][:p]), f"{what}: sequence {s}: spill ids differ"
                assert np.array_equal(bits(g["spill_fp"][:p]), bits(w["spill_fp"][:p])), f"{what}: sequence {s}: spilled entries differ"
            assert (g["ids"][t:] == GUARD_I).all() and (g["offsets"][n_off:] == GUARD_I).all(), f"{what}: sequence {s}: ids / offsets written beyond {t}"
            assert (bits(g["fp"][e:]) == bits(SENTINEL)).all(), f"{what}: sequence {s}: entries written at or beyond {e}"
            assert (g["spill_ids"][p:] == GUARD_I).all() and (bits(g["spill_fp"][p:]) == bits(SENTINEL)).all(), \
                f"{what}: sequence {s}: spills written at or beyond {p}"


def _tracks(f):
    return [(int(t), f["fp"][int(f["offsets"][k]):int(f["offsets"][k + 1])]) for k, t in enumerate(f["ids"])]


def _same_but(g, w, skip_ids, what):
    """Both streams equal the model's except for the place and the entries of `skip_ids` (repeated ids: which occurrence
    the store keeps is open)."""
    n_t, n_p = len(w["ids"]), len(w["spill_ids"])
    got = _tracks({"ids": g["ids"][:n_t], "offsets": g["offsets"][:n_t + 1], "fp": g["fp"]})
    want = _tracks(w)
    assert sorted(t for t, _ in got) == sorted(t for t, _ in want), f"{what}: ended ids differ"
    assert {t: len(e) for t, e in got} == {t: len(e) for t, e in want}, f"{what}: lengths differ"
    for (tg, eg), (tw, ew) in zip([x for x in got if x[0] not in skip_ids], [x for x in want if x[0] not in skip_ids]):
        assert tg == tw and np.array_equal(bits(eg), bits(ew)), f"{what}: track {tw} differs"
    sg = [(int(t), g["spill_fp"][k]) for k, t in enumerate(g["spill_ids"][:n_p])]
    sw = [(int(t), w["spill_fp"][k]) for k, t in enumerate(w["spill_ids"])]
    assert sorted(t for t, _ in sg) == sorted(t for t, _ in sw), f"{what}: spilled ids differ"
    for (tg, eg), (tw, ew) in zip([x for x in sg if x[0] not in skip_ids], [x for x in sw if x[0] not in skip_ids]):
        assert tg == tw and np.array_equal(bits(eg), bits(ew)), f"{what}: spill of {tw} differs"


class Run:
    """A store beside the capped and the unbounded model and a TrackArchive; frame() = begin, leaving export, commit."""

    def __init__(self, n_seq, max_tracks, max_history, seed):
        self.h = Harness(n_seq, max_tracks, max_history, seed=seed)
        self.S = n_seq
        self.capped = [CappedStore(max_history) for _ in range(n_seq)]
        self.full = [UnboundedMap() for _ in range(n_seq)]
        self.archive = TrackArchive(n_seq)
        self.n_spilled = self.n_full_ended = self.n_ended = 0
        self.skip = set()

    def close(self):
        self.h.close()

    def orders(self):
        return [c.order for c in self.capped]

    def packed(self):
        """export_packed of the committed frame on the host: per sequence (offsets, entries)."""
        h, torch = self.h, self.h.torch
        ns = [len(o) for o in self.orders()]
        off = [torch.zeros(n + 1, dtype=torch.int64, device=h.dev) for n in ns]
        fp = [torch.zeros((n * h.H, 3), dtype=torch.float32, device=h.dev) for n in ns]
        torch.cuda.synchronize()
        h.store.export_packed(fp, off)
        h.est.synchronize()
        return [(o.cpu().numpy(), f.cpu().numpy()) for o, f in zip(off, fp)]

    def begin(self, ids, decoy=None):
        """Uploads the frame and begins it (after a begin of `decoy`, if given, which is thereby abandoned)."""
        h = self.h
        host, t_ids, t_new, t_feat = h.upload(ids)
        if decoy is not None:
            d_ids = [h.to(np.asarray(i, dtype=np.int32)) for i in decoy]
            h.torch.cuda.synchronize()
            h.store.begin(d_ids, None)
            self.decoy_hold = d_ids
        h.store.begin(t_ids, t_new)
        self.pending = (ids, host, t_ids, t_new, t_feat)

    def want(self, ids, flush=None):
        return [as_frame(*c.leaving(i, flush=bool(flush and flush[s]))) for s, (c, i) in enumerate(zip(self.capped, ids))]

    def export(self, buf, flush=None):
        buf.h_order = self.orders()
        self.h.store.export_leaving(**buf.args(), flush=flush)

    def commit(self):
        ids, host, t_ids, t_new, t_feat = self.pending
        self.h.store.commit(*t_feat)
        self.h.est.synchronize()
        erased = []
        for s in range(self.S):
            self.capped[s].commit(ids[s], *host[s])
            erased.append(self.full[s].frame(ids[s], *host[s]))
        return erased

    def frame(self, ids, decoy=None, what=""):
        """One frame with every check: the export against the capped model and against the packed export of one call
        earlier, the archive against the unbounded model."""
        h = self.h
        before = self.packed()
        order = [list(o) for o in self.orders()]
        self.begin(ids, decoy)
        buf = Buffers(h, [len(o) for o in order])
        h.torch.cuda.synchronize()
        self.export(buf)
        want = self.want(ids)
        erased = self.commit()
        buf.check(want, what, skip_ids=self.skip)
        got = buf.host()
        for s in range(self.S):  # the ended tracks as the packed export wrote them one call earlier
            off, fp = before[s]
            place = {}
            for i, tid in enumerate(order[s]):
                place.setdefault(tid, i)
            for tid, e in _tracks(got[s]):
                i = place[tid]
                assert np.array_equal(bits(e), bits(fp[int(off[i]):int(off[i + 1])])), f"{what}: sequence {s}: track {tid} != packed export"
                self.n_full_ended += len(e) == h.H
            self.n_ended += len(got[s]["ids"])
            self.n_spilled += len(got[s]["spill_ids"])
        self.check_archive(self.archive.push(got), erased, what)

    def check_archive(self, done, erased, what):
        for s in range(self.S):
            got = {t.id: t.entries for t in done if t.sequence == s}
            assert sorted(got) == [k for k, _ in erased[s]], f"{what}: sequence {s}: the archive closed other tracks"
            for k, e in erased[s]:
                if k not in self.skip:
                    assert got[k].shape == e.shape and np.array_equal(bits(got[k]), bits(e)), f"{what}: sequence {s}: archived track {k}"
                else:
                    assert len(got[k]) == len(e)

    def finish(self):
        """The end of the recording: a flush of every sequence, no begun frame."""
        h = self.h
        buf = Buffers(h, [len(o) for o in self.orders()])
        h.torch.cuda.synchronize()
        self.export(buf, flush=[1] * self.S)
        h.est.synchronize()
        want = [as_frame(*c.leaving(flush=True)) for c in self.capped]
        buf.check(want, "flush of all", skip_ids=self.skip)
        got = buf.host()
        self.n_full_ended += sum(len(e) == h.H for g in got for _, e in _tracks(g))
        self.check_archive(self.archive.push(got), [f.end() for f in self.full], "end")
        assert all(not self.archive.open_tracks(s) for s in range(self.S))


def _ids(rng, prev, n, mode, next_id, immortal):
    """n ids: `mode` "same" (prev permuted), "fresh" (no survivor), else 30 % churn with the ids 0 .. immortal-1
    (as many as fit) always among them."""
    if mode == "same":
        return rng.permutation(prev).astype(np.int32), next_id
    if mode == "fresh":
        return np.arange(next_id, next_id + n, dtype=np.int32), next_id + n
    keep = np.arange(min(immortal, n))
    mortal_prev = np.array([t for t in prev if t >= immortal], dtype=np.int64)
    rest, next_id = churn(rng, mortal_prev, n - len(keep), 0.3, next_id)
    ids = np.concatenate([keep, rest]).astype(np.int64)
    rng.shuffle(ids)
    return ids.astype(np.int32), next_id


@pytest.mark.parametrize("max_history,frames,fresh_at", [(2, 8, 5), (3, 8, 5), (16, 20, 1)])
def test_churn_against_both_models(max_history, frames, fresh_at):
    """Three sequences, one of them without tracks; the other two walk through 1, 255, 256, 257 and 600 tracks.  Frame 3
    repeats the ids of frame 2 (none leave), frame `fresh_at` has no survivor (all leave), the others churn 30 % around
    7 ids that stay: tracks outlive max_history, full tracks end and full tracks spill."""
    r = Run(3, 600, max_history, seed=max_history)
    rng = np.random.default_rng(40 + max_history)
    prev, next_id = [np.zeros(0, np.int32)] * 3, [1000, 200000, 0]
    for f in range(frames):
        ids = []
        for s in range(3):
            mode = "same" if f == 3 else ("fresh" if f == fresh_at else "churn")
            n = 0 if s == 2 else (len(prev[s]) if f == 3 else SIZES[(f + 2 * s + (f > 3)) % 5])
            i, next_id[s] = _ids(rng, prev[s], n, mode, next_id[s], 7)
            ids.append(i)
        r.frame(ids, what=f"frame {f}")
        prev = ids
    r.finish()
    assert r.n_spilled > 0 and r.n_full_ended > 0 and r.n_ended > 600
    r.close()


def test_rows_recycle_when_max_tracks_is_the_frame():
    """max_tracks = the 300 tracks of every frame, max_history 3: every row that an ended track frees is taken again at
    once; frames without a survivor alternate with 50 % churn."""
    r = Run(2, 300, 3, seed=7)
    rng = np.random.default_rng(7)
    prev, next_id = [np.zeros(0, np.int32)] * 2, [0, 50000]
    for f in range(8):
        ids = []
        for s in range(2):
            if f % 2 == 1 and s == 0:
                i, next_id[s] = _ids(rng, prev[s], 300, "fresh", next_id[s], 0)
            else:
                i, next_id[s] = churn(rng, prev[s], 300, 0.5, next_id[s])
            ids.append(i)
        r.frame(ids, what=f"frame {f}")
        prev = ids
    assert r.n_spilled > 0
    r.finish()
    r.close()


def test_a_frame_begun_twice_follows_the_second_begin():
    """A begin of other ids stamps its marks and is abandoned by the second begin: the export follows the second."""
    r = Run(2, 600, 2, seed=11)
    a = [np.arange(0, 600, dtype=np.int32), np.arange(0, 257, dtype=np.int32)]
    r.frame(a, what="first")
    r.frame(a, what="second")  # (every track is full now)
    decoy = [np.arange(0, 300, dtype=np.int32), np.arange(100, 257, dtype=np.int32)]
    real = [np.arange(300, 900, dtype=np.int32), np.arange(0, 50, dtype=np.int32)]
    r.frame(real, decoy=decoy, what="begun twice")
    assert r.n_spilled == 300 + 50 + 600 + 257 and r.n_ended == 300 + 207
    r.finish()
    r.close()


def test_repeated_ids_in_the_committed_and_in_the_begun_frame():
    """Sequence 0 repeats a known id (42), sequence 1 a new one (777); the next frame repeats 42 again and 5 anew.  A
    repeated id stands once in the streams; where it stands and what its entries are depends on the occurrence the store
    kept, so for these ids presence and length are compared with the model and the entries with the packed export."""
    r = Run(2, 400, 2, seed=23)
    rng = np.random.default_rng(23)
    base = np.arange(0, 300, dtype=np.int32)
    r.frame([base, base], what="plain")
    r.skip = {42, 777, 5}
    others = np.setdiff1d(np.arange(0, 298, dtype=np.int32), [42])
    ids0 = np.concatenate([[42], rng.permutation(others), [42]]).astype(np.int32)
    ids1 = np.concatenate([[777], np.arange(100, 398, dtype=np.int32), [777]]).astype(np.int32)
    r.frame([ids0, ids1], what="repeated in the begun frame")
    assert r.h.store.counts()[:, 5].tolist() == [1, 1]
    nxt0 = np.concatenate([[5, 42], np.arange(150, 400, dtype=np.int32), [42, 5]]).astype(np.int32)  # 42 continues, full: it spills once
    nxt1 = np.arange(300, 500, dtype=np.int32)                                                       # 777 ends, once
    r.frame([nxt0, nxt1], what="repeated in the committed frame")
    r.frame([np.arange(0, 10, dtype=np.int32), np.arange(300, 310, dtype=np.int32)], what="after")
    r.finish()
    r.close()


def test_a_sequence_with_more_blocks_than_the_scan_is_wide():
    """66 000 tracks (258 blocks: the per-sequence scan takes a second pass of 256 block sums), max_history 2."""
    n = 66000
    assert (n + 255) // 256 > 256
    r = Run(1, n, 2, seed=17)
    rng = np.random.default_rng(17)
    ids, next_id = churn(rng, np.zeros(0, np.int32), n, 0.3, 0)
    r.frame([ids], what="first")
    ids, next_id = churn(rng, ids, n, 0.3, next_id)
    r.frame([ids], what="churn")  # (every committed track is full: 30 % end, 70 % spill)
    assert r.n_spilled == n - r.n_ended and r.n_ended == int(round(n * 0.3))
    r.close()


@pytest.fixture(scope="module")
def begun():
    """Three sequences (600, 0 and 257 tracks), max_history 3, six frames around 7 ids that stay, and a seventh frame
    begun and not committed: the leaving export is read-only, every test below reads this state."""
    r = Run(3, 600, 3, seed=29)
    rng = np.random.default_rng(29)
    sizes, prev, next_id = [600, 0, 257], [np.zeros(0, np.int32)] * 3, [1000, 0, 90000]
    for f in range(7):
        ids = []
        for s in range(3):
            i, next_id[s] = _ids(rng, prev[s], sizes[s], "churn", next_id[s], 7)
            ids.append(i)
        if f < 6:
            r.frame(ids, what=f"frame {f}")
        else:
            r.begin(ids)
        prev = ids
    want = r.want(ids)
    assert all(min(w["record"][:3]) > 7 for w in want[::2]) and want[1]["record"].tolist() == [0, 0, 0, 0]
    yield r, ids, want
    r.close()


@pytest.mark.parametrize("which", ["zero", "one", "count-1", "count", "count+3"])
def test_capacities_truncate_the_arrays_and_never_the_records(begun, which):
    r, ids, want = begun
    pick = lambda n: {"zero": 0, "one": 1, "count-1": max(n - 1, 0), "count": n, "count+3": n + 3}[which]  # noqa: E731
    buf = Buffers(r.h, [len(o) for o in r.orders()], tcap=[pick(int(w["record"][0])) for w in want],
                  ecap=[pick(int(w["record"][1])) for w in want], scap=[pick(int(w["record"][2])) for w in want])
    r.h.torch.cuda.synchronize()
    r.export(buf)
    r.h.est.synchronize()
    buf.check(want, f"capacity {which}")


def test_capacities_that_truncate_one_array_each(begun):
    """Only the tracks, only the entries, only the spills cut short: the other arrays are complete."""
    r, ids, want = begun
    ns = [len(o) for o in r.orders()]
    for k in range(3):
        caps = [[int(w["record"][j]) // 2 if j == k else int(w["record"][j]) for w in want] for j in range(3)]
        buf = Buffers(r.h, ns, *caps)
        r.h.torch.cuda.synchronize()
        r.export(buf)
        r.h.est.synchronize()
        buf.check(want, f"column {k} halved")


def test_flush_of_one_lane_beside_lanes_that_go_by_marks(begun):
    r, ids, want = begun
    flush = [0, 0, 1]
    buf = Buffers(r.h, [len(o) for o in r.orders()])
    r.h.torch.cuda.synchronize()
    r.export(buf, flush=flush)
    r.h.est.synchronize()
    mixed = r.want(ids, flush=flush)
    assert mixed[2]["record"].tolist()[::2] == [len(r.capped[2].stored()), 0] and mixed[0]["record"].tolist() == want[0]["record"].tolist()
    buf.check(mixed, "flush of lane 2")


def test_two_exports_queued_back_to_back(begun):
    """They share the scan scratch and the descriptor ring; the first one is truncated."""
    r, ids, want = begun
    ns = [len(o) for o in r.orders()]
    first = Buffers(r.h, ns, *[[int(w["record"][j]) // 3 for w in want] for j in range(3)])
    second = Buffers(r.h, ns)
    r.h.torch.cuda.synchronize()
    r.export(first)
    r.export(second, flush=[1, 0, 0])
    r.h.est.synchronize()
    first.check(want, "first of two")
    second.check(r.want(ids, flush=[1, 0, 0]), "second of two")


def test_refusals(begun):
    r, ids, want = begun
    h = r.h
    lib, tr, S = h.store._lib, h.store._tr, h.S
    buf = Buffers(h, [len(o) for o in r.orders()])
    buf.h_order = r.orders()
    a = buf.args()
    h.torch.cuda.synchronize()
    tab = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    cap = lambda v: (C.c_int64 * S)(*v)  # noqa: E731
    names = ("ids_out", "offsets_out", "fp_out", "spill_ids_out", "spill_fp_out", "track_capacity", "entry_capacity",
             "spill_capacity", "record_out_dev")

    def good():
        return [tab(a["ids"]), tab(a["offsets"]), tab(a["fp"]), tab(a["spill_ids"]), tab(a["spill_fp"]), cap(buf.tcap),
                cap(buf.ecap), cap(buf.scap), C.c_void_p(int(buf.record.data_ptr()))]

    def refused(fn, word, args, lead):
        assert getattr(lib, fn)(tr, *lead, *args) == capi.MLD_ERR_INVALID_ARG, (fn, word)
        text = lib.mld_tracks_last_error(tr).decode()
        assert fn in text and word in text, text

    assert lib.mld_tracks_export_leaving_device(None, None, *good()) == capi.MLD_ERR_INVALID_ARG
    for fn, lead in (("mld_tracks_export_leaving_device", [None]), ("mld_tracks_set_leaving_sink", [])):
        for k, name in enumerate(names):  # a null required table
            args = good()
            args[k] = None
            refused(fn, name, args, lead)
        for k in range(5):  # a null array where the capacity is > 0 and the sequence has tracks (sequence 2)
            args = good()
            args[k][2] = None
            refused(fn, names[k], args, lead)
        for k in (5, 6, 7):  # a negative capacity
            args = good()
            args[k][0] = -1
            refused(fn, names[k], args, lead)
        for k, step in ((0, 2), (1, 4), (2, 2), (3, 1), (4, 3)):  # a misaligned array
            args = good()
            args[k][0] = int(args[k][0]) + step
            refused(fn, names[k], args, lead)
        args = good()
        args[8] = C.c_void_p(int(buf.record.data_ptr()) + 4)
        refused(fn, "record_out_dev", args, lead)
    with pytest.raises(ValueError):
        h.store.export_leaving(**{**a, "ids": a["ids"][:2]})
    with pytest.raises(ValueError):
        h.store.export_leaving(**{**a, "offsets": [t[:-1] for t in a["offsets"]]})
    # the refused calls queued nothing; a sequence without tracks needs no arrays, a capacity of 0 neither
    h.est.synchronize()
    assert (buf.record.cpu().numpy() == GUARD_I).all() and all(buf.untouched(s) for s in range(S))
    args = good()
    for k in range(5):
        args[k][1] = None
    args[2][0], args[6][0] = None, 0
    buf.ecap[0] = 0
    assert lib.mld_tracks_export_leaving_device(tr, None, *args) == capi.MLD_OK
    h.est.synchronize()
    buf.check(want, "after the refusals")
    # the sink alone: an array may be null only where its capacity is 0, tracks or not (sequence 1 has none)
    args = good()
    args[0][1] = None
    args[5][1] = 4
    assert lib.mld_tracks_set_leaving_sink(tr, *args) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_export_leaving_device(tr, None, *args) == capi.MLD_OK
    assert lib.mld_tracks_set_leaving_sink(tr, *good()) == capi.MLD_OK
    assert lib.mld_tracks_set_leaving_sink(tr, *([None] * 9)) == capi.MLD_OK  # taken away again
    h.est.synchronize()


def test_without_a_begun_frame_only_a_flush_of_every_sequence_is_served():
    r = Run(3, 300, 4, seed=31)
    a = [np.arange(0, 300, dtype=np.int32), np.zeros(0, np.int32), np.arange(5, 262, dtype=np.int32)]
    for f in range(4):
        r.frame(a, what=f"frame {f}")
    h = r.h
    ns = [len(o) for o in r.orders()]

    def not_served(flush):
        buf = Buffers(h, ns)
        h.torch.cuda.synchronize()
        with pytest.raises(DepthEstimatorError) as e:
            r.export(buf, flush=flush)
        assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED and "mld_tracks_export_leaving_device" in str(e.value)
        h.est.synchronize()
        assert (buf.record.cpu().numpy() == GUARD_I).all() and all(buf.untouched(s) for s in range(3))

    not_served(None)
    not_served([1, 0, 1])
    buf = Buffers(h, ns)
    h.torch.cuda.synchronize()
    r.export(buf, flush=[1, 1, 1])
    h.est.synchronize()
    want = [as_frame(*c.leaving(flush=True)) for c in r.capped]
    assert [w["record"].tolist() for w in want] == [[300, 1200, 0, 0], [0, 0, 0, 0], [257, 1028, 0, 0]]
    buf.check(want, "flush of all, nothing begun")
    own = h.store.leaving_buffers(ns)  # the store's own set, which never truncates, read back with leaving_host()
    h.torch.cuda.synchronize()
    h.store.export_leaving(**own, flush=[1, 1, 1])
    h.est.synchronize()
    for s, (g, w) in enumerate(zip(TrackletStore.leaving_host(own), want)):
        for k, x in w.items():
            assert np.array_equal(g[k].view(np.uint32) if x.dtype == np.float32 else g[k], x.view(np.uint32) if x.dtype == np.float32 else x), (s, k)
    # a begin abandoned by an import counts as no begun frame
    r.begin(a)
    h.store.reset(select=[0, 0, 1])
    r.capped[2].reset()
    ns = [len(o) for o in r.orders()]
    not_served([1, 0, 0])
    r.close()


# ---- through TrackletBatch.step(leaving=...) on a small synthetic cloud ----
H_STEP = 3
N_STEP = (257, 64, 300)


def _step_frames():
    """Five frames of three lanes on VLP-16 clouds (28 800 points): per lane (cloud, coeffs, inliers, ids, u0, v0, u1, v1)."""
    cam, rng = kitti_camera(), np.random.default_rng(37)
    prev, next_id, out = [np.zeros(0, np.int32)] * 3, [0, 0, 7000], []
    for f in range(5):
        per = []
        for s in range(3):
            cloud = synth.make_cloud(synth.VLP16, seed=80 + s, frame=2 * f)
            coeffs, inl = synth.make_ground_plane(cloud)
            ids, next_id[s] = churn(rng, prev[s], N_STEP[s], 0.3, next_id[s])
            u0 = rng.uniform(-2, cam.width + 2, N_STEP[s]).astype(np.float32)
            v0 = rng.uniform(100, cam.height + 2, N_STEP[s]).astype(np.float32)
            u1 = (u0 + rng.normal(0, 3, N_STEP[s])).astype(np.float32)
            v1 = (v0 + rng.normal(0, 2, N_STEP[s])).astype(np.float32)
            per.append((cloud, coeffs, inl, ids, u0, v0, u1, v1))
            prev[s] = ids
        out.append(per)
    return out


def _run_steps(frames, restart_at, with_sink):
    """The frames through step(); lane 1 restarts at frame `restart_at`.  Returns per frame the step's outputs (depths,
    histories, counts), and with a sink per frame the buffers on the host and whether they were left untouched."""
    import torch
    dev = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    tb = TrackletBatch(capi.params_c0(), kitti_camera(), synth.T_CAM_LIDAR, 3, max(N_STEP))
    store = tb.attach_store(H_STEP)
    h = type("H", (), {"torch": torch, "dev": dev, "H": H_STEP})()
    results, sinks = [], []
    for f, per in enumerate(frames):
        clouds = [to(p[0]) for p in per]
        masks = [_mask_of(p[2], p[0].shape[0], dev) for p in per]
        feats = [[to(p[k]) for p in per] for k in (4, 5, 6, 7)]
        outs = ([torch.empty(n, dtype=torch.float32, device=dev) for n in N_STEP],
                [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in N_STEP])
        table = tb.prepare_step(clouds, np.stack([p[1] for p in per]), masks, [to(p[3]) for p in per], *feats, *outs)
        buf = Buffers(h, [0 if f == 0 else n for n in N_STEP])
        restart = [0, 1, 0] if f == restart_at else None
        armed = with_sink and f != restart_at + 1  # (the frame after the restart runs without: the sink was consumed)
        torch.cuda.synchronize()
        tb.step(table, restart=restart, leaving=buf.args() if armed else None)
        fp = [torch.full((n, H_STEP, 3), float(SENTINEL), dtype=torch.float32, device=dev) for n in N_STEP]
        ln = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in N_STEP]
        store.export(fp, ln)
        counts = store.counts()
        tb.est.synchronize()
        results.append({"d_cur": [t.cpu().numpy() for t in outs[0]], "d_last": [t.cpu().numpy() for t in outs[1]],
                        "fp": [t.cpu().numpy() for t in fp], "len": [t.cpu().numpy() for t in ln], "counts": counts})
        sinks.append((buf, armed))
    tb.close()
    return results, sinks


def test_step_with_a_sink_delivers_the_restarting_lane_whole_and_changes_nothing_else():
    """Lane 1 restarts at frame 3.  With a sink armed for every step but the one after the restart: depths, histories
    and counts equal the run without a sink bit for bit; every step's sink equals the capped model fed the step's own
    depths - the restarting lane flushed whole, the other lanes by the marks; the step that follows without `leaving`
    writes nothing (the sink was consumed by one step)."""
    frames, restart_at = _step_frames(), 3
    plain, _ = _run_steps(frames, restart_at, False)
    sunk, sinks = _run_steps(frames, restart_at, True)
    for f, (a, b) in enumerate(zip(plain, sunk)):
        for k in ("d_cur", "d_last", "fp"):
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[k], b[k])), (f, k)
        assert all(np.array_equal(x, y) for x, y in zip(a["len"], b["len"])) and np.array_equal(a["counts"], b["counts"]), f
    capped, archive, full = [CappedStore(H_STEP) for _ in range(3)], TrackArchive(3), [UnboundedMap() for _ in range(3)]
    n_spilled = n_found = 0
    for f, per in enumerate(frames):
        buf, armed = sinks[f]
        flush = [f == restart_at and s == 1 for s in range(3)]
        want = [as_frame(*capped[s].leaving(per[s][3], flush=flush[s])) for s in range(3)]
        buf.h_order = [c.order for c in capped]
        if armed:
            buf.check(want, f"sink of step {f}")
            if f == restart_at:
                assert want[1]["record"].tolist() == [N_STEP[1], int(sunk[f - 1]["len"][1].sum()), 0, 0]
                lens = sunk[f - 1]["len"][1]
                whole = np.concatenate([sunk[f - 1]["fp"][1][i, :lens[i]] for i in range(N_STEP[1])])
                assert np.array_equal(bits(buf.host()[1]["fp"]), bits(whole))  # the lane's whole store, as exported a step earlier
            n_spilled += sum(int(w["record"][2]) for w in want)
            got = buf.host()
        else:
            buf.check(want, f"step {f} without a sink", written=[False] * 3)
            got = want  # (the archive goes on with the model's frame)
        done = archive.push(got)
        erased = []
        for s in range(3):
            p = per[s]
            ended = full[s].end() if flush[s] else []  # the restart: a new TrackletDepthModule
            if flush[s]:
                capped[s].reset()
            args = (p[3], p[4], p[5], p[6], p[7], sunk[f]["d_cur"][s], sunk[f]["d_last"][s])
            capped[s].commit(*args)
            erased.append(ended + full[s].frame(*args))
            n_found += int((sunk[f]["d_cur"][s] > 0).sum())
        for s in range(3):
            got_s = {t.id: t.entries for t in done if t.sequence == s}
            assert sorted(got_s) == sorted(k for k, _ in erased[s]), (f, s)
            for k, e in erased[s]:
                assert np.array_equal(bits(got_s[k]), bits(e)), (f, s, k)
    assert n_spilled > 0 and n_found > 0  # (tracks outlived max_history 3, and real depths were stored)


def test_a_step_refused_before_its_begin_leaves_the_sink_armed_and_writes_nothing():
    import torch
    dev = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    frames = _step_frames()[:2]
    tb = TrackletBatch(capi.params_c0(), kitti_camera(), synth.T_CAM_LIDAR, 3, max(N_STEP))
    store = tb.attach_store(H_STEP)
    h = type("H", (), {"torch": torch, "dev": dev, "H": H_STEP})()
    capped = [CappedStore(H_STEP) for _ in range(3)]
    tables, outs_all = [], []
    for per in frames:
        outs = ([torch.empty(n, dtype=torch.float32, device=dev) for n in N_STEP],
                [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in N_STEP])
        tables.append(tb.prepare_step([to(p[0]) for p in per], np.stack([p[1] for p in per]),
                                      [_mask_of(p[2], p[0].shape[0], dev) for p in per], [to(p[3]) for p in per],
                                      *[[to(p[k]) for p in per] for k in (4, 5, 6, 7)], *outs))
        outs_all.append(outs)
    torch.cuda.synchronize()
    tb.step(tables[0])
    tb.est.synchronize()
    for s, p in enumerate(frames[0]):
        capped[s].commit(p[3], p[4], p[5], p[6], p[7], outs_all[0][0][s].cpu().numpy(), outs_all[0][1][s].cpu().numpy())
    buf = Buffers(h, N_STEP)
    buf.h_order = [c.order for c in capped]
    store.set_leaving_sink(**buf.args())
    bad = dict(tables[1])
    bad["nt"] = (C.c_int64 * 3)(N_STEP[0], -1, N_STEP[2])  # a negative track count: refused by the begin's checks
    torch.cuda.synchronize()
    with pytest.raises(DepthEstimatorError) as e:
        tb.step(bad)
    assert e.value.code == capi.MLD_ERR_INVALID_ARG
    tb.est.synchronize()
    want = [as_frame(*capped[s].leaving(frames[1][s][3])) for s in range(3)]
    buf.check(want, "refused step", written=[False] * 3)
    tb.step(tables[1])  # the sink is still armed
    tb.est.synchronize()
    buf.check(want, "the step after the refusal")
    tb.close()
