"""mld_tracks_export_packed_device (TrackletStore.export_packed): the stored tracks back to back with their offsets.

The store is driven with synthetic depths (a fifth -1, a few NaN) through the Harness of tests/test_track_store_gpu.py.
Everything is compared on bit patterns, twice: with the dict-of-lists restatement of
tracklet_depth_module.cpp:209-259 (every Tracklet carries exactly `curTracklet.size()` points), and with the compaction
of the store's own fixed-stride export of the same state, `concat_i fp[i, :len[i]]`.  The output buffers are longer than
they are said to be and hold a sentinel: nothing at or beyond min(total, capacity) may change.

Shapes: 0, 1, 255, 256, 257 and 600 tracks (a block of the kernels takes 256 tracks), ragged in one call, 1 / 5 / 13
sequences, max_history 2 / 3 / 16 with tracks of every age from 1 to beyond max_history, and one sequence with more
blocks than one pass of the sequence-level scan is wide.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimatorError, TrackletBatch, capi, synth

from helpers import kitti_camera
from test_track_store_gpu import SENTINEL, Harness, Restatement, bits, churn

pytestmark = pytest.mark.gpu

SCAN_WIDTH = 256  # W: block sums one pass of k_tracks_pack_scan takes (kScanWidth, csrc/tracks/mld_tracks.hip)
BLOCK = 256       # tracks per block of the store's kernels
PAD = 9           # entries of sentinel behind what a buffer is said to hold
SIZES = (0, 1, 255, 256, 257, 600)


def compact(lens, fp):
    """(offsets [n + 1] int64, entries [total, 3]) of fixed-stride (lengths [n], entries [n, H, 3])."""
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    keep = np.arange(fp.shape[1])[None, :] < np.asarray(lens)[:, None]
    return off, np.ascontiguousarray(fp[keep]).reshape(-1, 3)


def export_fixed(h, ns):
    """The store's fixed-stride export of the committed frame, on the host."""
    torch = h.torch
    fp = [torch.full((n, h.H, 3), float(SENTINEL), dtype=torch.float32, device=h.dev) for n in ns]
    ln = [torch.full((n,), -9, dtype=torch.int32, device=h.dev) for n in ns]
    torch.cuda.synchronize()
    h.store.export(fp, ln)
    h.est.synchronize()
    return [t.cpu().numpy() for t in ln], [t.cpu().numpy() for t in fp]


class Packed:
    """Output buffers of one packed export: offsets pre-filled with -9, entries with SENTINEL and PAD entries longer
    than the capacity the store is told."""

    def __init__(self, h, ns, caps=None, with_fp=True):
        torch = h.torch
        self.h, self.ns = h, ns
        self.caps = [h.store.packed_capacity(n) for n in ns] if caps is None else list(caps)
        self.off = [torch.full((n + 1,), -9, dtype=torch.int64, device=h.dev) for n in ns]
        self.buf = [torch.full((c + PAD, 3), float(SENTINEL), dtype=torch.float32, device=h.dev) for c in self.caps]
        self.fp = [b[:c] for b, c in zip(self.buf, self.caps)] if with_fp else None

    def run(self):
        self.h.store.export_packed(self.fp, self.off)

    def check(self, expect, what, skip_tracks=None):
        """expect: per sequence (offsets, entries).  skip_tracks: per sequence the indices of tracks whose entries are
        not compared (their offsets are)."""
        for s, (e_off, e_fp) in enumerate(expect):
            n, cap = self.ns[s], self.caps[s]
            g_off, g_buf = self.off[s].cpu().numpy(), self.buf[s].cpu().numpy()
            if n == 0:  # nothing is written for a sequence without tracks
                assert g_off.tolist() == [-9] and (bits(g_buf) == bits(SENTINEL)).all(), f"{what}: sequence {s} was written"
                continue
            assert np.array_equal(g_off, e_off), f"{what}: sequence {s}: offsets differ"
            total = int(e_off[-1])
            m = min(total, cap) if self.fp is not None else 0
            want = e_fp[:m].copy()
            got = g_buf[:m].copy()
            for i in (skip_tracks[s] if skip_tracks else ()):
                a, b = min(int(e_off[i]), m), min(int(e_off[i + 1]), m)
                got[a:b] = want[a:b]
            assert np.array_equal(bits(got), bits(want)), f"{what}: sequence {s}: entries differ"
            assert (bits(g_buf[m:]) == bits(SENTINEL)).all(), f"{what}: sequence {s}: written at or beyond {m}"


def expect_restatement(h):
    return [compact(*r.export()) for r in h.ref]


def expect_fixed(h, ns):
    lens, fps = export_fixed(h, ns)
    return [compact(l, f) for l, f in zip(lens, fps)]


def check_both(h, what, skip_tracks=None):
    """One packed export of the committed frame against the restatement and against the fixed-stride export."""
    ns = [len(r.order) for r in h.ref]
    fixed = expect_fixed(h, ns)
    p = Packed(h, ns)
    h.torch.cuda.synchronize()
    p.run()
    h.est.synchronize()
    p.check(expect_restatement(h), what + " / restatement", skip_tracks)
    p.check(fixed, what + " / fixed stride")
    return fixed


def grow(h, sizes_of_frame, frames, check_at, seed):
    """`frames` frames with 30 % new tracks each; sizes_of_frame(f) = the track counts of frame f."""
    rng = np.random.default_rng(seed)
    prev = [np.zeros(0, np.int32)] * h.S
    next_id = [100000 * s for s in range(h.S)]
    for f in range(frames):
        ids = []
        for s, n in enumerate(sizes_of_frame(f)):
            i, next_id[s] = churn(rng, prev[s], n, 0.3, next_id[s])
            ids.append(i)
        h.frame(ids, check=False)
        prev = ids
        if f in check_at:
            check_both(h, f"frame {f}")


def test_one_sequence_at_every_size():
    """One sequence whose frame shrinks and grows through 600, 257, 256, 255, 1 and 0 tracks, max_history 2: every track
    is as old as the history is long after its first frame."""
    h = Harness(1, 600, 2, seed=3)
    order = (600, 257, 256, 255, 1, 0, 600, 600)
    grow(h, lambda f: [order[f]], len(order), set(range(len(order))), seed=3)
    h.close()


def test_five_sequences_ragged_history_of_three():
    """0, 1, 255, 256, 257 and 600 tracks over five sequences in one call, rotating one place every second frame;
    max_history 3, so lengths 2 and 3 mix wherever tracks survive."""
    h = Harness(5, 600, 3, seed=5)
    grow(h, lambda f: [SIZES[(s + f // 2) % 6] for s in range(5)], 8, {0, 1, 3, 5, 7}, seed=5)
    h.close()


def test_thirteen_sequences_every_age_up_to_and_beyond_a_history_of_sixteen():
    """All six sizes and seven more in one call, 19 frames with 30 % new tracks each: tracks of every age from 1 to 19
    exist, the oldest longer than max_history 16 (their rings have wrapped)."""
    sizes = list(SIZES) + [0, 599, 300, 2, 513, 64, 431]
    h = Harness(13, 600, 16, seed=13)
    grow(h, lambda f: sizes, 19, {0, 7, 15, 18}, seed=13)
    lens = np.concatenate([r.export()[0] for r in h.ref])
    assert set(lens.tolist()) == set(range(2, 17))  # every length occurs, 16 = the ones older than the history
    heads_wrapped = sum(1 for r in h.ref for t in r.order if len(r.map[t]) == 16)
    assert heads_wrapped > 0
    h.close()


def test_a_sequence_with_more_blocks_than_the_scan_is_wide():
    """256 * W + 257 tracks (W = 256 block sums per pass of the sequence-level scan: 258 blocks, the second pass takes
    two of them) and 70 001 tracks (274 blocks) as two sequences of one call, max_history 2, two frames."""
    n0 = BLOCK * SCAN_WIDTH + 257
    assert (n0 + BLOCK - 1) // BLOCK > SCAN_WIDTH
    ns = (n0, 70001)
    h = Harness(2, max(ns), 2, seed=17)
    grow(h, lambda f: ns, 2, {1}, seed=17)
    h.close()


def _duplicate_frames(h):
    """test_track_store_gpu's frames with a repeated id: sequence 0 repeats a known id, sequence 1 a new one."""
    rng = np.random.default_rng(23)
    h.frame([np.arange(0, 300, dtype=np.int32), np.arange(0, 300, dtype=np.int32)], check=False)
    others = np.setdiff1d(np.arange(0, 298, dtype=np.int32), [42])
    ids0 = np.concatenate([[42], rng.permutation(others), [42]]).astype(np.int32)
    ids1 = np.concatenate([[777], np.arange(100, 398, dtype=np.int32), [777]]).astype(np.int32)
    h.frame([ids0, ids1], check=False)
    return [ids0, ids1]


def test_a_frame_with_repeated_ids():
    """Both occurrences of a repeated id export the stored occurrence's history: the offsets are the restatement's
    (either occurrence has the same length), the entries of the two tracks are the fixed-stride export's, whichever
    occurrence the store kept."""
    h = Harness(2, 400, 4, seed=23)
    ids = _duplicate_frames(h)
    assert h.store.counts()[:, 5].tolist() == [1, 1]
    skip = [np.flatnonzero(ids[0] == 42).tolist(), np.flatnonzero(ids[1] == 777).tolist()]
    assert [len(k) for k in skip] == [2, 2]
    fixed = check_both(h, "repeated ids", skip_tracks=skip)
    for s in range(2):  # the loser's entries are the winner's
        off, fp = fixed[s]
        a, b = skip[s]
        assert off[a + 1] - off[a] == off[b + 1] - off[b] > 0
        assert np.array_equal(bits(fp[off[a]:off[a + 1]]), bits(fp[off[b]:off[b + 1]]))
    h.close()


@pytest.fixture(scope="module")
def grown():
    """Four ragged sequences (one without tracks), max_history 5, seven frames; with the expected packed export."""
    h = Harness(4, 600, 5, seed=29)
    sizes = [600, 0, 257, 1]
    grow(h, lambda f: sizes, 7, set(), seed=29)
    expect = expect_restatement(h)
    assert [int(e[0][-1]) for e in expect][1] == 0 and min(int(e[0][-1]) for e in expect[::2]) > 600
    yield h, sizes, expect
    h.close()


@pytest.mark.parametrize("which", ["zero", "total-1", "total", "total+7"])
def test_capacity_truncates_the_entries_and_never_the_offsets(grown, which):
    h, sizes, expect = grown
    totals = [int(e[0][-1]) for e in expect]
    caps = [{"zero": 0, "total-1": max(t - 1, 0), "total": t, "total+7": t + 7}[which] for t in totals]
    p = Packed(h, sizes, caps=caps)
    h.torch.cuda.synchronize()
    p.run()
    h.est.synchronize()
    p.check(expect, f"capacity {which}")
    p.check(expect_fixed(h, sizes), f"capacity {which} / fixed stride")


def test_offsets_alone(grown):
    h, sizes, expect = grown
    p = Packed(h, sizes, with_fp=False)
    h.torch.cuda.synchronize()
    p.run()
    h.est.synchronize()
    p.check(expect, "fp_out = None")  # (the buffers, which the store never saw, still hold the sentinel)


def test_two_exports_queued_back_to_back(grown):
    """Two calls without a synchronisation between them, into different buffers, the first one truncated: they share
    the store's scan scratch and its descriptor ring, and neither disturbs the other."""
    h, sizes, expect = grown
    totals = [int(e[0][-1]) for e in expect]
    first, second = Packed(h, sizes, caps=[t // 2 for t in totals]), Packed(h, sizes)
    h.torch.cuda.synchronize()
    first.run()
    second.run()
    h.est.synchronize()
    first.check(expect, "first of two")
    second.check(expect, "second of two")


def test_refusals(grown):
    h, sizes, expect = grown
    lib, tr, S = h.store._lib, h.store._tr, h.S
    p = Packed(h, sizes)
    h.torch.cuda.synchronize()
    tab = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    cap = lambda v: (C.c_int64 * S)(*v)  # noqa: E731

    def refused(word, *args):
        assert lib.mld_tracks_export_packed_device(*args) == capi.MLD_ERR_INVALID_ARG
        text = lib.mld_tracks_last_error(tr).decode()
        assert "mld_tracks_export_packed_device" in text and word in text, text

    assert lib.mld_tracks_export_packed_device(None, tab(p.fp), cap(p.caps), tab(p.off)) == capi.MLD_ERR_INVALID_ARG
    refused("offsets_out", tr, tab(p.fp), cap(p.caps), None)
    refused("capacity", tr, tab(p.fp), None, tab(p.off))
    refused("capacity", tr, tab(p.fp), cap([p.caps[0], 0, -1, p.caps[3]]), tab(p.off))
    hole = tab(p.off)
    hole[2] = None  # (sequence 2 has tracks)
    refused("offsets_out", tr, tab(p.fp), cap(p.caps), hole)
    hole = tab(p.fp)
    hole[0] = None
    refused("fp_out", tr, hole, cap(p.caps), tab(p.off))
    with pytest.raises(DepthEstimatorError) as e:
        h.store.export_packed(p.fp, None)
    assert e.value.code == capi.MLD_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        h.store.export_packed(p.fp[:2], p.off)
    # a sequence without tracks needs no arrays, and the refused calls wrote nothing and left the store usable
    h.est.synchronize()
    for s in range(S):
        assert (p.off[s].cpu().numpy() == -9).all() and (bits(p.buf[s].cpu().numpy()) == bits(SENTINEL)).all()
    fp_tab, off_tab = tab(p.fp), tab(p.off)
    fp_tab[1] = None
    off_tab[1] = None
    assert lib.mld_tracks_export_packed_device(tr, fp_tab, cap(p.caps), off_tab) == capi.MLD_OK
    h.est.synchronize()
    p.check(expect, "after the refusals")


def _mask_of(inl, n, dev):
    import torch
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return torch.from_numpy(m.view(np.int32)).to(dev)


def test_queued_behind_a_step_with_real_depths():
    """TrackletBatch.step on two VLP-16 clouds (28 800 points), then the packed export at once, no synchronisation in
    between: the export reads the histories the step's commit has just written.  Three frames, so lengths 2, 3 and 4."""
    import torch
    dev = torch.device("cuda:0")
    S, H, ns = 2, 6, (300, 257)
    cam, rng = kitti_camera(), np.random.default_rng(31)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tb = TrackletBatch(capi.params_c0(), cam, synth.T_CAM_LIDAR, S, max(ns))
    store = tb.attach_store(H)
    ref = [Restatement(H) for _ in range(S)]
    prev, next_id, found = [np.zeros(0, np.int32)] * S, [0] * S, 0
    for f in range(3):
        per = []
        for s in range(S):
            cloud = synth.make_cloud(synth.VLP16, seed=70 + s, frame=2 * f)
            coeffs, inl = synth.make_ground_plane(cloud)
            ids, next_id[s] = churn(rng, prev[s], ns[s], 0.3, next_id[s])
            u0 = rng.uniform(-2, cam.width + 2, ns[s]).astype(np.float32)
            v0 = rng.uniform(100, cam.height + 2, ns[s]).astype(np.float32)
            u1 = (u0 + rng.normal(0, 3, ns[s])).astype(np.float32)
            v1 = (v0 + rng.normal(0, 2, ns[s])).astype(np.float32)
            per.append((cloud, coeffs, inl, ids, u0, v0, u1, v1))
            prev[s] = ids
        clouds = [to(p[0]) for p in per]
        masks = [_mask_of(p[2], p[0].shape[0], dev) for p in per]
        feats = [[to(p[k]) for p in per] for k in (4, 5, 6, 7)]
        ids_d = [to(p[3]) for p in per]
        outs = ([torch.empty(n, dtype=torch.float32, device=dev) for n in ns],
                [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in ns])
        table = tb.prepare_step(clouds, np.stack([p[1] for p in per]), masks, ids_d, *feats, *outs)
        off = [torch.full((n + 1,), -9, dtype=torch.int64, device=dev) for n in ns]
        buf = [torch.full((store.packed_capacity(n) + PAD, 3), float(SENTINEL), dtype=torch.float32, device=dev) for n in ns]
        torch.cuda.synchronize()
        tb.step(table)
        store.export_packed([b[:store.packed_capacity(n)] for b, n in zip(buf, ns)], off)  # (directly behind the step)
        tb.est.synchronize()
        fp = [torch.full((n, H, 3), float(SENTINEL), dtype=torch.float32, device=dev) for n in ns]
        ln = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
        torch.cuda.synchronize()
        store.export(fp, ln)
        tb.est.synchronize()
        for s in range(S):
            p = per[s]
            ref[s].commit(p[3], p[4], p[5], p[6], p[7], outs[0][s].cpu().numpy(), outs[1][s].cpu().numpy())
            g_off, g_buf = off[s].cpu().numpy(), buf[s].cpu().numpy()
            for what, (e_off, e_fp) in (("restatement", compact(*ref[s].export())),
                                        ("fixed stride", compact(ln[s].cpu().numpy(), fp[s].cpu().numpy()))):
                total = int(e_off[-1])
                assert np.array_equal(g_off, e_off), f"frame {f}, sequence {s}, {what}: offsets differ"
                assert np.array_equal(bits(g_buf[:total]), bits(e_fp)), f"frame {f}, sequence {s}, {what}: entries differ"
                assert (bits(g_buf[total:]) == bits(SENTINEL)).all()
            found += int((g_buf[:int(g_off[-1]), 2] > 0).sum())
    assert set(np.diff(g_off).tolist()) == {2, 3, 4} and found > 0  # (real depths were stored)
    tb.close()
