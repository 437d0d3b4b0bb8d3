"""mld_row_growth_* on clouds that came out of the projection: the twelve random parameter sets, scaled cameras and rotated
mountings of random_batch_setups.py (unit "rows"), two sequences per call - the seed's frame and the scanner one frame on -,
300 features each, five growth sets.  test_row_growth_gpu.py is thorough about shapes, capacities and bad values on
hand-made visible lists at C0 under the identity transform; here more than half of a visible list lies behind the camera, a
cloud has up to 129 rows of up to 573 points, a window up to 135 returns and a grown list up to 687 entries.

What is compared against is test_row_growth_randomized_cpu.py's, made once per seed: the restatement on the oracle's arrays,
whose tail that file checks against the oracle on the same seeds, and whose states, types and list lengths it asserts.  The
machinery is test_row_growth_gpu.py's: records, row tables and lists BIT-EQUAL between guard bytes.  No tolerance anywhere.

The second half runs TrackletBatch.row_growth behind a step, with no host synchronisation in between: the projection's
arrays against the oracle's, the records against the restatement, and the merge into the arrays the step wrote against a
second, identical batch that did not merge."""
import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimatorError, RowGrowth, TrackletBatch, capi

import row_growth_restatement as RG
from helpers import make_estimator
from random_batch_setups import SEEDS, setup
from test_projected_clouds_gpu import bits
from test_row_growth_gpu import GUARD32, check, dev, run, segment
from test_row_growth_randomized_cpu import (GROWTH, LIST_CAPACITY, N_TRACKS, ROW_CAPACITY, SMALL_ROWS, chain_set, cloud_of, features, form,
                                            restated)

pytestmark = pytest.mark.gpu


class Arrays:
    """A cloud of the CPU file as run() and segment() of test_row_growth_gpu.py read a scene (copies: the shared arrays are
    read-only)."""

    def __init__(self, c):
        self.pm, self.index, self.cam, self.vis_uv = c.pm.copy(), c.index.copy(), c.cam.copy(), c.vis_uv.copy()


@pytest.fixture(scope="module")
def units():
    """One estimator per seed on the seed's parameters, camera and mounting; RowGrowth objects on them; closed at the end."""
    made, objs = {}, []

    def unit(seed, G, row_capacity):
        if seed not in made:
            P, cam, T, _, _ = setup(seed, "rows")
            made[seed] = make_estimator(P, camera=cam, T=T, max_frames=1)
        points = max(cloud_of(seed, w).n_points for w in (0, 1))
        rg = RowGrowth(made[seed], 2, N_TRACKS, points, row_capacity, growth=G)
        objs.append(rg)
        return rg

    yield unit
    for rg in objs:
        rg.close()
    for e in made.values():
        e.close()


def summary(recs):
    """states reached, type-20 count, longest list, for the line a test prints."""
    states = np.concatenate([r["state"] for r in recs])
    return (f"states {dict((int(s), int(n)) for s, n in zip(*np.unique(states, return_counts=True)))}, "
            f"type 20 {sum(int((r['type'] == 20).sum()) for r in recs)}, longest list {max(int(r['n_grown'].max()) for r in recs)}")


# ---- the cloud stage -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_the_rows_of_projected_clouds(units, seed):
    """segment() on the oracle's visible lists of both sequences: record and row table, the guard behind the last entry."""
    cap = ROW_CAPACITY[seed]
    clouds = [cloud_of(seed, w) for w in (0, 1)]
    rec, rows, _ = segment(units(seed, GROWTH["yaml"](), cap), [c.vis_uv.copy() for c in clouds], slack=2)
    for w, c in enumerate(clouds):
        wrec, wrows = RG.cloud_record(c.vis_uv[:, 0], cap, GUARD32)
        assert rec[w] == wrec and np.array_equal(rows[w], wrows), (seed, w)
        assert rec[w]["flags"] == 0 and rec[w]["n_vis"] == c.n_vis
    print(f"row-growth seed {seed} set -: rows {rec['n_rows'].tolist()} of capacity {cap}, longest row {rec['longest_row'].tolist()}, "
          f"visible {rec['n_vis'].tolist()}")


def test_a_row_table_below_the_row_count(units):
    """The table holds 16 rows, the clouds 129: the cloud record says so, the table ends with the start of the first row
    that did not fit and keeps its guard, and every feature is flagged and nothing else."""
    seed, cap = SMALL_ROWS
    clouds = [cloud_of(seed, w) for w in (0, 1)]
    rg = units(seed, GROWTH["wide"](), cap)
    rec, rows, _ = segment(rg, [c.vis_uv.copy() for c in clouds])
    for w, c in enumerate(clouds):
        wrec, wrows = RG.cloud_record(c.vis_uv[:, 0], cap, GUARD32)
        assert rec[w] == wrec and np.array_equal(rows[w], wrows) and rows[w].size == cap + 1, w
        assert rec[w]["flags"] == RG.ROWS_TRUNCATED and rec[w]["n_rows"] > cap + 1
    for tracks in (False, True):
        uvs = [features(seed, w).copy() for w in (0, 1)]
        got = run(rg, [Arrays(c) for c in clouds], uvs, cap=4, tracks=tracks, merge=True)
        for w in (0, 1):
            check(got[w], restated(seed, "wide", w, tracks=tracks, row_capacity=cap), f"seed {seed} sequence {w} tracks {tracks}")
            r, grown, depth, types = got[w]
            assert (r["flags"] == RG.ROWS_TRUNCATED).all() and (r["type"] == 0).all() and (grown == GUARD32).all()
            assert types.tolist() == list(range(50, 50 + N_TRACKS)) and (depth == 100.0 + 0.5 * np.arange(N_TRACKS)).all()
    print(f"row-growth seed {seed} set wide: row capacity {cap} below rows {rec['n_rows'].tolist()}: every feature ROWS_TRUNCATED")


# ---- the feature stage -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GROWTH))
@pytest.mark.parametrize("seed", SEEDS)
def test_records_and_lists_equal_the_restatement(units, seed, name):
    """Both sequences in one call, the feature form by the seed (tracks on the odd ones), the lists cut at the set's
    capacity; the merge arrays hold the decided entries and keep the others and their guards."""
    tracks, cap = form(seed), LIST_CAPACITY[name]
    clouds = [cloud_of(seed, w) for w in (0, 1)]
    want = [restated(seed, name, w) for w in (0, 1)]
    uvs = [features(seed, w).copy() for w in (0, 1)]
    got = run(units(seed, GROWTH[name](), ROW_CAPACITY[seed]), [Arrays(c) for c in clouds], uvs, cap=cap, tracks=tracks, merge=True)
    for w in (0, 1):
        check(got[w], want[w], f"seed {seed} set {name} sequence {w}")
        rec, depth, types = want[w][0], got[w][2], got[w][3]
        dec = RG.decides(rec)
        merged_d = np.where(dec, rec["depth"], 100.0 + 0.5 * np.arange(N_TRACKS)).astype(np.float32 if tracks else np.float64)
        assert np.array_equal(bits(depth), bits(merged_d)), (seed, name, w)
        assert np.array_equal(types, np.where(dec, rec["type"], 50 + np.arange(N_TRACKS))), (seed, name, w)
    print(f"row-growth seed {seed} set {name}: {summary([w[0] for w in want])}, list capacity {cap}, rows "
          f"{[int(RG.cloud_record(c.vis_uv[:, 0], 1)[0]['n_rows']) for c in clouds]}, {'tracks' if tracks else 'uv'} form")


# ---- TrackletBatch.row_growth behind a step ------------------------------------------------------------------------------------

def mask_of(inliers, n):
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    inliers = np.asarray(inliers, dtype=np.int64)
    np.bitwise_or.at(m, inliers >> 5, (np.uint32(1) << (inliers & 31).astype(np.uint32)))
    return m.view(np.int32)


class Chain:
    """A TrackletBatch on the seed's setup with its two sequences and their 300 tracks each, the projected clouds exported
    and one frame prepared: on the odd seeds for step() with a store, on the even ones for run()."""

    def __init__(self, seed, G):
        import torch
        d = dev()
        P, cam, T, _, _ = setup(seed, "rows")
        self.clouds = [cloud_of(seed, w) for w in (0, 1)]
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
        self.with_store = seed % 2 == 1
        self.tb = tb = TrackletBatch(P, cam, T, 2, N_TRACKS)
        points = max(c.n_points for c in self.clouds)
        tb.attach_projected_clouds(points)
        if self.with_store:
            tb.attach_store(4)
        self.G, self.points = G, points
        cl = [to(c.cloud.copy()) for c in self.clouds]
        self.pc = tb.projected_clouds(cl, cam=True, pixel_map=True)
        tracks = [features(seed, w).astype(np.float32) for w in (0, 1)]
        rng = np.random.default_rng(6500 + seed)
        u = [to(t[:, 0]) for t in tracks]
        v = [to(t[:, 1]) for t in tracks]
        u_old = [to(t[:, 0] + rng.normal(0, 2, N_TRACKS).astype(np.float32)) for t in tracks]
        v_old = [to(t[:, 1] + rng.normal(0, 1, N_TRACKS).astype(np.float32)) for t in tracks]
        self.d_cur = [torch.full((N_TRACKS,), -77.0, dtype=torch.float32, device=d) for _ in range(2)]
        self.d_last = [torch.full((N_TRACKS,), -77.0, dtype=torch.float32, device=d) for _ in range(2)]
        self.t_cur = [torch.full((N_TRACKS,), -7, dtype=torch.int32, device=d) for _ in range(2)]
        self.t_last = [torch.full((N_TRACKS,), -7, dtype=torch.int32, device=d) for _ in range(2)]
        coeffs = np.stack([np.asarray(c.plane[0], dtype=np.float32) for c in self.clouds])
        masks = [to(mask_of(c.plane[1], c.n_points)) for c in self.clouds]
        outs = (self.d_cur, self.d_last, self.t_cur, self.t_last)
        if self.with_store:
            ids = [to(np.arange(N_TRACKS, dtype=np.int32) + 1000 * w) for w in (0, 1)]
            self.f = tb.prepare_step(cl, coeffs, masks, ids, u, v, u_old, v_old, *outs)
        else:
            new = [torch.ones(N_TRACKS, dtype=torch.uint8, device=d) for _ in range(2)]
            self.f = tb.prepare(cl, coeffs, masks, u, v, u_old, v_old, new, *outs)
        torch.cuda.synchronize()

    def step(self):
        self.tb.step(self.f) if self.with_store else self.tb.run(self.f)

    def current(self):
        """(the bits of the float32 depths, types) per sequence of what stands in the step's output arrays (a host read:
        waits for the estimator's stream first, which a step alone does not make torch's stream do)."""
        self.tb.est.synchronize()
        return [(self.d_cur[w].cpu().numpy().view(np.uint32), self.t_cur[w].cpu().numpy()) for w in (0, 1)]

    def close(self):
        self.tb.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_tracklet_batch_row_growth_behind_a_step(seed):
    """projected_clouds -> step -> row_growth(merge) with nothing in between, against a second batch that only stepped."""
    name = chain_set(seed)
    G, cap = GROWTH[name](), LIST_CAPACITY[name]
    want = [restated(seed, name, w, tracks=True) for w in (0, 1)]
    a, b = Chain(seed, G), Chain(seed, G)
    try:
        for ch in (a, b):
            rg = ch.tb.attach_row_growth(G, ROW_CAPACITY[seed], ch.points)
            assert type(rg) is RowGrowth and ch.tb.attach_row_growth() is rg
        # the projection on the seed's mounting is the oracle's
        nvis = a.pc["n_visible"].cpu().numpy()
        for w, c in enumerate(a.clouds):
            m = int(nvis[w])
            assert m == c.n_vis
            assert np.array_equal(a.pc["pixel_map"][w].cpu().numpy(), c.pm) and np.array_equal(a.pc["index"][w][:m].cpu().numpy(), c.index)
            assert np.array_equal(bits(a.pc["cam"][w].cpu().numpy()), bits(c.cam))
            assert np.array_equal(bits(a.pc["uv"][w][:m].cpu().numpy()), bits(c.vis_uv))
        import torch
        torch.cuda.synchronize()
        # a: the step and the merge, queued without a host synchronisation between them; b: the step alone
        a.step()
        out = a.tb.row_growth(a.f, a.pc, list_capacity=cap, merge=a.f["current"])
        b.step()
        stepped = b.current()
        assert all((t != -7).all() for _, t in stepped)  # (the step wrote every entry)
        merged = a.current()
        crec = RowGrowth.cloud_records(out["cloud"])
        n_changed = 0
        for w, c in enumerate(a.clouds):
            rec, lists = want[w]
            assert RG.same_records(RowGrowth.records(out["record"][w]), rec) == [], (seed, w)
            grown = out["grown"][w].cpu().numpy()
            for i, ls in enumerate(lists):
                k = min(ls.size, cap)
                assert np.array_equal(grown[i, :k], ls[:k]), (seed, w, i)
            wrec, wrows = RG.cloud_record(c.vis_uv[:, 0], ROW_CAPACITY[seed])
            assert crec[w] == wrec
            rows = out["row_start"][w].cpu().numpy()
            assert np.array_equal(rows[:wrec["n_rows"] + 1], wrows[:wrec["n_rows"] + 1])
            # the merge: the decided entries hold the stage's result, every other one is what the step wrote
            dec = RG.decides(rec)
            want_d = np.where(dec, rec["depth"].astype(np.float32), stepped[w][0].view(np.float32))
            want_t = np.where(dec, rec["type"], stepped[w][1])
            assert np.array_equal(merged[w][0], want_d.view(np.uint32)) and np.array_equal(merged[w][1], want_t), (seed, w)
            # (a type-20 depth is not always positive: on seed 2, do_use_cut_behind_camera 0, lists grown from a second seed
            #  behind the camera give -3.7 .. -16.7 m, in the restatement and on the GPU alike)
            assert (want_d[np.isin(rec["type"], (3, 4))] == -1.0).all() and np.isfinite(want_d[rec["type"] == 20]).all()
            changed = (merged[w][0] != stepped[w][0]) | (merged[w][1] != stepped[w][1])
            assert not changed[~dec].any()
            n_changed += int(changed.sum())
        # merge=None leaves the step's outputs as they are; a second call on the same table gives the same records
        again_b = b.tb.row_growth(b.f, b.pc, list_capacity=cap)
        again_a = a.tb.row_growth(a.f, a.pc)
        assert again_a["grown"] is None
        for w in (0, 1):
            assert RG.same_records(RowGrowth.records(again_b["record"][w]), want[w][0]) == [], (seed, w)
            assert RG.same_records(RowGrowth.records(again_a["record"][w]), want[w][0]) == [], (seed, w)
            assert np.array_equal(again_b["grown"][w].cpu().numpy()[:, :1][want[w][0]["n_grown"] > 0, 0],
                                  np.array([ls[0] for ls in want[w][1] if ls.size], dtype=np.int32))
        for got, was in zip(b.current(), stepped):
            assert np.array_equal(got[0], was[0]) and np.array_equal(got[1], was[1])
        for got, was in zip(a.current(), merged):
            assert np.array_equal(got[0], was[0]) and np.array_equal(got[1], was[1])
        decided = sum(int(RG.decides(w[0]).sum()) for w in want)
        print(f"row-growth seed {seed} set {name}: {summary([w[0] for w in want])}, rows {crec['n_rows'].tolist()}; behind "
              f"{'step()' if a.with_store else 'run()'}: {decided} entries decided, {n_changed} of them differ from the step's")
    finally:
        a.close()
        b.close()


def test_row_growth_without_attach_names_both():
    P, cam, T, _, _ = setup(0, "rows")
    tb = TrackletBatch(P, cam, T, 1, 10)
    try:
        with pytest.raises(DepthEstimatorError) as e:
            tb.row_growth({"features": ([None], [None])}, {})
        assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED
        assert "TrackletBatch.row_growth without attach_row_growth" in str(e.value)
        for bad in (dict(row_capacity=0), dict(row_capacity=RowGrowth.MAX_ROWS + 1), dict(max_points=0),
                    dict(growth=capi.row_growth_params_yaml().replace(depth_segmentation_max_pointcount=RowGrowth.MAX_COUNT + 1))):
            with pytest.raises(DepthEstimatorError) as e:
                tb.attach_row_growth(**bad)
            assert e.value.code == capi.MLD_ERR_INVALID_ARG and tb.row_growth_lists is None
    finally:
        tb.close()


def test_close_destroys_the_unit_before_the_estimator(monkeypatch):
    """With the calls still queued: the unit's destroy waits for them, then the estimator goes."""
    import torch
    seed, name = 9, "tight"
    ch = Chain(seed, GROWTH[name]())
    rg = ch.tb.attach_row_growth(ch.G, ROW_CAPACITY[seed], ch.points)
    order = []
    rg_close, est_close = rg.close, ch.tb.est.close
    monkeypatch.setattr(rg, "close", lambda: (order.append("row_growth"), rg_close())[1])
    monkeypatch.setattr(ch.tb.est, "close", lambda: (order.append("estimator"), est_close())[1])
    out = ch.tb.row_growth(ch.f, ch.pc, list_capacity=LIST_CAPACITY[name])
    ch.close()
    assert order == ["row_growth", "estimator"] and ch.tb.row_growth_lists is None and rg._rg is None
    torch.cuda.synchronize()
    for w in (0, 1):
        rec, lists = restated(seed, name, w, tracks=True)
        assert RG.same_records(RowGrowth.records(out["record"][w]), rec) == [], w
        assert np.array_equal(out["grown"][w].cpu().numpy()[rec["n_grown"] > 0, 0], np.array([ls[0] for ls in lists if ls.size], dtype=np.int32))
