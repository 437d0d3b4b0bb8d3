#!/usr/bin/env python3
"""Import, lanes and restart of the batched tracklet layer on BASELINE config 5's shapes (profiles/track_import.md).

  --part import   mld_tracks_import_packed_device against mld_tracks_export_packed_device of the SAME store in the same
                  run (the store takes its own export back in), 256 sequences x 10 000 tracks x max_history 16 after 16
                  frames with 30 % churn - the shape of profiles/packed_export.md.  Event windows around `--reps` calls at
                  the C entry, in turn; both against the bytes they must move at the streaming rate of
                  profiles/r6_streamread.txt.  The import is checked first: the store's exports after it equal those
                  before it, bit for bit.
  --part step     the step of profiles/tools/track_store_step.py (128 x 4096 clouds, 10 000 tracks, 30 % new per frame,
                  list capacities 48 / 24) three ways in one process, in turn: `step` (mld_tracklets_step_device), `lanes`
                  (mld_tracklets_step_lanes_device, every lane running, restart NULL) and `restart` (the same with ONE
                  lane restarting on every step).  Wall time over `--steps` steps queued back to back.

Prints one JSON line and a markdown table per part; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, TrackletBatch, TrackletStore, capi, synth  # noqa: E402

STREAM_TBS = 7.0  # profiles/r6_streamread.txt: 16-byte records, non-temporal loads


def camera():
    return CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)


def stat(v):
    return {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def cell(r):
    return f"{r['median_ms']:.3f} [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]"


def part_import(S, n, H, frames, new_frac, reps, rounds, n_check):
    import torch
    dev = torch.device("cuda", 0)
    est = DepthEstimator(device=0, max_frames=1)
    est.InitConfig(capi.params_c0())
    est.Initialize(camera(), synth.T_CAM_LIDAR)
    store = TrackletStore(est, S, n, H)
    stream = torch.cuda.ExternalStream(est.stream, device=dev)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    n_new = int(n * new_frac)
    ids = (torch.arange(n, dtype=torch.int64, device=dev)[None, :] + (torch.arange(S, device=dev) * 7919)[:, None]).contiguous()
    next_id = n
    for f in range(frames):  # (the frames of profiles/tools/packed_export.py)
        if f:
            where = torch.rand((S, n), generator=gen, device=dev).argsort(dim=1)[:, :n_new]
            fresh = torch.arange(next_id, next_id + n_new, device=dev)[None, :] + (torch.arange(S, device=dev) * 7919)[:, None]
            ids.scatter_(1, where, fresh)
            next_id += n_new
        ids32 = ids.to(torch.int32).contiguous()
        feat = [torch.rand((S, n), generator=gen, device=dev) * 1200.0 for _ in range(4)]
        depth = [torch.rand((S, n), generator=gen, device=dev) * 80.0 for _ in range(2)]
        for d in depth:
            d[torch.rand((S, n), generator=gen, device=dev) < 0.2] = -1.0
        torch.cuda.synchronize()
        store.begin(rows(ids32))
        store.commit(*[rows(t) for t in feat + depth])
        est.synchronize()
    before = store.counts()
    cap = store.packed_capacity(n)
    fp = torch.zeros((2, S, cap, 3), dtype=torch.float32, device=dev)
    offsets = torch.zeros((2, S, n + 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib, tr = store._lib, store._tr
    table = lambda t: (C.c_void_p * S)(*[int(t[q].data_ptr()) for q in range(S)])  # noqa: E731
    t_fp, t_off, t_ids = [table(fp[k]) for k in range(2)], [table(offsets[k]) for k in range(2)], table(ids32)
    caps, nt = (C.c_int64 * S)(*[cap] * S), (C.c_int64 * S)(*[n] * S)

    def export(k=0):
        assert lib.mld_tracks_export_packed_device(tr, t_fp[k], caps, t_off[k]) == capi.MLD_OK

    export()
    est.synchronize()
    totals = offsets[0, :, n].cpu().numpy()
    ne = (C.c_int64 * S)(*[int(x) for x in totals])

    def load():
        assert lib.mld_tracks_import_packed_device(tr, None, t_ids, nt, t_off[0], t_fp[0], ne) == capi.MLD_OK

    # the same store afterwards
    load()
    export(1)
    after = store.counts()
    assert torch.equal(offsets[0], offsets[1]), "offsets after the import differ"
    for q in range(min(n_check, S)):
        m = int(totals[q])
        assert torch.equal(fp[0, q, :m].view(torch.int32), fp[1, q, :m].view(torch.int32)), f"sequence {q}: entries differ"
    assert (after[:, [0, 3, 4, 5]] == before[:, [0, 3, 4, 5]]).all() and (after[:, 1] == n).all() and (after[:, 2] == 0).all()

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        est.synchronize()
        return e0.elapsed_time(e1) / reps

    window(export)
    window(load)
    w = {"export": [], "import": []}
    for _ in range(rounds):
        w["export"].append(window(export))
        w["import"].append(window(load))
    entries, tracks = int(totals.sum()), S * n
    table_slots = 2
    while table_slots < 2 * n:
        table_slots <<= 1
    # bytes each call must move (device memory, once each)
    #   import: ids 4 + offsets 8 per track and 12 per entry read; written: the table cleared (8 per slot) and a slot per
    #           track (8), the free stack (4 per row), 12 per entry into the rows, head / len / row / slot / dup_row (20)
    #   export: row, len and head per track (12) and 12 per entry read; 12 per entry and an offset per track (8) written
    floor_import = tracks * (4 + 8 + 8 + 20) + entries * 24 + S * (8 * table_slots + 4 * n)
    floor_export = tracks * (12 + 8) + entries * 24
    res = {"part": "import", "S": S, "n_tracks": n, "max_history": H, "frames": frames, "new_frac": new_frac, "reps": reps,
           "rounds": rounds, "entries": entries, "mean_length": round(entries / tracks, 3), "export": stat(w["export"]),
           "import": stat(w["import"]), "import_floor_bytes": floor_import, "export_floor_bytes": floor_export,
           "stream_TB_per_s": STREAM_TBS}
    for k in ("import", "export"):
        res[k + "_floor_ms"] = round(res[k + "_floor_bytes"] / (STREAM_TBS * 1e12) * 1e3, 4)
        res[k + "_over_floor"] = round(res[k]["median_ms"] / res[k + "_floor_ms"], 2)
    store.close()
    est.close()
    lines = [json.dumps(res), "", "| call | ms per call | MB it must move | floor at 7.0 TB/s, ms | multiple of its floor |", "|---|---|---|---|---|"]
    for k in ("export", "import"):
        lines.append(f"| {k} | {cell(res[k])} | {res[k + '_floor_bytes'] / 1e6:.1f} | {res[k + '_floor_ms']:.3f} | {res[k + '_over_floor']:.2f} |")
    return lines


def mask_words(inl, n):
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return m.view(np.int32)


def part_step(S, steps, rounds, history, n_tracks=10000, new_frac=0.3):
    import torch
    dev = torch.device("cuda", 0)
    cam = camera()
    U, K = 4, 8  # (the clouds, planes and feature sets of profiles/tools/track_store_step.py)
    clouds_h = [synth.make_cloud(synth.DENSE128, seed=5, frame=f) for f in range(U)]
    planes_h = [synth.make_ground_plane(c) for c in clouds_h]
    N = clouds_h[0].shape[0]
    all_clouds = torch.empty((2, S, N, 4), dtype=torch.float32, device=dev)
    all_masks = torch.empty((2, S, (N + 31) // 32), dtype=torch.int32, device=dev)
    d_unique = [torch.from_numpy(c).to(dev) for c in clouds_h]
    m_unique = [torch.from_numpy(mask_words(p[1], N)).to(dev) for p in planes_h]
    for b in range(2):
        for q in range(S):
            all_clouds[b, q].copy_(d_unique[(b + 2 * q) % U])
            all_masks[b, q].copy_(m_unique[(b + 2 * q) % U])
    del d_unique, m_unique
    rng = np.random.default_rng(5)
    n_new = int(n_tracks * new_frac)
    sets_d = []
    for k in range(K):
        u0 = rng.integers(0, cam.width, n_tracks).astype(np.float32)
        v0 = rng.integers(100, cam.height, n_tracks).astype(np.float32)
        u1 = (u0 + rng.integers(-3, 4, n_tracks)).astype(np.float32)
        v1 = (v0 + rng.integers(-2, 3, n_tracks)).astype(np.float32)
        sets_d.append(tuple(torch.from_numpy(a).to(dev) for a in (u0, v0, u1, v1)))
    modes = ("step", "lanes", "restart")
    total = 1 + steps * len(modes) * (rounds + 1)
    ids_d, cur, next_id = [], np.tile(np.arange(n_tracks, dtype=np.int64), (S, 1)), n_tracks
    for t in range(total):
        if t:
            for q in range(S):
                cur[q, rng.choice(n_tracks, n_new, replace=False)] = np.arange(next_id, next_id + n_new)
            next_id += n_new
        ids_d.append(torch.from_numpy((cur + 7919 * np.arange(S)[:, None]).astype(np.int32)).to(dev))
    outs = [torch.empty((S, n_tracks), dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32, torch.int32)]
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    coeffs = [np.stack([planes_h[(b + 2 * q) % U][0] for q in range(S)]) for b in range(2)]
    pick = lambda b, j: [sets_d[(b + q) % K][j] for q in range(S)]  # noqa: E731
    tb = TrackletBatch(capi.params_c0(), cam, synth.T_CAM_LIDAR, S, n_tracks, list_capacity=(48, 24))
    store = tb.attach_store(history)
    prep = [tb.prepare_step(rows(all_clouds[t % 2]), coeffs[t % 2], rows(all_masks[t % 2]), rows(ids_d[t]), pick(t % 2, 0),
                            pick(t % 2, 1), pick(t % 2, 2), pick(t % 2, 3), *[rows(o) for o in outs]) for t in range(total)]
    torch.cuda.synchronize()
    est, lib = tb.est, tb.est._lib
    running = (C.c_uint8 * S)(*[1] * S)

    def lanes(f, restart):  # TrackletBatch.step, with the lanes entry whatever the flags
        est._check(lib.mld_set_clouds_planes_range_device(est._ctx, tb.bank * S, S, f["clouds"], f["n"], 16,
                                                          f["coeffs"].ctypes.data_as(C.POINTER(C.c_float)), f["masks"]))
        store._check(lib.mld_tracklets_step_lanes_device(est._ctx, store._tr, tb.bank, running, restart, f["ids"], f["u_new"],
                                                         f["v_new"], f["u_old"], f["v_old"], f["nt"], f["d_cur"], f["d_last"],
                                                         f["t_cur"], f["t_last"]))
        tb.bank = 1 - tb.bank

    def one(mode, t):
        if mode == "step":
            tb.step(prep[t])
        elif mode == "lanes":
            lanes(prep[t], None)
        else:
            lanes(prep[t], (C.c_uint8 * S)(*[int(q == t % S) for q in range(S)]))

    tb.step(prep[0])
    t, w = 1, {m: [] for m in modes}
    for r in range(rounds + 1):  # (round 0 is the warm-up)
        for mode in modes:
            est.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one(mode, t)
                t += 1
            est.synchronize()
            if r:
                w[mode].append((time.perf_counter() - t0) / steps * 1e3)
    counts = store.counts()
    assert (counts[:, 0] == n_tracks).all() and (counts[:, 5] == 0).all()
    tb.close()
    res = {"part": "step", "S": S, "steps": steps, "rounds": rounds, "max_history": history, "n_tracks": n_tracks}
    res.update({m: stat(w[m]) for m in modes})
    lines = [json.dumps(res), "", "| S | step, ms/step | lanes, ms/step | one lane restarting, ms/step |", "|---|---|---|---|",
             f"| {S} | {cell(res['step'])} | {cell(res['lanes'])} | {cell(res['restart'])} |"]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("import", "step"), required=True)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--history", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16, help="import: frames committed before the export")
    ap.add_argument("--new-frac", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=8, help="import: calls per timed window")
    ap.add_argument("--steps", type=int, default=8, help="step: steps per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per variant")
    ap.add_argument("--check", type=int, default=8, help="import: sequences whose entries are compared after the import")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    if a.part == "import":
        lines = part_import(a.seqs, a.tracks, a.history, a.frames, a.new_frac, a.reps, a.rounds, a.check)
    else:
        lines = part_step(a.seqs, a.steps, a.rounds, a.history, a.tracks, a.new_frac)
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
