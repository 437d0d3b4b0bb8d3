#!/usr/bin/env python3
"""The leaving export of the GPU-resident tracklet store beside the packed export of the whole store, on BASELINE
config 5's store shape (256 sequences x 10 000 tracks x max_history 16):

  packed   mld_tracks_export_packed_device   every track of the committed frame, back to back + int64 offsets - what a
                                             caller who wants every track once and complete had to copy after every step
  leaving  mld_tracks_export_leaving_device  between a begin and its commit: the tracks that end (ids, offsets, entries)
                                             and the entries the commit overwrites (ids, one entry each)

The store alone is driven (no clouds), as profiles/tools/packed_export.py drives it: `--frames` frames of synthetic
depths, `--new-frac` of every sequence's tracks replaced by fresh ids per frame; then one more frame of the same churn
is BEGUN and not committed, and both exports are timed in that state - each with a pair of events on the context's
stream around `--reps` calls queued back to back, one warm-up window each, then `--rounds` rounds that take a window of
each in turn; the median is reported with the smallest and largest.  The calls go to the C-ABI with pointer tables made
once.  Before anything is timed the leaving export of `--check` sequences is compared with the packed one: the ended
ids are the committed ids the begun frame lacks, in the committed frame's order, and every ended track's entries are
the packed export's bit for bit; the spilled entries are the last entries of the full tracks that continue.  The bytes
are what a caller has to copy to the host: for the packed export all entries and offsets, for the leaving export the
ended tracks' ids, offsets and entries, the spilled ids and entries and the records.

`--step-seqs` > 0 adds the cost of a TrackletBatch.step with and without a sink: that many lanes on VLP-16 clouds,
`--step-tracks` tracks each, two frames whose ids differ by `--new-frac` stepped in turn (the tracks both hold are full
and spill on every step, the others end on every step), the sink armed through the C-ABI with tables made once.

Prints one JSON line per run and a markdown table; needs an MI355X."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, TrackletBatch, TrackletStore, capi, synth  # noqa: E402

stat = lambda v: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}  # noqa: E731


def camera():
    return CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)


def leaving_tables(S, buf, caps):
    """The nine output arguments of the leaving export / the sink as ctypes tables, made once."""
    table = lambda t: (C.c_void_p * S)(*[int(t[q].data_ptr()) for q in range(S)])  # noqa: E731
    i64 = lambda v: (C.c_int64 * S)(*[int(v)] * S)  # noqa: E731
    return [table(buf["ids"]), table(buf["offsets"]), table(buf["fp"]), table(buf["spill_ids"]), table(buf["spill_fp"]),
            i64(caps[0]), i64(caps[1]), i64(caps[2]), C.c_void_p(int(buf["record"].data_ptr()))]


def leaving_buffers(torch, dev, S, n, H):
    return {"ids": torch.zeros((S, n), dtype=torch.int32, device=dev), "offsets": torch.zeros((S, n + 1), dtype=torch.int64, device=dev),
            "fp": torch.zeros((S, n * H, 3), dtype=torch.float32, device=dev),
            "spill_ids": torch.zeros((S, n), dtype=torch.int32, device=dev),
            "spill_fp": torch.zeros((S, n, 3), dtype=torch.float32, device=dev),
            "record": torch.zeros((S, 4), dtype=torch.int64, device=dev)}


def measure_store(S, n, H, frames, new_frac, reps, rounds, n_check):
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
    committed = None
    for f in range(frames + 1):  # the last one is begun only
        if f:
            where = torch.rand((S, n), generator=gen, device=dev).argsort(dim=1)[:, :n_new]
            fresh = torch.arange(next_id, next_id + n_new, device=dev)[None, :] + (torch.arange(S, device=dev) * 7919)[:, None]
            ids.scatter_(1, where, fresh)
            next_id += n_new
        ids32 = ids.to(torch.int32).contiguous()
        torch.cuda.synchronize()
        store.begin(rows(ids32))
        if f == frames:
            break
        feat = [torch.rand((S, n), generator=gen, device=dev) * 1200.0 for _ in range(4)]
        depth = [torch.rand((S, n), generator=gen, device=dev) * 80.0 for _ in range(2)]
        for d in depth:
            d[torch.rand((S, n), generator=gen, device=dev) < 0.2] = -1.0
        torch.cuda.synchronize()
        store.commit(*[rows(t) for t in feat + depth])
        est.synchronize()
        committed = ids32
    begun = ids32

    cap = store.packed_capacity(n)
    fp_packed = torch.zeros((S, cap, 3), dtype=torch.float32, device=dev)
    offsets = torch.zeros((S, n + 1), dtype=torch.int64, device=dev)
    buf = leaving_buffers(torch, dev, S, n, H)
    torch.cuda.synchronize()
    lib, tr = store._lib, store._tr
    table = lambda t: (C.c_void_p * S)(*[int(t[q].data_ptr()) for q in range(S)])  # noqa: E731
    t_packed, t_off, caps = table(fp_packed), table(offsets), (C.c_int64 * S)(*[cap] * S)
    t_leave = leaving_tables(S, buf, (n, cap, n))

    def packed():
        assert lib.mld_tracks_export_packed_device(tr, t_packed, caps, t_off) == capi.MLD_OK

    def leaving():
        assert lib.mld_tracks_export_leaving_device(tr, None, *t_leave) == capi.MLD_OK

    # the same answer first
    packed()
    leaving()
    est.synchronize()
    rec = buf["record"].cpu().numpy()
    lens = offsets[:, 1:] - offsets[:, :-1]
    for q in range(min(n_check, S)):
        stays = torch.isin(committed[q], begun[q])
        n_e, n_ee, n_s = (int(x) for x in rec[q, :3])
        assert torch.equal(buf["ids"][q, :n_e], committed[q][~stays]), f"sequence {q}: ended ids"
        assert torch.equal(buf["offsets"][q, 1:n_e + 1] - buf["offsets"][q, :n_e], lens[q][~stays]), f"sequence {q}: ended lengths"
        entry_of = torch.repeat_interleave(torch.arange(n, device=dev), lens[q])  # the track of every packed entry
        want = fp_packed[q, :int(offsets[q, n])][~stays[entry_of]].view(torch.int32)
        assert n_ee == want.shape[0] and torch.equal(buf["fp"][q, :n_ee].view(torch.int32), want), f"sequence {q}: ended entries"
        full = stays & (lens[q] == H)
        assert torch.equal(buf["spill_ids"][q, :n_s], committed[q][full]), f"sequence {q}: spilled ids"
        oldest = fp_packed[q][offsets[q, 1:][full] - 1].view(torch.int32)
        assert torch.equal(buf["spill_fp"][q, :n_s].view(torch.int32), oldest), f"sequence {q}: spilled entries"

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        est.synchronize()
        return e0.elapsed_time(e1) / reps

    window(packed)
    window(leaving)
    w = {"packed": [], "leaving": []}
    for _ in range(rounds):  # (in turn: whatever else the box does hits both alike)
        w["packed"].append(window(packed))
        w["leaving"].append(window(leaving))
    entries = int(offsets[:, n].sum())
    n_e, n_ee, n_s = (int(x) for x in rec[:, :3].sum(axis=0))
    res = {"run": "store", "S": S, "n_tracks": n, "max_history": H, "frames": frames, "new_frac": new_frac, "reps": reps,
           "rounds": rounds, "stored_entries": entries, "mean_length": round(entries / (S * n), 3), "ended_tracks": n_e,
           "ended_entries": n_ee, "spilled_entries": n_s, "packed": stat(w["packed"]), "leaving": stat(w["leaving"]),
           "packed_host_bytes": entries * 12 + S * (n + 1) * 8,
           "leaving_host_bytes": n_ee * 12 + n_e * 12 + S * 8 + n_s * 16 + S * 32}
    res["leaving_over_packed_time"] = round(res["leaving"]["median_ms"] / res["packed"]["median_ms"], 4)
    res["leaving_over_packed_bytes"] = round(res["leaving_host_bytes"] / res["packed_host_bytes"], 4)
    store.close()
    est.close()
    return res


def measure_step(S, n, H, new_frac, reps, rounds):
    import torch
    dev = torch.device("cuda", 0)
    cam, rng = camera(), np.random.default_rng(3)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tb = TrackletBatch(capi.params_c0(), cam, synth.T_CAM_LIDAR, S, n)
    store = tb.attach_store(H)
    n_new = int(n * new_frac)
    tables = []
    for f in range(2):
        clouds, masks, coeffs, ids, feats = [], [], [], [], [[], [], [], []]
        for s in range(S):
            cloud = synth.make_cloud(synth.VLP16, seed=90 + s, frame=2 * f)
            co, inl = synth.make_ground_plane(cloud)
            m = np.zeros((cloud.shape[0] + 31) // 32, dtype=np.uint32)
            np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
            clouds.append(to(cloud))
            masks.append(to(m.view(np.int32)))
            coeffs.append(co)
            i = np.arange(n, dtype=np.int32)
            i[:n_new] += (f + 1) * n  # the first n_new places change hands between the two frames
            ids.append(to(i))
            u0 = rng.uniform(-2, cam.width + 2, n).astype(np.float32)
            v0 = rng.uniform(100, cam.height + 2, n).astype(np.float32)
            for k, a in enumerate((u0, v0, u0 + rng.normal(0, 3, n).astype(np.float32), v0 + rng.normal(0, 2, n).astype(np.float32))):
                feats[k].append(to(a.astype(np.float32)))
        outs = ([torch.empty(n, dtype=torch.float32, device=dev) for _ in range(S)], [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(S)])
        tables.append(tb.prepare_step(clouds, np.stack(coeffs), masks, ids, *feats, *outs))
    buf = leaving_buffers(torch, dev, S, n, H)
    t_sink = leaving_tables(S, buf, (n, n * H, n))
    stream = torch.cuda.ExternalStream(tb.est.stream, device=dev)
    lib, tr = store._lib, store._tr
    torch.cuda.synchronize()
    state = {"f": 0}

    def step(sink):
        if sink:
            assert lib.mld_tracks_set_leaving_sink(tr, *t_sink) == capi.MLD_OK
        tb.step(tables[state["f"] & 1])
        state["f"] += 1

    for _ in range(2 * H):  # until the tracks both frames hold are full
        step(False)
    tb.est.synchronize()

    def window(sink):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            step(sink)
        e1.record(stream)
        tb.est.synchronize()
        return e0.elapsed_time(e1) / reps

    window(False)
    window(True)
    rec = buf["record"].cpu().numpy().sum(axis=0)
    w = {"plain": [], "sink": []}
    for _ in range(rounds):
        w["plain"].append(window(False))
        w["sink"].append(window(True))
    res = {"run": "step", "S": S, "n_tracks": n, "max_history": H, "new_frac": new_frac, "cloud_points": int(tables[0]["n"][0]),
           "reps": reps, "rounds": rounds, "ended_tracks_per_step": int(rec[0]), "ended_entries_per_step": int(rec[1]),
           "spilled_entries_per_step": int(rec[2]), "step": stat(w["plain"]), "step_with_sink": stat(w["sink"])}
    res["sink_over_plain_time"] = round(res["step_with_sink"]["median_ms"] / res["step"]["median_ms"], 4)
    tb.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--history", type=int, default=16)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--new-frac", type=float, nargs="+", default=[0.3, 0.1], help="churn per frame; one store run each")
    ap.add_argument("--reps", type=int, default=8, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per export")
    ap.add_argument("--check", type=int, default=8, help="sequences whose leaving export is compared with the packed one")
    ap.add_argument("--step-seqs", type=int, default=16, help="lanes of the step run (0: none)")
    ap.add_argument("--step-tracks", type=int, default=2000)
    ap.add_argument("--out", default=None, help="also write the JSON lines and the tables to this file")
    a = ap.parse_args()
    cell = lambda r, k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    runs = [measure_store(a.seqs, a.tracks, a.history, a.frames, c, a.reps, a.rounds, a.check) for c in a.new_frac]
    lines = [json.dumps(r) for r in runs] + [
        "", "| S x tracks x history | churn | mean length | ended tracks | ended entries | spilled | packed, ms | leaving, ms | leaving / packed | packed, MB to the host | leaving, MB to the host |",
        "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in runs:
        lines.append(f"| {r['S']} x {r['n_tracks']} x {r['max_history']} | {r['new_frac']:.0%} | {r['mean_length']:.2f} | {r['ended_tracks']} | "
                     f"{r['ended_entries']} | {r['spilled_entries']} | {cell(r, 'packed')} | {cell(r, 'leaving')} | "
                     f"{r['leaving_over_packed_time']:.3f} | {r['packed_host_bytes'] / 1e6:.1f} | {r['leaving_host_bytes'] / 1e6:.1f} |")
    if a.step_seqs > 0:
        r = measure_step(a.step_seqs, a.step_tracks, a.history, a.new_frac[0], a.reps, a.rounds)
        lines += ["", json.dumps(r), "", "| lanes x tracks x history | cloud points | ended / spilled per step | step, ms | step with sink, ms | with / without |",
                  "|---|---|---|---|---|---|",
                  f"| {r['S']} x {r['n_tracks']} x {r['max_history']} | {r['cloud_points']} | {r['ended_tracks_per_step']} / "
                  f"{r['spilled_entries_per_step']} | {cell(r, 'step')} | {cell(r, 'step_with_sink')} | {r['sink_over_plain_time']:.3f} |"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
