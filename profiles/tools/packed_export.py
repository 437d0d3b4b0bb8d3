#!/usr/bin/env python3
"""The two exports of the GPU-resident tracklet store on BASELINE config 5's store shape (256 sequences x 10 000 tracks x
max_history 16), on histories of mixed ages:

  fixed   mld_tracks_export_device         n_tracks x max_history x 3 float32 per sequence + int32 lengths (the baseline)
  packed  mld_tracks_export_packed_device  the tracks back to back + int64 offsets

The store alone is driven (no clouds): `--frames` frames of synthetic depths, `--new-frac` of every sequence's tracks
replaced by fresh ids per frame, so that a track's length is min(age + 1, max_history) with ages geometrically
distributed.  Each export is timed with a pair of events on the context's stream around `--reps` calls queued back to
back; one such window per export is the warm-up, then `--rounds` rounds take a window of each in turn, and the median
is reported with the smallest and largest.  The calls go to the C-ABI with pointer tables made once: the Python
wrappers (TrackletStore.export / export_packed) rebuild their tables of `--seqs` pointers on every call, which at 256
sequences takes longer than either export runs, and a window around them times the host.  The bytes are what a
caller would have to copy to the host to have the message there: everything the fixed-stride export writes into (holes
included, a copy cannot skip them), against the entries and offsets of the packed one.  The packed output of `--check` sequences is compared bit for bit with the
compaction of the fixed-stride output before anything is timed.

Prints one JSON line and a markdown table; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, TrackletStore, capi, synth  # noqa: E402


def measure(S, n, H, frames, new_frac, reps, rounds, n_check):
    import torch
    dev = torch.device("cuda", 0)
    est = DepthEstimator(device=0, max_frames=1)
    est.InitConfig(capi.params_c0())
    est.Initialize(CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV), synth.T_CAM_LIDAR)
    store = TrackletStore(est, S, n, H)
    stream = torch.cuda.ExternalStream(est.stream, device=dev)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    # the frames: own id space per sequence, new_frac of the places take fresh ids every frame
    n_new = int(n * new_frac)
    ids = (torch.arange(n, dtype=torch.int64, device=dev)[None, :] + (torch.arange(S, device=dev) * 7919)[:, None]).contiguous()
    next_id = n
    for f in range(frames):
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
    counts = store.counts()
    assert (counts[:, 0] == n).all() and (counts[:, 5] == 0).all(), "the frames did not commit as planned"

    fp_fixed = torch.zeros((S, n, H, 3), dtype=torch.float32, device=dev)
    ln_fixed = torch.zeros((S, n), dtype=torch.int32, device=dev)
    cap = store.packed_capacity(n)
    fp_packed = torch.zeros((S, cap, 3), dtype=torch.float32, device=dev)
    offsets = torch.zeros((S, n + 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib, tr = store._lib, store._tr
    table = lambda t: (C.c_void_p * S)(*[int(t[q].data_ptr()) for q in range(S)])  # noqa: E731
    t_fixed, t_len, t_packed, t_off = table(fp_fixed), table(ln_fixed), table(fp_packed), table(offsets)
    caps = (C.c_int64 * S)(*[cap] * S)

    def fixed():
        assert lib.mld_tracks_export_device(tr, t_fixed, t_len) == capi.MLD_OK

    def packed():
        assert lib.mld_tracks_export_packed_device(tr, t_packed, caps, t_off) == capi.MLD_OK

    # the same answer first
    fixed()
    packed()
    est.synchronize()
    totals = offsets[:, n].clone()
    assert torch.equal(offsets[:, 1:] - offsets[:, :-1], ln_fixed.to(torch.int64)), "offsets are not the prefix of the lengths"
    for q in range(min(n_check, S)):
        keep = torch.arange(H, device=dev)[None, :] < ln_fixed[q][:, None]
        want = fp_fixed[q][keep].view(torch.int32)
        got = fp_packed[q, :int(totals[q])].view(torch.int32)
        assert torch.equal(got, want), f"sequence {q}: the packed entries are not the compaction of the fixed-stride ones"
    hist = torch.bincount(ln_fixed.flatten().to(torch.int64), minlength=H + 1).cpu().tolist()

    def window(fn):
        """ms per call of `reps` calls between two events on the context's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        est.synchronize()
        return e0.elapsed_time(e1) / reps

    window(fixed)
    window(packed)
    w = {"fixed": [], "packed": []}
    for _ in range(rounds):  # (in turn: whatever else the box does hits both alike)
        w["fixed"].append(window(fixed))
        w["packed"].append(window(packed))
    stat = lambda v: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}  # noqa: E731
    entries = int(totals.sum())
    res = {"S": S, "n_tracks": n, "max_history": H, "frames": frames, "new_frac": new_frac, "reps": reps, "rounds": rounds,
           "entries": entries, "mean_length": round(entries / (S * n), 3), "length_histogram": hist,
           "fixed": stat(w["fixed"]), "packed": stat(w["packed"]),
           "fixed_host_bytes": S * n * (H * 12 + 4), "packed_host_bytes": entries * 12 + S * (n + 1) * 8}
    res["packed_over_fixed_time"] = round(res["packed"]["median_ms"] / res["fixed"]["median_ms"], 4)
    res["packed_over_fixed_bytes"] = round(res["packed_host_bytes"] / res["fixed_host_bytes"], 4)
    store.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--history", type=int, default=16)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--new-frac", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=8, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per export")
    ap.add_argument("--check", type=int, default=8, help="sequences whose packed entries are compared with the fixed-stride ones")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    r = measure(a.seqs, a.tracks, a.history, a.frames, a.new_frac, a.reps, a.rounds, a.check)
    cell = lambda k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    lines = [json.dumps(r), "",
             "| S x tracks x history | mean length | fixed, ms | packed, ms | packed / fixed | fixed, MB to the host | packed, MB to the host |",
             "|---|---|---|---|---|---|---|",
             f"| {r['S']} x {r['n_tracks']} x {r['max_history']} | {r['mean_length']:.2f} | {cell('fixed')} | {cell('packed')} | "
             f"{r['packed_over_fixed_time']:.3f} | {r['fixed_host_bytes'] / 1e6:.1f} | {r['packed_host_bytes'] / 1e6:.1f} |"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
