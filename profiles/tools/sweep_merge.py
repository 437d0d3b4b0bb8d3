#!/usr/bin/env python3
"""The sweep merge for a batch at two cloud shapes: S sequences of 3 sweeps of
  config2   64 x 2048 clouds (131 072 points per sweep)
  config5   128 x 4096 clouds (524 288 points per sweep)
the current sweep without a transform, the two older ones shifted by their frame distance along x, each with the gate off
(0, inf) and with a gate that drops about half of the finite records (max_range: their median range).

Figures from ONE process, one library, one context and stream, every sweep of every sequence in GPU memory of its own (four
distinct frames per sweep age, cloned):
  merge     mld_sweep_merge_run_device without and with sweep_out / orig_out.  `--calls` calls queued back to back through
            the C-ABI with tables made beforehand, then ONE synchronisation; a host clock around that, divided by the
            calls.  One untimed pass as warm-up, then `--rounds` timed passes
  floor     bytes read or written ONCE and their time at the streaming rate profiles/r6_streamread.txt records (7.0 TB/s,
            non-temporal 16-byte records): the pass reads 16 bytes per record; the write reads 16 bytes per KEPT record
            (what the kernel loads; the issue's model - every record again - is printed beside it) and the masks, and stores
            16 bytes per kept record, 5 more with both optional arrays
  torch     a straightforward torch composition of the same outputs on the same tensors - per sweep a float64 matrix
            product, the two tests, boolean indexing, then one torch.cat per sequence -, timed with torch.cuda.synchronize
            around `--torch-rounds` passes (not bit-equal in the sums' order; the comparison a user would otherwise write)
`--trace` makes the calls only, with both optional arrays (no torch, no floors): the run to put under a kernel trace, one
`--gate` per process so that the trace's per-kernel statistics are those of one gate.
Prints one JSON line and a markdown table per shape; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, SweepMerge, capi, synth  # noqa: E402

STREAM_TBS = 7.0  # profiles/r6_streamread.txt: 16-byte records, non-temporal loads
SHAPES = {"config2": synth.HDL64, "config5": synth.DENSE128, "small": synth.VLP16}
K = 3
FRAME = 6


def shift(frames_back):
    return np.array([[1.0, 0.0, 0.0, -float(frames_back)], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


def torch_merge(sweeps, mats, lo2, hi2):
    """One sequence, the outputs of the call by torch operations."""
    import torch
    parts, sw, og = [], [], []
    for j, c in enumerate(sweeps):
        xyz = c[:, :3]
        if mats[j] is not None:
            xyz = (xyz.double() @ mats[j][:, :3].T + mats[j][:, 3]).float()
        r2 = (xyz * xyz).sum(dim=1)
        keep = torch.isfinite(xyz).all(dim=1) & (r2 >= lo2) & (r2 <= hi2)
        idx = keep.nonzero(as_tuple=True)[0]
        parts.append(torch.cat([xyz[idx], c[idx, 3:4]], dim=1))
        sw.append(torch.full((idx.numel(),), j, dtype=torch.uint8, device=c.device))
        og.append(idx.to(torch.int32))
    return torch.cat(parts), torch.cat(sw), torch.cat(og)


def measure(S, shape, rounds, calls, torch_rounds, trace, only=None):
    import torch
    import sweep_merge_restatement as R
    dev = torch.device("cuda", 0)
    scanner = SHAPES[shape]
    U = 4
    frames_h = [[synth.make_cloud(scanner, seed=3, frame=FRAME + u - j) for j in range(K)] for u in range(U)]
    n_pts = frames_h[0][0].shape[0]
    mats_h = [None, shift(1), shift(2)]
    want = R.merge_sequence(frames_h[0], mats_h)
    xyz = R.merged_cloud(want)[:, :3].astype(np.float64)
    half_range = float(np.median(np.sqrt((xyz * xyz).sum(axis=1))))
    gates = {"off": (0.0, float("inf")), "half": (0.0, half_range)}
    gates = {k: v for k, v in gates.items() if only in (None, k)}

    est = DepthEstimator(device=0, max_frames=1, max_features=16)
    est.InitConfig(capi.params_c0())
    est.Initialize(CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV), synth.T_CAM_LIDAR)
    base = [[torch.from_numpy(c).to(dev) for c in row] for row in frames_h]
    sweeps = [[base[s % U][j].clone() for j in range(K)] for s in range(S)]
    merged = [torch.empty((K * n_pts, 4), dtype=torch.float32, device=dev) for _ in range(S)]
    sw_out = [torch.empty(K * n_pts, dtype=torch.uint8, device=dev) for _ in range(S)]
    og_out = [torch.empty(K * n_pts, dtype=torch.int32, device=dev) for _ in range(S)]
    record = torch.empty((S, SweepMerge.WORDS), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    vp = lambda ts: (C.c_void_p * len(ts))(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    mats_c = [None if m is None else np.ascontiguousarray(m.reshape(-1)) for m in mats_h]
    T = (C.c_void_p * (S * K))(*[mats_c[j].ctypes.data if mats_c[j] is not None else None for _ in range(S) for j in range(K)])
    pts = vp([c for row in sweeps for c in row])
    n = (C.c_int64 * (S * K))(*[n_pts] * (S * K))
    cap = (C.c_int64 * S)(*[K * n_pts] * S)
    t_merged, t_sw, t_og = vp(merged), vp(sw_out), vp(og_out)
    sm = SweepMerge(est, S, K, n_pts)
    lib = est._lib

    def run_merge(count, gate, optional):
        for _ in range(count):
            sm._check(lib.mld_sweep_merge_run_device(sm._sm, K, pts, n, 16, T, gate[0], gate[1], cap, t_merged,
                                                     t_sw if optional else None, t_og if optional else None, int(record.data_ptr())))
        est.synchronize()

    def clock(fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        return (time.perf_counter() - t0) * 1e3

    med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
    stat = lambda w: {"median_ms": round(med(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}  # noqa: E731
    ms = lambda b: b / (STREAM_TBS * 1e12) * 1e3  # noqa: E731

    res = {"S": S, "shape": shape, "sweeps": K, "points_per_sweep": n_pts, "rounds": rounds, "calls_per_round": calls, "gates": []}
    for name, gate in gates.items():
        run_merge(1, gate, True)  # (warm-up as well)
        rec = SweepMerge.records(record)
        exp = R.merge_sequence(frames_h[0], mats_h, *gate)
        assert rec[0].tobytes() == exp["record"].tobytes(), "the call's record differs from the restatement's"
        k0 = int(rec[0]["n_kept"])
        assert merged[0][:k0].cpu().numpy().view(np.uint32).tobytes() == exp["merged"].tobytes(), "the merged cloud differs"
        n_in, n_kept = int(rec["n_in"].sum()), int(rec["n_kept"].sum())
        row = {"gate": name, "max_range": gate[1], "n_in": n_in, "n_kept": n_kept, "kept_share": round(n_kept / n_in, 4)}
        if trace:
            run_merge(calls, gate, True)
            res["gates"].append(row)
            continue
        for optional in (False, True):
            w = [clock(run_merge, calls, gate, optional) / calls for _ in range(rounds)]
            masks = n_in // 8
            pass_b = 16 * n_in
            write_b = 16 * n_kept + masks + (16 + (5 if optional else 0)) * n_kept
            floor_b, issue_b = pass_b + masks + write_b, pass_b + masks + write_b + 16 * (n_in - n_kept)
            key = "with_optional" if optional else "plain"
            row[key] = dict(stat(w), floor_bytes=floor_b, floor_ms=round(ms(floor_b), 4), over_floor=round(med(w) / ms(floor_b), 2),
                            issue_floor_bytes=issue_b, issue_floor_ms=round(ms(issue_b), 4), over_issue_floor=round(med(w) / ms(issue_b), 2))
        if torch_rounds:
            lo2, hi2 = np.float32(gate[0]) ** 2, np.float32(gate[1]) ** 2
            mats_t = [None if m is None else torch.from_numpy(m).to(dev) for m in mats_h]

            def run_torch():
                outs = [torch_merge(sweeps[s], mats_t, float(lo2), float(hi2)) for s in range(S)]
                torch.cuda.synchronize()
                return outs

            outs = run_torch()
            assert int(outs[0][0].shape[0]) == k0 and np.array_equal(outs[0][2].cpu().numpy(), exp["orig"])
            del outs
            row["torch"] = stat([clock(run_torch) for _ in range(torch_rounds)])
        res["gates"].append(row)
    sm.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--shapes", default="config2,config5", help="comma-separated: config2, config5, small (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7, help="timed passes per figure")
    ap.add_argument("--calls", type=int, default=5, help="calls queued per timed pass")
    ap.add_argument("--torch-rounds", type=int, default=3, help="timed passes of the torch composition (0: none)")
    ap.add_argument("--trace", action="store_true", help="the calls only: the run for a kernel trace")
    ap.add_argument("--gate", default=None, choices=("off", "half"), help="one gate only")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the tables to this file")
    a = ap.parse_args()
    lines = []
    for shape in a.shapes.split(","):
        r = measure(a.seqs, shape, a.rounds, a.calls, a.torch_rounds, a.trace, a.gate)
        cell = lambda s: f"{s['median_ms']:.3f} [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]"  # noqa: E731
        block = [json.dumps(r), ""]
        if not a.trace:
            block += [f"{shape}: {r['S']} sequences x {r['sweeps']} sweeps x {r['points_per_sweep']} points", "",
                      "| gate | kept | outputs | ms per call | floor, MB / ms | call / floor | issue's floor, MB / ms | call / issue's floor | torch, ms |",
                      "|---|---|---|---|---|---|---|---|---|"]
            for g in r["gates"]:
                for key, label in (("plain", "merged"), ("with_optional", "merged, sweep, orig")):
                    p = g[key]
                    t = cell(g["torch"]) if "torch" in g and key == "with_optional" else ""
                    block.append(f"| {g['gate']} | {g['kept_share']:.3f} | {label} | {cell(p)} | {p['floor_bytes'] / 1e6:.0f} / {p['floor_ms']:.3f} | "
                                 f"{p['over_floor']} | {p['issue_floor_bytes'] / 1e6:.0f} / {p['issue_floor_ms']:.3f} | {p['over_issue_floor']} | {t} |")
        block.append("")
        print("\n".join(block), flush=True)
        lines += block
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
