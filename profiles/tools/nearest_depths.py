#!/usr/bin/env python3
"""Nearest-return depths for a batch at BASELINE's two cloud shapes: S sequences of 1242 x 375 pixels, parameters C0,
  config5   128 x 4096 clouds (524 288 points), 10 000 uniform features per sequence
  config2   64 x 2048 clouds (131 072 points), 2 000 uniform features per sequence
at (radius, count) = (10, 10), (24, 16), (40, 256) and - the reference's "k nearest" corner, a generous radius - (64, 10).

Figures from ONE process, one library, one context and stream, the arrays in GPU memory (the pixel maps, point indices
and camera-frame clouds as mld_projected_clouds_export_device wrote them for four distinct clouds, every sequence with
arrays of its own; four distinct feature sets):
  nearest   mld_nearest_depths_collect_device without lists.  `--calls` calls queued back to back through the C-ABI with
            tables made beforehand, then ONE synchronisation; a host clock around that, divided by the calls.  One untimed
            pass as warm-up, then `--rounds` timed passes, alternating with
  traces    mld_feature_traces_collect_device without lists and without planes on the same inputs: the existing kernel of
            the same one-wavefront-per-feature form
  stages    from the records, not from the kernel: the stage (half size 4, 8, 16, 32, 64, capped at the radius) at which
            a feature's search closed - the first whose inscribed circle holds the whole list (r r >= d2_last) for a full
            list, the last stage otherwise - as shares of the features
  floors    bytes read or written ONCE and their time at the 6.29 TB/s a float4 copy reaches on this GPU: `search` - the
            cells of the clipped square at which the search closed, 4 each, 4 (index) + 24 (point) per list entry, 16 + 64
            per feature (uv, record); `disc` - the same with the cells of the whole clipped disc, which the kernel reads
            for n_in_radius, and 4 (index) per candidate
  success   on sequence 0: MLD_Success of the window (the oracle's calculate_depth, road off) against the nearest lists
            (the CPU restatement tests/nearest_depth_restatement.py, whose records the call's must equal bit for bit -
            asserted here)
Prints one JSON line and a markdown table; run it on the GPU box."""
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
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, FeatureTraces, NearestDepths, ProjectedClouds, capi, synth  # noqa: E402

COPY_TBS = 6.29  # measured float4 copy bandwidth of the MI355X, TB/s
PAIRS = ((10, 10), (24, 16), (40, 256), (64, 10))
SHAPES = {"config5": (synth.DENSE128, 10000), "config2": (synth.HDL64, 2000), "small": (synth.VLP16, 300)}


def stage_list(R):
    out, r = [], min(4, R)
    while True:
        out.append(r)
        if r >= R:
            return out
        r = min(2 * r, R)


def closing_stage(rec, R, k):
    """Per record the half size of the stage at which the search closed."""
    stages = np.asarray(stage_list(R))
    full = rec["n_in_radius"] >= k
    first = stages[np.searchsorted(stages * stages, np.maximum(rec["d2_last"], 0))]
    return np.where(full, first, R)


def clipped_cells(cx, cy, half, W, H, R=None):
    """Cells of the image in the square of half size half[i] around (cx[i], cy[i]); with R those within the disc as well."""
    if R is None:
        nx = np.clip(np.minimum(cx + half, W - 1) - np.maximum(cx - half, 0) + 1, 0, None)
        ny = np.clip(np.minimum(cy + half, H - 1) - np.maximum(cy - half, 0) + 1, 0, None)
        return nx * ny
    total = np.zeros(cx.shape, dtype=np.int64)
    for dy in range(-R, R + 1):
        w = int(np.floor(np.sqrt(R * R - dy * dy)))
        y = cy + dy
        nx = np.clip(np.minimum(cx + w, W - 1) - np.maximum(cx - w, 0) + 1, 0, None)
        total += np.where((y >= 0) & (y < H), nx, 0)
    return total


def measure(S, shape, rounds, calls, pairs):
    import torch
    import nearest_depth_restatement as N
    from helpers import make_oracle
    dev = torch.device("cuda", 0)
    scanner, n_feat = SHAPES[shape]
    W, H = synth.KITTI_W, synth.KITTI_H
    cam = CameraPinhole(W, H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    P = capi.params_c0()
    U = 4
    clouds_h = [synth.make_cloud(scanner, seed=3, frame=f) for f in range(U)]
    uv_h = [synth.make_features(n_feat, seed=3 + f) for f in range(U)]
    n_pts = clouds_h[0].shape[0]

    est = DepthEstimator(device=0, max_frames=1, max_features=16)
    est.InitConfig(P)
    est.Initialize(cam, synth.T_CAM_LIDAR)
    pc = ProjectedClouds(est, U, n_pts)
    src = [torch.from_numpy(c).to(dev) for c in clouds_h]
    nvis = torch.empty(U, dtype=torch.int64, device=dev)
    uvp = [torch.empty((n_pts, 2), dtype=torch.float64, device=dev) for _ in range(U)]
    idx = [torch.empty(n_pts, dtype=torch.int32, device=dev) for _ in range(U)]
    camc = [torch.empty((n_pts, 3), dtype=torch.float64, device=dev) for _ in range(U)]
    pmap = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(U)]
    torch.cuda.synchronize()
    pc.export(src, [n_pts] * U, nvis, uvp, idx, None, camc, pmap)
    est.synchronize()
    n_vis = [int(x) for x in nvis.cpu().numpy()]
    pc.close()
    del uvp, src
    maps = [pmap[q % U].clone() for q in range(S)]
    index = [idx[q % U][:n_vis[q % U]].clone() for q in range(S)]
    cams = [camc[q % U].clone() for q in range(S)]
    uvs = [torch.from_numpy(uv_h[q % U]).to(dev) for q in range(S)]
    rec_nd = [torch.empty((n_feat, NearestDepths.WORDS), dtype=torch.int64, device=dev) for _ in range(S)]
    rec_ft = [torch.empty((n_feat, FeatureTraces.WORDS), dtype=torch.int64, device=dev) for _ in range(S)]
    torch.cuda.synchronize()

    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    i64 = lambda xs: (C.c_int64 * S)(*xs)  # noqa: E731
    inputs = (vp(uvs), i64([n_feat] * S), vp(maps), vp(index), i64([int(t.numel()) for t in index]), vp(cams), i64([n_pts] * S))
    t_nd, t_ft = vp(rec_nd), vp(rec_ft)
    lib = est._lib
    ft = FeatureTraces(est, S, n_feat)

    def run_traces(n):
        for _ in range(n):
            ft._check(lib.mld_feature_traces_collect_device(ft._ft, *inputs, None, None, 0, t_ft, None, None, None, None))
        est.synchronize()

    def clock(fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        return (time.perf_counter() - t0) * 1e3

    med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
    stat = lambda w: {"median_ms": round(med(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}  # noqa: E731
    ms = lambda b: b / (COPY_TBS * 1e12) * 1e3  # noqa: E731

    run_traces(1)
    window = FeatureTraces.records(rec_ft[0])
    # sequence 0 on the CPU: the window's Success by the oracle, the nearest lists by the restatement
    ref = make_oracle(P)
    ref.set_cloud(clouds_h[0])
    ref.set_ground_plane(None, None)
    _, win_types = ref.calculate_depth(uv_h[0])
    assert np.array_equal(win_types, window["main_type"]), "the traces' main types differ from the oracle's"
    pm0, index0 = ref.pixel_map(), ref.point_index()
    cam0 = np.ascontiguousarray(ref.cloud_camera_cs().T)

    res = {"S": S, "shape": shape, "W": W, "H": H, "points": n_pts, "features_per_seq": n_feat, "rounds": rounds,
           "calls_per_round": calls, "window_success_seq0": int((win_types == 1).sum()),
           "window_type2_seq0": int((win_types == 2).sum()), "pairs": []}
    t_traces = []
    for R, k in pairs:
        nd = NearestDepths(est, S, n_feat, R, k)

        def run_nearest(n):
            for _ in range(n):
                nd._check(lib.mld_nearest_depths_collect_device(nd._nd, *inputs, 0, t_nd, None))
            est.synchronize()

        run_nearest(1)  # (warm-up as well)
        recs = [NearestDepths.records(rec_nd[q]) for q in range(U)]  # (the sequences beyond repeat these)
        tn = []
        for _ in range(rounds):
            tn.append(clock(run_nearest, calls) / calls)
            t_traces.append(clock(run_traces, calls) / calls)
        want, _ = N.records(ref, P, pm0, index0, index0.size, n_pts, cam0, uv_h[0], R, k)
        bad = N.same_records(recs[0], want)
        assert not bad, f"the call and the restatement differ in {bad} at (R, k) = ({R}, {k})"
        # stages and floors over the U distinct sequences, scaled to S
        shares = {r: 0 for r in stage_list(R)}
        search_b = disc_b = 0
        for q in range(U):
            rec, uv = recs[q], uv_h[q]
            cx = np.floor(np.clip(uv[:, 0], -(R + 1), W + R)).astype(np.int64)
            cy = np.floor(np.clip(uv[:, 1], -(R + 1), H + R)).astype(np.int64)
            close = closing_stage(rec, R, k)
            for r in shares:
                shares[r] += int((close == r).sum())
            per_list = 28 * int(rec["n_nb"].sum()) + 80 * rec.size
            search_b += 4 * int(clipped_cells(cx, cy, close, W, H).sum()) + per_list
            disc_b += 4 * int(clipped_cells(cx, cy, None, W, H, R).sum()) + 4 * int(rec["n_in_radius"].sum()) + 24 * int(rec["n_nb"].sum()) + \
                80 * rec.size
        scale = S / U
        row = {"R": R, "k": k, "nearest": stat(tn),
               "stage_share": {str(r): round(n / (U * n_feat), 4) for r, n in shares.items()},
               "search_floor_bytes": int(search_b * scale), "search_floor_ms": round(ms(search_b * scale), 4),
               "disc_floor_bytes": int(disc_b * scale), "disc_floor_ms": round(ms(disc_b * scale), 4),
               "over_disc_floor": round(med(tn) / ms(disc_b * scale), 1), "over_search_floor": round(med(tn) / ms(search_b * scale), 1),
               "nearest_success_seq0": int((want["type"] == 1).sum()), "nearest_type2_seq0": int((want["type"] == 2).sum()),
               "nearest_types_seq0": {str(t): int(n) for t, n in zip(*np.unique(want["type"], return_counts=True))},
               "mean_n_in_radius": round(float(np.mean([r["n_in_radius"].mean() for r in recs])), 1)}
        res["pairs"].append(row)
        nd.close()
    res["traces"] = stat(t_traces)
    ft.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--shapes", default="config5,config2", help="comma-separated: config5, config2, small (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5, help="timed passes per figure")
    ap.add_argument("--calls", type=int, default=3, help="calls queued per timed pass")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the tables to this file")
    a = ap.parse_args()
    lines = []
    for shape in a.shapes.split(","):
        r = measure(a.seqs, shape, a.rounds, a.calls, PAIRS)
        cell = lambda s: f"{s['median_ms']:.3f} [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]"  # noqa: E731
        block = [json.dumps(r), "",
                 f"{shape}: {r['S']} x {r['features_per_seq']} features, {r['points']} points; traces without lists {cell(r['traces'])} ms; "
                 f"window Success on sequence 0: {r['window_success_seq0']} (type 2: {r['window_type2_seq0']})", "",
                 "| R | k | ms per call | closed at stage: share | search floor, MB / ms | disc floor, MB / ms | call / disc floor | "
                 "Success, type 2 on sequence 0 | mean n_in_radius |", "|---|---|---|---|---|---|---|---|---|"]
        for p in r["pairs"]:
            share = ", ".join(f"{s}: {v:.3f}" for s, v in p["stage_share"].items())
            block.append(f"| {p['R']} | {p['k']} | {cell(p['nearest'])} | {share} | {p['search_floor_bytes'] / 1e6:.0f} / {p['search_floor_ms']:.3f} | "
                         f"{p['disc_floor_bytes'] / 1e6:.0f} / {p['disc_floor_ms']:.3f} | {p['over_disc_floor']} | "
                         f"{p['nearest_success_seq0']}, {p['nearest_type2_seq0']} | {p['mean_n_in_radius']} |")
        block.append("")
        print("\n".join(block), flush=True)
        lines += block
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")

if __name__ == "__main__":
    main()
