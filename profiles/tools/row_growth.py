#!/usr/bin/env python3
"""Row-growth depths for a batch at BASELINE's two cloud shapes: S sequences of 1242 x 375 pixels, parameters C0,
  config5   128 x 4096 clouds (524 288 points), 10 000 uniform features per sequence
  config2   64 x 2048 clouds (131 072 points), 2 000 uniform features per sequence
with the growth values of the shipped parameters.yaml (count 4) and with the same values and count -1.

Figures from ONE process, one library, one context and stream, the arrays in GPU memory (visible uv, pixel maps, point
indices and camera-frame clouds as mld_projected_clouds_export_device wrote them for four distinct clouds, every sequence
with arrays of its own; four distinct feature sets):
  segment   mld_row_growth_segment_device.  `--calls` calls queued back to back through the C-ABI with tables made
            beforehand, then ONE synchronisation; a host clock around that, divided by the calls.  One untimed pass as
            warm-up, then `--rounds` timed passes.  Its floor: 16 bytes per visible point (the (u, v) pairs whose lines it
            streams), 4 per row, 16 per sequence, at the 6.29 TB/s a float4 copy reaches on this GPU
  collect   mld_row_growth_collect_device with the merge arrays and without lists, timed the same way, alternating with
  traces    mld_feature_traces_collect_device without lists and without planes on the same features and clouds: the sibling
            with one wavefront per feature
  host      the CPU restatement (tests/row_growth_restatement.py: plain Python loops, the tail through the oracle's parts)
            on `--host-features` features of each of two sequences, scaled to the call - a straightforward host
            composition of the same records, which the call's records must equal bit for bit (asserted here)
  rows      n_rows and the longest row of the distinct clouds
  type 20   on the four distinct sequences: the features the stage turns into SuccessRegionGrowing, and among them those the
            main path (the traces' main_type) had NOT given a depth
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
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, FeatureTraces, ProjectedClouds, RowGrowth, capi, synth  # noqa: E402

COPY_TBS = 6.29  # measured float4 copy bandwidth of the MI355X, TB/s
SHAPES = {"config5": (synth.DENSE128, 10000), "config2": (synth.HDL64, 2000), "small": (synth.VLP16, 300)}
ROW_CAPACITY = 1024


def measure(S, shape, rounds, calls, host_features):
    import torch
    import row_growth_restatement as RG
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
    nvis_u = torch.empty(U, dtype=torch.int64, device=dev)
    uvp = [torch.empty((n_pts, 2), dtype=torch.float64, device=dev) for _ in range(U)]
    idx = [torch.empty(n_pts, dtype=torch.int32, device=dev) for _ in range(U)]
    camc = [torch.empty((n_pts, 3), dtype=torch.float64, device=dev) for _ in range(U)]
    pmap = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(U)]
    torch.cuda.synchronize()
    pc.export(src, [n_pts] * U, nvis_u, uvp, idx, None, camc, pmap)
    est.synchronize()
    n_vis = [int(x) for x in nvis_u.cpu().numpy()]
    pc.close()
    del src
    maps = [pmap[q % U].clone() for q in range(S)]
    index = [idx[q % U][:n_vis[q % U]].clone() for q in range(S)]
    vis = [uvp[q % U][:n_vis[q % U]].clone() for q in range(S)]
    cams = [camc[q % U].clone() for q in range(S)]
    uvs = [torch.from_numpy(uv_h[q % U]).to(dev) for q in range(S)]
    nvis = torch.tensor([n_vis[q % U] for q in range(S)], dtype=torch.int64, device=dev)
    rows = [torch.empty(ROW_CAPACITY + 1, dtype=torch.int32, device=dev) for _ in range(S)]
    cloud = torch.empty((S, 4), dtype=torch.int32, device=dev)
    rec_rg = [torch.empty((n_feat, RowGrowth.WORDS), dtype=torch.int64, device=dev) for _ in range(S)]
    rec_ft = [torch.empty((n_feat, FeatureTraces.WORDS), dtype=torch.int64, device=dev) for _ in range(S)]
    depth = [torch.full((n_feat,), -1.0, dtype=torch.float64, device=dev) for _ in range(S)]
    types = [torch.zeros(n_feat, dtype=torch.int32, device=dev) for _ in range(S)]
    torch.cuda.synchronize()

    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    i64 = lambda xs: (C.c_int64 * S)(*xs)  # noqa: E731
    inputs = (vp(uvs), i64([n_feat] * S), vp(maps), vp(index), i64([int(t.numel()) for t in index]), vp(cams), i64([n_pts] * S))
    seg_args = (vp(vis), i64([int(t.shape[0]) for t in vis]), int(nvis.data_ptr()), vp(rows), int(cloud.data_ptr()))
    grow_args = (vp(vis), vp(rows), int(cloud.data_ptr()), 0, vp(rec_rg), None, vp(depth), vp(types))
    t_ft = vp(rec_ft)
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
    main_types = [FeatureTraces.records(rec_ft[q])["main_type"].copy() for q in range(U)]
    res = {"S": S, "shape": shape, "W": W, "H": H, "points": n_pts, "visible": n_vis, "features_per_seq": n_feat, "rounds": rounds,
           "calls_per_round": calls, "main_success": [int((t == 1).sum()) for t in main_types], "sets": []}
    t_traces = []
    frame = make_oracle(P)
    for name, G in (("yaml", capi.row_growth_params_yaml()),
                    ("yaml, count -1", capi.row_growth_params_yaml().replace(depth_segmentation_max_pointcount=-1))):
        rg = RowGrowth(est, S, n_feat, n_pts, ROW_CAPACITY, growth=G)

        def run_segment(n):
            for _ in range(n):
                rg._check(lib.mld_row_growth_segment_device(rg._rg, *seg_args))
            est.synchronize()

        def run_collect(n):
            for _ in range(n):
                rg._check(lib.mld_row_growth_collect_device(rg._rg, *inputs, *grow_args))
            est.synchronize()

        run_segment(1)
        run_collect(1)  # (warm-up as well)
        crec = RowGrowth.cloud_records(cloud)[:U]
        recs = [RowGrowth.records(rec_rg[q]) for q in range(U)]
        ts, tc = [], []
        for _ in range(rounds):
            ts.append(clock(run_segment, calls) / calls)
            tc.append(clock(run_collect, calls) / calls)
            t_traces.append(clock(run_traces, calls) / calls)
        # two sequences on the host: the restatement, whose records the call's must equal
        t_host = []
        for q in range(2):
            seq = RG.Sequence(pmap[q].cpu().numpy(), idx[q][:n_vis[q]].cpu().numpy(), n_vis[q], camc[q].cpu().numpy(),
                              uvp[q][:n_vis[q]].cpu().numpy(), rows[q].cpu().numpy(), crec[q]["n_rows"], crec[q]["n_vis"], ROW_CAPACITY)
            t0 = time.perf_counter()
            want, _ = RG.records(frame, P, G, seq, uv_h[q][:host_features])
            t_host.append((time.perf_counter() - t0) * 1e3)
            bad = RG.same_records(recs[q][:host_features], want)
            assert not bad, f"the call and the restatement differ in {bad} ({name}, sequence {q})"
        floor_b = sum(16 * n_vis[q % U] + 4 * (int(crec[q % U]["n_rows"]) + 1) + 16 for q in range(S))
        t20 = [int((r["type"] == 20).sum()) for r in recs]
        new20 = [int(((r["type"] == 20) & (m != 1)).sum()) for r, m in zip(recs, main_types)]
        states = {str(k): int(v) for k, v in zip(*np.unique(np.concatenate([r["state"] for r in recs]), return_counts=True))}
        res["sets"].append({"growth": name, "segment": stat(ts), "collect": stat(tc), "segment_floor_bytes": floor_b,
                            "segment_floor_ms": round(ms(floor_b), 4), "segment_over_floor": round(med(ts) / ms(floor_b), 1),
                            "host_ms_scaled": round(sum(t_host) / (2 * host_features) * n_feat * S, 0), "host_features": host_features,
                            "n_rows": crec["n_rows"].tolist(), "longest_row": crec["longest_row"].tolist(), "type20": t20,
                            "type20_without_main_success": new20, "states": states,
                            "flags": int(np.bitwise_or.reduce(np.concatenate([r["flags"] for r in recs]))),
                            "max_n_grown": int(max(r["n_grown"].max() for r in recs))})
        rg.close()
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
    ap.add_argument("--host-features", type=int, default=300, help="features per sequence the host restatement is timed on")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the tables to this file")
    a = ap.parse_args()
    lines = []
    for shape in a.shapes.split(","):
        r = measure(a.seqs, shape, a.rounds, a.calls, a.host_features)
        cell = lambda s: f"{s['median_ms']:.3f} [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]"  # noqa: E731
        block = [json.dumps(r), "",
                 f"{shape}: {r['S']} x {r['features_per_seq']} features, {r['points']} points ({r['visible']} visible in the four distinct "
                 f"clouds); traces without lists {cell(r['traces'])} ms; main-path Success per distinct sequence: {r['main_success']}", "",
                 "| growth | segment, ms per call | floor, MB / ms | segment / floor | collect, ms per call | host restatement, scaled, s | "
                 "rows; longest row | type 20 per distinct sequence (of them without a main-path Success) | states |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for p in r["sets"]:
            block.append(f"| {p['growth']} | {cell(p['segment'])} | {p['segment_floor_bytes'] / 1e6:.0f} / {p['segment_floor_ms']:.3f} | "
                         f"{p['segment_over_floor']} | {cell(p['collect'])} | {p['host_ms_scaled'] / 1e3:.0f} | {p['n_rows']}; {p['longest_row']} | "
                         f"{p['type20']} ({p['type20_without_main_success']}) | {p['states']} |")
        block.append("")
        print("\n".join(block), flush=True)
        lines += block
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
