#!/usr/bin/env python3
"""The per-feature traces of a batch (mld_feature_traces_collect_tracks_device) beside the depth step they explain.

Shapes: `config5` = 256 sequences x 10 000 integer-pixel features on 128 x 4096 clouds (524 288 points), `config2` = 256
sequences x 2000 features on 64 x 2048 clouds; C0 parameters, the analytic ground of the synthetic frame as the plane.
Steps, each in a child process of its own with its own time limit (a step that fails or runs out of time ends the tool;
nothing more is started on the GPU after it):
  <shape>:batch   after ONE projection of the batch (mld_set_clouds_planes_range_device) and ONE export of its projected
                  clouds (mld_projected_clouds_export_device), timed in the same process on the same inputs:
                    depth      mld_tracklets_depths_device (no new tracks): the yardstick - the trace reads the same windows
                    records    the trace, records only (list_capacity 0)
                    lists32    the trace with all four lists at capacity 32
  <shape>:debug   the route without this object: per sequence the cloud and plane on ONE slot, then
                  mld_calculate_depth_debug with the features from the host; host clock, 16 sequences; the tool scales the
                  figure to the batch and labels it as scaled
A batched figure is the time between two hipEvents on the context's stream around `--calls` back-to-back calls of the C
entry point on host tables made once, divided by the calls, after `--warmup` untimed calls; `--rounds` such figures
(rounds x calls >= 100), median with the smallest and largest.  The trace kernel is the only kernel of a call besides the
descriptor upload, so the figure is its time plus a launch.
Beside it the algorithmic bytes of the call: per feature its coordinates, the map cells of its narrow window (from the
parameters and the image size) and its record; per neighbour the index and the camera-frame point (28 bytes); for the
features that reach the road the wide window's cells, its neighbours and a mask word each; the list entries written.  The
neighbour counts are those the records of the call report.  Floor = those bytes at 7.0 TB/s (profiles/r6_streamread.txt).
The records of sequence 0 are checked against the depth step's types before anything is timed.
Prints one JSON line per step and a markdown table; run it on the GPU box."""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"config5": ("DENSE128", 10000, (48, 24)), "config2": ("HDL64", 2000, None)}
S_FULL, S_DEBUG = 256, 16
READ_TBS = 7.0  # profiles/r6_streamread.txt


def stat(w):
    w = sorted(w)
    return {"median_ms": round(w[len(w) // 2], 4), "min_ms": round(w[0], 4), "max_ms": round(w[-1], 4)}


def frames(shape, S):
    """Four distinct synthetic frames with their planes, cycled over S sequences; integer-pixel features."""
    from mono_lidar_depth_amd import synth
    scanner, F, _ = SHAPES[shape]
    hosts = [synth.make_cloud(getattr(synth, scanner), seed=5, frame=f) for f in range(4)]
    planes = [synth.make_ground_plane(h) for h in hosts]
    uvs = [synth.make_features(F, seed=q, integer=True) for q in range(4)]
    return hosts, planes, uvs, F


def mask_words(n, inliers):
    bits = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
    bits[inliers] = 1
    return np.packbits(bits, bitorder="little").view(np.int32)


def step_batch(shape, a):
    import torch
    from mono_lidar_depth_amd import CameraPinhole, FeatureTraces, TrackletBatch, capi, synth
    S = a.sequences
    hosts, planes, uvs, F = frames(shape, S)
    N = hosts[0].shape[0]
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    P = capi.params_c0()
    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, F, list_capacity=SHAPES[shape][2])
    est, lib = tb.est, tb.est._lib
    clouds = torch.empty((S, N, 4), dtype=torch.float32, device=dev)  # distinct HBM per sequence
    masks = torch.empty((S, (N + 31) // 32), dtype=torch.int32, device=dev)
    u = torch.empty((S, F), dtype=torch.float32, device=dev)
    v = torch.empty((S, F), dtype=torch.float32, device=dev)
    for q in range(S):
        clouds[q].copy_(torch.from_numpy(hosts[q % 4]))
        masks[q].copy_(torch.from_numpy(mask_words(N, planes[q % 4][1])))
        u[q].copy_(torch.from_numpy(uvs[q % 4][:, 0].astype(np.float32)))
        v[q].copy_(torch.from_numpy(uvs[q % 4][:, 1].astype(np.float32)))
    coeffs = np.stack([planes[q % 4][0] for q in range(S)]).astype(np.float32)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    d_cur = torch.empty((S, F), dtype=torch.float32, device=dev)
    d_last = torch.empty((S, F), dtype=torch.float32, device=dev)
    t_cur = torch.empty((S, F), dtype=torch.int32, device=dev)
    t_last = torch.empty((S, F), dtype=torch.int32, device=dev)
    is_new = torch.zeros((S, F), dtype=torch.uint8, device=dev)
    f = tb.prepare(rows(clouds), coeffs, rows(masks), rows(u), rows(v), rows(u), rows(v), rows(is_new), rows(d_cur),
                   rows(d_last), rows(t_cur), rows(t_last))
    tb.attach_projected_clouds(N)
    tb.attach_traces()
    torch.cuda.synchronize()
    pc = tb.projected_clouds(rows(clouds), cam=True, pixel_map=True)
    tb.run(f)  # projection into bank 0 and one depth step
    est.synchronize()
    stream = torch.cuda.ExternalStream(est.stream, device=dev)
    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    nF, nN = (C.c_int64 * S)(*[F] * S), (C.c_int64 * S)(*[N] * S)

    def depth_call():
        rc = lib.mld_tracklets_depths_device(est._ctx, S, 0, 0, f["u_new"], f["v_new"], f["u_old"], f["v_old"], f["is_new"],
                                             f["nt"], f["d_cur"], f["d_last"], f["t_cur"], f["t_last"])
        assert rc == 0, rc

    trace = torch.empty((S, F, FeatureTraces.WORDS), dtype=torch.int64, device=dev)
    lists = [torch.empty((S, F, 32), dtype=torch.int32, device=dev) for _ in range(4)]
    head = (tb.feature_traces._ft, vp(rows(u)), vp(rows(v)), nF, vp(pc["pixel_map"]), vp(pc["index"]), nN, vp(pc["cam"]), nN,
            coeffs.ctypes.data_as(C.POINTER(C.c_float)), vp(rows(masks)))
    t_tab, l_tabs = vp(rows(trace)), [vp(rows(t)) for t in lists]

    def trace_call(cap):
        def call():
            rc = lib.mld_feature_traces_collect_tracks_device(*head, cap, t_tab, *(l_tabs if cap else [None] * 4))
            assert rc == 0, tb.feature_traces._last_error(tb.feature_traces._ft)
        return call

    def timed(issue):
        for _ in range(a.warmup):
            issue()
        est.synchronize()
        out = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.calls):
                issue()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / a.calls)
        return out

    # sequence 0: what the records imply against the depth step's types
    depth_call()
    trace_call(32)()
    est.synchronize()
    rec = FeatureTraces.records(trace.reshape(S * F, -1))
    r0, types0 = rec[:F], t_cur[0].cpu().numpy()
    fit = r0["road_state"] == 4
    assert np.array_equal(types0[~fit], r0["main_type"][~fit]) and np.isin(types0[fit], (16, 4, 5, 6, 7)).all()
    res = {"step": f"{shape}:batch", "S": S, "features": F, "points": N, "calls": a.calls, "rounds": a.rounds,
           "depth": stat(timed(depth_call)), "records": stat(timed(trace_call(0))), "lists32": stat(timed(trace_call(32)))}
    # the algorithmic bytes of a call
    W, H = synth.KITTI_W, synth.KITTI_H
    cells = lambda w, h, sx, sy: min(W, int(2 * (w * 0.5 * sx)) + 2) * min(H, int(2 * (h * 0.5 * sy)) + 2)  # noqa: E731
    c1 = cells(P.pixelarea_search_witdh, P.pixelarea_search_height, 1.0, 1.0)
    c2 = cells(P.pixelarea_search_witdh, P.pixelarea_search_height, 2.0, 1.5)
    reached = rec["road_state"] != 0
    read = S * F * (8 + 4 * c1) + 28 * int(rec["n_nb"].sum()) + int(reached.sum()) * 4 * c2 + 32 * int(rec["n_road"].sum())
    written = S * F * 184
    in_lists = sum(int(np.minimum(rec[k], 32).sum()) for k in ("n_nb", "n_seg", "n_road", "n_road_inl")) * 4
    for name, extra in (("records", 0), ("lists32", in_lists)):
        b = read + written + extra
        res[name].update(bytes=b, floor_ms=round(b / (READ_TBS * 1e12) * 1e3, 4),
                         over_floor=round(res[name]["median_ms"] / (b / (READ_TBS * 1e12) * 1e3), 1),
                         over_depth=round(res[name]["median_ms"] / res["depth"]["median_ms"], 2))
    res["per_feature"] = {"n_nb": round(float(rec["n_nb"].mean()), 2), "n_road": round(float(rec["n_road"][reached].mean()), 2),
                          "reached_road": round(float(reached.mean()), 3), "n_nb_max": int(rec["n_nb"].max()),
                          "n_road_max": int(rec["n_road"].max()), "cells": [c1, c2]}
    tb.close()
    est.close()
    return res


def step_debug(shape, a):
    """The cloud and plane on one slot and mld_calculate_depth_debug from the host, sequence after sequence."""
    import torch
    from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, capi, synth
    S = S_DEBUG
    hosts, planes, uvs, F = frames(shape, S)
    N = hosts[0].shape[0]
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    est = DepthEstimator(device=0, max_frames=1, max_features=F)
    est.InitConfig(capi.params_c0())
    est.Initialize(cam, synth.T_CAM_LIDAR)
    clouds = [torch.from_numpy(hosts[q % 4]).to(dev) for q in range(S)]
    masks = [torch.from_numpy(mask_words(N, planes[q % 4][1])).to(dev) for q in range(S)]
    torch.cuda.synchronize()
    depth, types, corners = np.empty(F), np.empty(F, np.int32), np.empty((F, 9))

    def route():
        for q in range(S):
            co = np.asarray(planes[q % 4][0], dtype=np.float32)
            est._check(est._lib.mld_set_clouds_planes_range_device(
                est._ctx, 0, 1, (C.c_void_p * 1)(int(clouds[q].data_ptr())), (C.c_int64 * 1)(N), 16,
                co.ctypes.data_as(C.POINTER(C.c_float)), (C.c_void_p * 1)(int(masks[q].data_ptr()))))
            est._check(est._lib.mld_calculate_depth_debug(est._ctx, 0, uvs[q % 4].ctypes.data, F, depth.ctypes.data,
                                                          types.ctypes.data, corners.ctypes.data))

    route()
    times = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        route()
        times.append((time.perf_counter() - t0) * 1e3)
    est.close()
    res = {"step": f"{shape}:debug", "S": S, "S_full": a.sequences, "features": F, "points": N, "rounds": a.rounds,
           "route": stat(times)}
    res["scaled_to_batch_ms"] = round(res["route"]["median_ms"] * a.sequences / S, 2)
    return res


def child(step, a):
    shape, kind = step.split(":")
    res = step_debug(shape, a) if kind == "debug" else step_batch(shape, a)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sequences", type=int, default=S_FULL)
    ap.add_argument("--no-debug", action="store_true", help="leave the one-slot route out")
    ap.add_argument("--calls", type=int, default=20, help="calls between the two events")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step's process may take")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the table to this file")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # (a child: one step in this process)
    a = ap.parse_args()
    if a.calls * a.rounds < 100:
        ap.error("--calls x --rounds must be at least 100")
    if a.step:
        child(a.step, a)
        return 0
    steps = []
    for shape in a.shapes.split(","):
        steps.append(f"{shape}:batch")
        if not a.no_debug:
            steps.append(f"{shape}:debug")
    results, lines = [], []
    for step in steps:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--rounds", str(a.rounds), "--sequences", str(a.sequences)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {a.step_timeout} s - stopping here", flush=True)
            return 124
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print(f"{step}: exit status {r.returncode} - stopping here\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        results.append(json.loads(got[-1][7:]))
        lines.append(got[-1][7:])
        print(got[-1][7:], flush=True)
    debug = {r["step"].split(":")[0]: r for r in results if r["step"].endswith(":debug")}
    table = ["", "| shape | S x features | depth step, ms | trace, records only, ms | x depth | floor, ms | trace, four lists of 32, ms "
             "| x depth | floor, ms | one-slot debug route SCALED to S, ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        if "depth" not in r:
            continue
        dbg = debug.get(r["step"].split(":")[0])
        scaled = f"{dbg['scaled_to_batch_ms']:.1f} (scaled from {dbg['S']})" if dbg else "-"
        cell = lambda c: f"{c['median_ms']:.3f} [{c['min_ms']:.3f} .. {c['max_ms']:.3f}]"  # noqa: E731
        table.append(f"| {r['step'].split(':')[0]} | {r['S']} x {r['features']} | {cell(r['depth'])} | {cell(r['records'])} | "
                     f"{r['records']['over_depth']} | {r['records']['floor_ms']:.3f} | {cell(r['lists32'])} | "
                     f"{r['lists32']['over_depth']} | {r['lists32']['floor_ms']:.3f} | {scaled} |")
    print("\n".join(table), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines + table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
