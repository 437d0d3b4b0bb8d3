#!/usr/bin/env python3
"""The depth reports of a batch (mld_depth_reports_collect_tracks_device) on BASELINE config 5's tracklet shape: 256
sequences x 10 000 tracks, f32 u / v / depth and int32 types in GPU memory, about 60 % of the tracks with a depth.

Steps, each in a child process of its own with its own time limit (a step that fails or runs out of time ends the tool;
nothing more is started on the GPU after it):
  stats          one collect_tracks call, statistics only (two launches behind the descriptor upload)
  points         with points_out and feature_out (three launches)
  stats:python   the same two through the Python wrapper (DepthReports.collect_tracks), whose per-sequence checks and
  points:python  pointer tables are then inside the figure
  host:stats     the route without this object, statistics: synchronise, copy the types to the host (one [S, N] tensor, one
                 copy), mld_result_histogram per sequence
  host:points    ... and the interpolated clouds: the depths to the host as well, NumPy points per sequence from host u / v
A batched figure is the time between two hipEvents on the context's stream around `--calls` (>= 20) back-to-back calls,
divided by the calls, after `--warmup` untimed calls; `--rounds` such figures, median with the smallest and largest.  The
plain steps call the C-ABI with pointer tables made once, as a C++ caller would.  The host route is timed with the host
clock around work that ends with the data on the host.
Beside it the streaming floor: the bytes the call must move - depth and type of every track, the record of every sequence,
and per interpolated track u, v, depth again, the point and the feature index - at 6.3 TB/s, the HBM rate a streaming
kernel reaches on this GPU.  The outputs of every sequence are compared with the host route before anything is timed.
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

STEPS = ("stats", "points", "stats:python", "points:python", "host:stats", "host:points")
HBM_TBS = 6.3
WORDS = 24


def setup(S, N):
    import torch
    from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, capi, synth
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    rng = np.random.default_rng(5)
    host = {"u": rng.uniform(0, cam.width, (S, N)).astype(np.float32), "v": rng.uniform(0, cam.height, (S, N)).astype(np.float32)}
    valid = rng.random((S, N)) < 0.6
    host["d"] = np.where(valid, rng.uniform(2, 80, (S, N)), -1.0).astype(np.float32)
    # the types a frame of the depth path gives: Success / SuccessRoad where there is a depth, a handful of failures else
    host["t"] = np.where(valid, rng.choice([1, 16], (S, N), p=[0.7, 0.3]),
                         rng.choice([2, 3, 6, 8, 11, 13, 15], (S, N))).astype(np.int32)
    d = {k: torch.from_numpy(a).to(dev) for k, a in host.items()}
    est = DepthEstimator(device=0, max_frames=1)
    est.InitConfig(capi.params_c0())
    est.Initialize(cam, synth.T_CAM_LIDAR)
    torch.cuda.synchronize()
    return torch, dev, cam, est, host, d


def stat(w):
    w = sorted(w)
    return {"median_ms": round(w[len(w) // 2], 5), "min_ms": round(w[0], 5), "max_ms": round(w[-1], 5)}


def host_route(torch, est, cam, host, d, S, points):
    """What a caller has without the object.  Returns (reports [S, 24], list of points or None)."""
    from mono_lidar_depth_amd import capi
    lib = capi.load()
    est.synchronize()
    t = d["t"].cpu().numpy()
    report = np.zeros((S, WORDS), np.int64)
    for s in range(S):
        lib.mld_result_histogram(t[s].ctypes.data, t.shape[1], report[s].ctypes.data_as(C.POINTER(C.c_int64)))
    report[:, 22] = t.shape[1]
    if not points:
        return report, None
    depth = d["d"].cpu().numpy()
    out = []
    f, cu, cv = cam.focal_length, cam.principal_point_x, cam.principal_point_y
    for s in range(S):
        dd = depth[s].astype(np.float64)
        ok = dd >= 0
        report[s, 23] = int(ok.sum())
        u, v = np.trunc(host["u"][s][ok]).astype(np.float64), np.trunc(host["v"][s][ok]).astype(np.float64)
        out.append(np.stack([(u - cu) / f * dd[ok], (v - cv) / f * dd[ok], dd[ok]], axis=1))
    return report, out


def step_batched(step, a):
    from mono_lidar_depth_amd import DepthReports
    S, N = a.sequences, a.tracks
    points, python = step.startswith("points"), step.endswith(":python")
    torch, dev, cam, est, host, d = setup(S, N)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    report = torch.empty((S, WORDS), dtype=torch.int64, device=dev)
    pts = torch.empty((S, N, 3), dtype=torch.float64, device=dev) if points else None
    feat = torch.empty((S, N), dtype=torch.int32, device=dev) if points else None
    dr = DepthReports(est, S, N)
    py_args = (rows(d["u"]), rows(d["v"]), rows(d["d"]), rows(d["t"]), report, None, rows(pts) if points else None,
               rows(feat) if points else None)
    tab = lambda t: (C.c_void_p * S)(*[int(x.data_ptr()) for x in rows(t)]) if t is not None else None  # noqa: E731
    n_tab = (C.c_int64 * S)(*[N] * S)
    c_args = (dr._dr, tab(d["u"]), tab(d["v"]), tab(d["d"]), tab(d["t"]), n_tab, n_tab if points else None, int(report.data_ptr()),
              tab(pts), tab(feat))
    lib = dr._lib

    def call():
        if python:
            dr.collect_tracks(*py_args)
        else:
            rc = lib.mld_depth_reports_collect_tracks_device(*c_args)
            assert rc == 0, lib.mld_depth_reports_last_error(dr._dr)

    torch.cuda.synchronize()
    call()
    est.synchronize()
    # every sequence against the host route
    want, want_pts = host_route(torch, est, cam, host, d, S, True)
    got = report.cpu().numpy()
    assert np.array_equal(got, want), "records differ from the host route"
    if points:
        for s in range(S):
            m = int(got[s, 23])
            assert np.array_equal(pts[s, :m].cpu().numpy().view(np.uint64), want_pts[s].view(np.uint64)), s
            assert np.array_equal(feat[s, :m].cpu().numpy(), np.flatnonzero(host["d"][s] >= 0)), s
    stream = torch.cuda.ExternalStream(est.stream, device=dev)
    for _ in range(a.warmup):
        call()
    est.synchronize()
    times, host_us = [], []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call()
        host_us.append((time.perf_counter() - t0) / a.calls * 1e6)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / a.calls)
    valid = int(got[:, 23].sum())
    read = 8 * S * N + (12 * valid if points else 0)
    written = 192 * S + (28 * valid if points else 0)
    res = {"step": step, "S": S, "tracks": N, "calls": a.calls, "rounds": a.rounds, "call": stat(times),
           "host_enqueue_us_per_call": round(sorted(host_us)[len(host_us) // 2], 2), "interpolated_share": round(valid / (S * N), 4),
           "bytes_read": read, "bytes_written": written, "floor_ms": round((read + written) / (HBM_TBS * 1e12) * 1e3, 5)}
    res["call_over_floor"] = round(res["call"]["median_ms"] / res["floor_ms"], 2)
    dr.close()
    est.close()
    return res


def step_host(step, a):
    S, N = a.sequences, a.tracks
    points = step.endswith("points")
    torch, dev, cam, est, host, d = setup(S, N)
    host_route(torch, est, cam, host, d, S, points)
    times = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        host_route(torch, est, cam, host, d, S, points)
        times.append((time.perf_counter() - t0) * 1e3)
    est.close()
    return {"step": step, "S": S, "tracks": N, "rounds": a.rounds, "route": stat(times)}


def child(step, a):
    res = step_host(step, a) if step.startswith("host") else step_batched(step, a)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default=",".join(STEPS), help="comma list of " + ", ".join(STEPS))
    ap.add_argument("--sequences", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=50, help="calls between the two events (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a step's process may take")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the table to this file")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # (a child: one step in this process)
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    if a.step:
        child(a.step, a)
        return 0
    results, lines = [], []
    for step in a.steps.split(","):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--rounds", str(a.rounds), "--sequences", str(a.sequences), "--tracks", str(a.tracks)]
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
    routes = {r["step"].split(":")[1]: r["route"]["median_ms"] for r in results if "route" in r}
    table = ["", "| step | S | tracks | with a depth | call, ms (hipEvents) | host enqueue, us | floor, ms | call / floor | host route, ms | host route / call |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        if "call" not in r:
            continue
        route = routes.get(r["step"].split(":")[0])
        c = r["call"]
        table.append(f"| {r['step']} | {r['S']} | {r['tracks']} | {r['interpolated_share']} | {c['median_ms']:.4f} [{c['min_ms']:.4f} .. "
                     f"{c['max_ms']:.4f}] | {r['host_enqueue_us_per_call']} | {r['floor_ms']:.4f} | {r['call_over_floor']} | "
                     + (f"{route:.2f} | {route / c['median_ms']:.0f} |" if route else "- | - |"))
    print("\n".join(table), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines + table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
