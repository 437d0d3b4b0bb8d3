#!/usr/bin/env python3
"""The projected clouds of a batch (mld_projected_clouds_export_device) on BASELINE config 5's shape (256 sequences x
524 288 points, 128 x 4096) and config 2's (1024 x 131 072, 64 x 2048), 16-byte records.

Steps, each in a child process of its own with its own time limit (a step that fails or runs out of time ends the tool;
nothing more is started on the GPU after it):
  <shape>:uv       uv + index only
  <shape>:depth    with depth_out
  <shape>:map      with map_out (and depth_out)
  <shape>:cam64    with cam_out, at 64 sequences (at the full batch cam_out alone is 3.2 GB)
  <shape>:slots    the route without this object: per sequence mld_set_cloud_device + mld_get_visible_image_points +
                   mld_get_point_index on ONE slot, host clock, 16 sequences; the tool scales the figure to the batch
A batched figure is the time between two hipEvents on the context's stream around `--calls` (>= 20) back-to-back calls,
divided by the calls, after `--warmup` untimed calls; `--rounds` such figures, median with the smallest and largest.
Beside it the streaming floor: 16 * sum(N) bytes read at 7.0 TB/s (profiles/r6_streamread.txt, measured with non-temporal
loads; this object's kernels load plainly, for which that file has 6.3) plus the bytes the call writes at the same rate.
The outputs of sequence 0 are compared with the one-slot getters before anything is timed.
Prints one JSON line per step and a markdown table; run it on the GPU box."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"config5": ("DENSE128", 256), "config2": ("HDL64", 1024), "small": ("VLP16", 32)}
VARIANTS = ("uv", "depth", "map", "cam64", "slots")
READ_TBS = 7.0  # profiles/r6_streamread.txt: 16-byte records with NON-TEMPORAL loads; the same file has 6.3 for the plain
                # loads the kernels of this object use - the floor is the stricter of the two


def setup(scanner_name, S):
    import torch
    from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, capi, synth
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    U = 4
    hosts = [synth.make_cloud(getattr(synth, scanner_name), seed=5, frame=f) for f in range(U)]
    N = hosts[0].shape[0]
    clouds = torch.empty((S, N, 4), dtype=torch.float32, device=dev)  # distinct HBM per sequence
    for q in range(S):
        clouds[q].copy_(torch.from_numpy(hosts[q % U]))
    est = DepthEstimator(device=0, max_frames=1)
    est.InitConfig(capi.params_c0())
    est.Initialize(cam, synth.T_CAM_LIDAR)
    torch.cuda.synchronize()
    return torch, dev, cam, est, clouds, N


def stat(w):
    w = sorted(w)
    return {"median_ms": round(w[len(w) // 2], 4), "min_ms": round(w[0], 4), "max_ms": round(w[-1], 4)}


def step_batched(shape, variant, a):
    from mono_lidar_depth_amd import NO_PLANE, ProjectedClouds
    scanner_name, S = SHAPES[shape]
    if variant == "cam64":
        S = min(S, 64)
    torch, dev, cam, est, clouds, N = setup(scanner_name, S)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    nvis = torch.empty(S, dtype=torch.int64, device=dev)
    uv = torch.empty((S, N, 2), dtype=torch.float64, device=dev)
    index = torch.empty((S, N), dtype=torch.int32, device=dev)
    depth = torch.empty((S, N), dtype=torch.float64, device=dev) if variant in ("depth", "map") else None
    pmap = torch.empty((S, cam.height, cam.width), dtype=torch.int32, device=dev) if variant == "map" else None
    cams = torch.empty((S, N, 3), dtype=torch.float64, device=dev) if variant == "cam64" else None
    args = (rows(clouds), None, nvis, rows(uv), rows(index), rows(depth) if depth is not None else None,
            rows(cams) if cams is not None else None, rows(pmap) if pmap is not None else None)
    pc = ProjectedClouds(est, S, N)
    torch.cuda.synchronize()
    pc.export(*args)
    est.synchronize()
    # sequence 0 against the one-slot getters
    nv = nvis.cpu().numpy()
    est.setInputCloud(clouds[0], NO_PLANE)
    m = est.getVisibleCount()
    assert nv[0] == m and 0 < m < N, (nv[0], m)
    assert np.array_equal(uv[0, :m].cpu().numpy().view(np.uint64), np.ascontiguousarray(est.getPointsCloudImageCs().T).view(np.uint64))
    assert np.array_equal(index[0, :m].cpu().numpy(), est.getPointIndex())
    if pmap is not None:
        assert np.array_equal(pmap[0].cpu().numpy(), est.getPixelMap())
    stream = torch.cuda.ExternalStream(est.stream, device=dev)
    for _ in range(a.warmup):
        pc.export(*args)
    est.synchronize()
    times = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            pc.export(*args)
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / a.calls)
    total_vis = int(nv.sum())
    read = 16 * S * N
    written = 8 * S + total_vis * (16 + 4 + (8 if depth is not None else 0))
    written += S * cam.width * cam.height * 4 if pmap is not None else 0
    written += 24 * S * N if cams is not None else 0
    res = {"step": f"{shape}:{variant}", "S": S, "points": N, "calls": a.calls, "rounds": a.rounds, "call": stat(times),
           "visible_share": round(total_vis / (S * N), 4), "bytes_read": read, "bytes_written": written,
           "floor_ms": round((read + written) / (READ_TBS * 1e12) * 1e3, 4)}
    res["call_over_floor"] = round(res["call"]["median_ms"] / res["floor_ms"], 2)
    pc.close()
    est.close()
    return res


def step_slots(shape, a):
    """mld_set_cloud_device + the two getters on one slot, sequence after sequence: what a caller has without the object."""
    from mono_lidar_depth_amd import NO_PLANE
    scanner_name, S_full = SHAPES[shape]
    S = min(16, S_full)
    torch, dev, cam, est, clouds, N = setup(scanner_name, S)

    def route():
        for q in range(S):
            est.setInputCloud(clouds[q], NO_PLANE)
            est.getPointsCloudImageCs()
            est.getPointIndex()

    route()
    times = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        route()
        times.append((time.perf_counter() - t0) * 1e3)
    est.close()
    res = {"step": f"{shape}:slots", "S": S, "S_full": S_full, "points": N, "rounds": a.rounds, "route": stat(times)}
    res["scaled_to_batch_ms"] = round(res["route"]["median_ms"] * S_full / S, 2)
    return res


def child(step, a):
    shape, variant = step.split(":")
    res = step_slots(shape, a) if variant == "slots" else step_batched(shape, variant, a)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="config5,config2", help="comma list of " + ", ".join(SHAPES))
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--calls", type=int, default=20, help="calls between the two events (>= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a step's process may take")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the table to this file")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # (a child: one step in this process)
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    if a.step:
        child(a.step, a)
        return 0
    results, lines = [], []
    for shape in a.shapes.split(","):
        for variant in a.variants.split(","):
            step = f"{shape}:{variant}"
            cmd = [sys.executable, str(Path(__file__).resolve()), "--step", step, "--calls", str(a.calls), "--warmup", str(a.warmup),
                   "--rounds", str(a.rounds)]
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
    slots = {r["step"].split(":")[0]: r for r in results if r["step"].endswith(":slots")}
    table = ["", "| step | S | points | visible | call, ms (hipEvents) | floor, ms | call / floor | one-slot route scaled to S, ms |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        if "call" not in r:
            continue
        sl = slots.get(r["step"].split(":")[0])
        scaled = f"{sl['route']['median_ms'] * r['S'] / sl['S']:.1f} (from {sl['S']})" if sl else "-"
        c = r["call"]
        table.append(f"| {r['step']} | {r['S']} | {r['points']} | {r['visible_share']} | {c['median_ms']:.3f} [{c['min_ms']:.3f} .. "
                     f"{c['max_ms']:.3f}] | {r['floor_ms']:.3f} | {r['call_over_floor']} | {scaled} |")
    print("\n".join(table), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines + table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
