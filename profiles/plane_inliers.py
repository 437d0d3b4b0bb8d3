#!/usr/bin/env python3
"""The ground-plane inliers of a batch (mld_plane_inliers_export_device) on BASELINE config 5's shape (256 sequences x
524 288 points, 128 x 4096), 16-byte records.

Steps, each in a child process of its own with its own time limit (a step that fails or runs out of time ends the tool;
nothing more is started on the GPU after it):
  <mask>:<filter>:<outputs>   mask    ransac  6000 set bits per sequence at random places (RANSAC takes its inliers from at
                                              most 6000 sampled points)
                                      dense   the analytic ground of the synthetic frame (synth.make_ground_plane), about
                                              the ground's share of the cloud
                              filter  off / on (ransac_plane_use_camx_treshold, ransac_plane_treshold_camx = 6 m)
                              outputs index (index_out alone) / all (with lidar_out and cam_out)
  <mask>:slots                the route without this object, filter on: per sequence mld_set_clouds_planes_range_device on
                              ONE slot + mld_get_ground_plane_inliers + mld_get_ground_plane_cloud, host clock, 16
                              sequences; the tool scales the figure to the batch
A batched figure is the time between two hipEvents on the context's stream around `--calls` (>= 20) back-to-back calls,
divided by the calls, after `--warmup` untimed calls; `--rounds` such figures, median with the smallest and largest.  It
is taken twice: `call` issues the C entry point on host tables made once, as a C caller would; `wrapper` goes through
PlaneInliers.export, which checks and lists every tensor of every sequence in Python on every call - with 256 sequences
that host work is longer than the kernels of a sparse call, and the interval between the events then measures it.
Beside it the call's byte floor at 7.0 TB/s (profiles/r6_streamread.txt): N / 8 bytes of mask per sequence, one 64-byte
line per inlier record gathered - once by the filter where it is on, once more by the write where lidar_out or cam_out
is asked for; never more than the 16 * N bytes of the cloud per such pass - and the bytes the call writes.
The outputs of sequence 0 are compared with the one-slot getters before anything is timed.
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

SCANNER, S_FULL = "DENSE128", 256
MASKS = ("ransac", "dense")
THR = 6.0
READ_TBS = 7.0  # profiles/r6_streamread.txt
LINE = 64       # bytes of a record gathered on its own


def setup(S, use):
    import torch
    from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, capi, synth
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    U = 4
    hosts = [synth.make_cloud(getattr(synth, SCANNER), seed=5, frame=f) for f in range(U)]
    N = hosts[0].shape[0]
    clouds = torch.empty((S, N, 4), dtype=torch.float32, device=dev)  # distinct HBM per sequence
    for q in range(S):
        clouds[q].copy_(torch.from_numpy(hosts[q % U]))
    P = capi.params_c0().replace(ransac_plane_use_camx_treshold=1 if use else 0, ransac_plane_treshold_camx=THR)
    est = DepthEstimator(device=0, max_frames=1)
    est.InitConfig(P)
    est.Initialize(cam, synth.T_CAM_LIDAR)
    torch.cuda.synchronize()
    return torch, dev, est, P, hosts, clouds, N


def make_masks(torch, dev, kind, hosts, S, N):
    """[S, N / 32] int32 on the device and the number of set bits per sequence."""
    from mono_lidar_depth_amd import synth
    W = (N + 31) // 32
    masks = torch.empty((S, W), dtype=torch.int32, device=dev)
    counts = []
    for q in range(S):
        bits = np.zeros(W * 32, dtype=np.uint8)
        if kind == "ransac":
            bits[np.random.default_rng(100 + q).choice(N, 6000, replace=False)] = 1
        else:
            bits[synth.make_ground_plane(hosts[q % len(hosts)])[1]] = 1
        counts.append(int(bits.sum()))
        masks[q].copy_(torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32)))
    return masks, counts


def stat(w):
    w = sorted(w)
    return {"median_ms": round(w[len(w) // 2], 4), "min_ms": round(w[0], 4), "max_ms": round(w[-1], 4)}


def set_plane(est, cloud, mask, N):
    """mld_set_clouds_planes_range_device of one sequence on slot 0."""
    coeffs = np.array([0.0, 0.0, 1.0, 1.73], dtype=np.float32)
    est._check(est._lib.mld_set_clouds_planes_range_device(
        est._ctx, 0, 1, (C.c_void_p * 1)(int(cloud.data_ptr())), (C.c_int64 * 1)(N), 16,
        coeffs.ctypes.data_as(C.POINTER(C.c_float)), (C.c_void_p * 1)(int(mask.data_ptr()))))


def step_batched(kind, filt, outputs, a):
    from mono_lidar_depth_amd import PlaneInliers
    use, S = filt == "on", S_FULL
    torch, dev, est, P, hosts, clouds, N = setup(S, use)
    masks, set_bits = make_masks(torch, dev, kind, hosts, S, N)
    cap = max(set_bits)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    counts = torch.empty((S, 2), dtype=torch.int64, device=dev)
    index = torch.empty((S, cap), dtype=torch.int32, device=dev)
    lidar = torch.empty((S, cap, 3), dtype=torch.float32, device=dev) if outputs == "all" else None
    cams = torch.empty((S, cap, 3), dtype=torch.float64, device=dev) if outputs == "all" else None
    args = (rows(clouds), rows(masks), [cap] * S, counts, rows(index), rows(lidar) if lidar is not None else None,
            rows(cams) if cams is not None else None)
    pi = PlaneInliers(est, S, N, P)
    torch.cuda.synchronize()
    pi.export(*args)
    est.synchronize()
    # sequence 0 against the one-slot getters
    cn = counts.cpu().numpy()
    set_plane(est, clouds[0], masks[0], N)
    inl = est.getGroundPlaneInliers()
    assert cn[0, 0] == inl.size == set_bits[0], (cn[0], inl.size)
    assert np.array_equal(index[0, :inl.size].cpu().numpy(), inl)
    one = np.ascontiguousarray(est.getCloudRansacPlane().T)
    assert cn[0, 1] == one.shape[0] and (use or cn[0, 1] == cn[0, 0]), (cn[0], one.shape)
    if cams is not None:
        assert np.array_equal(cams[0, :one.shape[0]].cpu().numpy().view(np.int64), one.view(np.int64))
    stream = torch.cuda.ExternalStream(est.stream, device=dev)
    # the C entry point on host tables made once - what a C caller issues - and the Python wrapper, which checks and lists
    # every tensor of every sequence on every call
    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts]) if ts is not None else None  # noqa: E731
    tables = (vp(args[0]), (C.c_int64 * S)(*[N] * S), 16, vp(args[1]), (C.c_int64 * S)(*[cap] * S), int(counts.data_ptr()),
              vp(args[4]), vp(args[5]), vp(args[6]))
    fn = est._lib.mld_plane_inliers_export_device

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

    def c_call():
        rc = fn(pi._pi, *tables)
        assert rc == 0, rc

    times = timed(c_call)
    wrapper = timed(lambda: pi.export(*args))
    n_in, n_cl = int(cn[:, 0].sum()), int(cn[:, 1].sum())
    passes = (1 if use else 0) + (1 if outputs == "all" else 0)
    gathered = sum(min(LINE * int(k), 16 * N) for k in cn[:, 0])  # (a dense mask gathers no more than the whole cloud)
    read = S * (N // 8) + passes * gathered
    written = 16 * S + 4 * n_in + ((12 * n_in + 24 * n_cl) if outputs == "all" else 0)
    res = {"step": f"{kind}:{filt}:{outputs}", "S": S, "points": N, "calls": a.calls, "rounds": a.rounds, "call": stat(times),
           "wrapper": stat(wrapper), "inliers_per_seq": round(n_in / S, 1), "cloud_per_seq": round(n_cl / S, 1), "bytes_read": read,
           "bytes_written": written, "floor_ms": round((read + written) / (READ_TBS * 1e12) * 1e3, 4)}
    res["call_over_floor"] = round(res["call"]["median_ms"] / res["floor_ms"], 2)
    pi.close()
    est.close()
    return res


def step_slots(kind, a):
    """The plane on one slot and the two getters, sequence after sequence: what a caller has without the object."""
    S = 16
    torch, dev, est, P, hosts, clouds, N = setup(S, True)
    masks, set_bits = make_masks(torch, dev, kind, hosts, S, N)

    def route():
        for q in range(S):
            set_plane(est, clouds[q], masks[q], N)
            est.getGroundPlaneInliers()
            est.getCloudRansacPlane()

    route()
    times = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        route()
        times.append((time.perf_counter() - t0) * 1e3)
    est.close()
    res = {"step": f"{kind}:slots", "S": S, "S_full": S_FULL, "points": N, "rounds": a.rounds, "route": stat(times)}
    res["scaled_to_batch_ms"] = round(res["route"]["median_ms"] * S_FULL / S, 2)
    return res


def child(step, a):
    parts = step.split(":")
    res = step_slots(parts[0], a) if parts[1] == "slots" else step_batched(parts[0], parts[1], parts[2], a)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--masks", default=",".join(MASKS))
    ap.add_argument("--no-slots", action="store_true", help="leave the one-slot route out")
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
    steps = []
    for kind in a.masks.split(","):
        steps += [f"{kind}:{filt}:{outputs}" for filt in ("off", "on") for outputs in ("index", "all")]
        if not a.no_slots:
            steps.append(f"{kind}:slots")
    results, lines = [], []
    for step in steps:
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
    table = ["", "| step | S | points | inliers / seq | cloud / seq | call, ms (hipEvents) | floor, ms | call / floor | through the Python wrapper, ms | one-slot route scaled to S, ms |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        if "call" not in r:
            continue
        sl = slots.get(r["step"].split(":")[0])
        scaled = f"{sl['scaled_to_batch_ms']:.1f} (from {sl['S']})" if sl else "-"
        c = r["call"]
        table.append(f"| {r['step']} | {r['S']} | {r['points']} | {r['inliers_per_seq']} | {r['cloud_per_seq']} | {c['median_ms']:.3f} "
                     f"[{c['min_ms']:.3f} .. {c['max_ms']:.3f}] | {r['floor_ms']:.3f} | {r['call_over_floor']} | {r['wrapper']['median_ms']:.3f} | {scaled} |")
    print("\n".join(table), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines + table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
