#!/usr/bin/env python3
"""Coverage maps for a batch at BASELINE config 2's shape: S sequences of 1242 x 375 pixels, HDL-64 clouds, parameters C0.

Figures from ONE process, one library, one context and stream, the arrays in GPU memory (the pixel maps, point indices
and camera-frame clouds as mld_projected_clouds_export_device wrote them for four distinct clouds, every sequence with
arrays of its own):
  reach      mld_coverage_maps_collect_device with reach_out alone
  all        the five maps and 16 x 16 buckets
             Each: `--calls` calls queued back to back through the C-ABI with tables made beforehand, then ONE
             synchronisation; a host clock around that, divided by the calls.  One untimed pass as warm-up, then
             `--rounds` timed passes, alternating; median with the smallest and largest.
  floor      the bytes the issue of this object lists - the map (4 W H) and the index read once, every requested output
             written once - and their time at the 6.29 TB/s a float4 copy reaches on this GPU
  depths     the only other route to the same answer: mld_calculate_depths_device with W * H features, on `--depth-seqs`
             frame slots, timed the same way (one call, one synchronisation) and scaled to S sequences
The maps of sequence 0 are compared with the types of that depth call before anything is timed (type 2 exactly where
bit 0 is clear, type 16 only where bit 1 is set).  Prints one JSON line and a markdown table; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import (CameraPinhole, CoverageMaps, DepthEstimator, GroundPlane, ProjectedClouds, capi,  # noqa: E402
                                  synth)

COPY_TBS = 6.29  # measured float4 copy bandwidth of the MI355X, TB/s


def measure(S, rounds, calls, depth_seqs, scanner):
    import torch
    dev = torch.device("cuda", 0)
    W, H = synth.KITTI_W, synth.KITTI_H
    cam = CameraPinhole(W, H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    U = 4
    clouds_h = [synth.make_cloud(scanner, seed=5, frame=f) for f in range(U)]
    planes_h = [synth.make_ground_plane(c) for c in clouds_h]
    N = clouds_h[0].shape[0]
    words = (N + 31) // 32

    est = DepthEstimator(device=0, max_frames=depth_seqs, max_features=W * H)
    est.InitConfig(capi.params_c0())
    est.Initialize(cam, synth.T_CAM_LIDAR)

    # the projected clouds of the U distinct frames, then a copy of its own for every sequence (distinct HBM)
    pc = ProjectedClouds(est, U, N)
    src = [torch.from_numpy(c).to(dev) for c in clouds_h]
    nvis = torch.empty(U, dtype=torch.int64, device=dev)
    uv = [torch.empty((N, 2), dtype=torch.float64, device=dev) for _ in range(U)]
    idx = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(U)]
    camc = [torch.empty((N, 3), dtype=torch.float64, device=dev) for _ in range(U)]
    pmap = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(U)]
    torch.cuda.synchronize()
    pc.export(src, [N] * U, nvis, uv, idx, None, camc, pmap)
    est.synchronize()
    n_vis = [int(x) for x in nvis.cpu().numpy()]
    pc.close()
    del uv
    masks_h = []
    for c, (_, inl) in zip(clouds_h, planes_h):
        bits = np.zeros(words * 32, dtype=bool)
        bits[np.asarray(inl, dtype=np.int64)] = True
        masks_h.append(np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.int32).reshape(-1).copy())
    maps = [pmap[q % U].clone() for q in range(S)]
    index = [idx[q % U][:n_vis[q % U]].clone() for q in range(S)]
    cams = [camc[q % U].clone() for q in range(S)]
    masks = [torch.from_numpy(masks_h[q % U]).to(dev) for q in range(S)]
    coeffs = np.ascontiguousarray(np.stack([np.asarray(planes_h[q % U][0], np.float32) for q in range(S)]))
    out = {name: [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(S)] for name in CoverageMaps.MAPS}
    record = torch.empty((S, CoverageMaps.WORDS), dtype=torch.int64, device=dev)
    cm = CoverageMaps(est, S)
    n_buckets = cm.buckets(16, 16)
    buckets = [torch.empty((n_buckets, 3), dtype=torch.int32, device=dev) for _ in range(S)]
    torch.cuda.synchronize()

    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    i64 = lambda xs: (C.c_int64 * S)(*xs)  # noqa: E731
    head = (cm._cm, vp(maps), vp(index), i64([int(t.numel()) for t in index]), vp(cams), i64([N] * S),
            coeffs.ctypes.data_as(C.POINTER(C.c_float)), vp(masks))
    t_out = {name: vp(out[name]) for name in CoverageMaps.MAPS}
    rec_p, caps, t_b = int(record.data_ptr()), i64([n_buckets] * S), vp(buckets)
    lib = est._lib

    def reach():
        for _ in range(calls):
            cm._check(lib.mld_coverage_maps_collect_device(*head, None, None, None, None, t_out["reach"], rec_p, 0, 0, None, None))
        est.synchronize()

    def everything():
        for _ in range(calls):
            cm._check(lib.mld_coverage_maps_collect_device(*head, *[t_out[n] for n in CoverageMaps.MAPS], rec_p, 16, 16, caps, t_b))
        est.synchronize()

    # the other route: W * H features per frame slot
    py, px = np.divmod(np.arange(W * H), W)
    uv_all = torch.from_numpy(np.ascontiguousarray(np.stack([px, py], axis=1).astype(np.float64))).to(dev)
    for q in range(depth_seqs):
        est.setInputCloud(clouds_h[q % U], GroundPlane(*planes_h[q % U]), slot=q)
    d_out = [torch.empty(W * H, dtype=torch.float64, device=dev) for _ in range(depth_seqs)]
    t_out_d = [torch.empty(W * H, dtype=torch.int32, device=dev) for _ in range(depth_seqs)]
    torch.cuda.synchronize()

    def depths():
        est.CalculateDepths([uv_all] * depth_seqs, d_out, t_out_d)
        est.synchronize()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    everything()  # (warm-up as well)
    reach()
    depths()
    types = t_out_d[0].cpu().numpy().reshape(H, W)
    bits = out["reach"][0].cpu().numpy()
    assert np.array_equal(types == 2, (bits & 1) == 0), "type 2 and bit 0 disagree"
    assert ((bits & 2) != 0)[types == 16].all() and (types == 16).any(), "type 16 outside bit 1"
    rec = CoverageMaps.records(record)[0]

    tr, ta, td = [], [], []
    for _ in range(rounds):
        tr.append(clock(reach) / calls)
        ta.append(clock(everything) / calls)
        td.append(clock(depths))
    med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
    stat = lambda w: {"median_ms": round(med(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}  # noqa: E731
    idx_bytes = 4 * sum(int(t.numel()) for t in index)
    floor_reach = S * (4 * W * H + W * H) + idx_bytes
    floor_all = S * (4 * W * H + 5 * W * H + 12 * n_buckets) + idx_bytes
    ms = lambda b: b / (COPY_TBS * 1e12) * 1e3  # noqa: E731
    res = {"S": S, "W": W, "H": H, "points": N, "rounds": rounds, "calls_per_round": calls, "reach": stat(tr), "all": stat(ta),
           "floor_reach_bytes": floor_reach, "floor_all_bytes": floor_all, "floor_reach_ms": round(ms(floor_reach), 4),
           "floor_all_ms": round(ms(floor_all), 4), "depths_seqs": depth_seqs, "depths": stat(td),
           "depths_scaled_ms": round(med(td) * S / depth_seqs, 1),
           "record_seq0": {n: (int(rec[n]) if n != "pad_" else 0) for n in CoverageMaps.DTYPE.names}}
    res["reach_over_floor"] = round(med(tr) / ms(floor_reach), 2)
    res["all_over_floor"] = round(med(ta) / ms(floor_all), 2)
    res["depths_scaled_over_all"] = round(res["depths_scaled_ms"] / med(ta), 1)
    cm.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7, help="timed passes per figure")
    ap.add_argument("--calls", type=int, default=20, help="calls queued per timed pass")
    ap.add_argument("--depth-seqs", type=int, default=2, help="frame slots of the depth-call route")
    ap.add_argument("--shape", choices=("config2", "small"), default="config2",
                    help="small: 16-beam clouds (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    r = measure(a.seqs, a.rounds, a.calls, a.depth_seqs, {"config2": synth.HDL64_KITTI, "small": synth.VLP16}[a.shape])
    cell = lambda k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    lines = [json.dumps(r), "",
             "| S | call | ms per call | byte floor, MB | floor at 6.29 TB/s, ms | call / floor |",
             "|---|---|---|---|---|---|",
             f"| {r['S']} | reach alone | {cell('reach')} | {r['floor_reach_bytes'] / 1e6:.1f} | {r['floor_reach_ms']:.3f} | {r['reach_over_floor']} |",
             f"| {r['S']} | five maps + 16 x 16 buckets | {cell('all')} | {r['floor_all_bytes'] / 1e6:.1f} | {r['floor_all_ms']:.3f} | {r['all_over_floor']} |",
             "",
             f"mld_calculate_depths_device with W * H features on {r['depths_seqs']} slots: {cell('depths')} ms; scaled to "
             f"{r['S']} sequences {r['depths_scaled_ms']} ms = {r['depths_scaled_over_all']} x the five-map call"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
