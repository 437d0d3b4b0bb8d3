#!/usr/bin/env python3
"""Depth images for a batch at BASELINE config 2's shape: S sequences of 1242 x 375 pixels, HDL-64 clouds, parameters C0,
the analytic ground of the synthetic frame as the plane.

Figures from ONE process, one library, one context and stream, the arrays in GPU memory (the pixel maps, point indices
and camera-frame clouds as mld_projected_clouds_export_device wrote them for four distinct clouds, every sequence with
arrays of its own):
  full / step4        mld_depth_images_render_device at every pixel and at every fourth pixel in both directions, with
                      type_out and depth32_out
  full+f64 / step4+f64  the same with depth_out added
             Each: `--calls` calls queued back to back through the C-ABI with tables made beforehand, then ONE
             synchronisation; a host clock around that, divided by the calls.  One untimed pass as warm-up, then
             `--rounds` timed passes, alternating; median with the smallest and largest.
  floor      the bytes a call cannot avoid - the map (4 W H) and the index read once, every requested output written
             once - and their time at the 6.29 TB/s a float4 copy reaches on this GPU
  depths     the only other route to the same answer: mld_calculate_depths_device with W * H features, on `--depth-seqs`
             frame slots, timed the same way (one call, one synchronisation) and SCALED to S sequences
The image of sequence 0 is compared with that depth call before anything is timed: types equal, main-path depths
bit-equal, road depths within 1e-4 m.  Prints one JSON line and a markdown table; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import (CameraPinhole, DepthEstimator, DepthImages, GroundPlane, ProjectedClouds, capi,  # noqa: E402
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
    o_type = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(S)]
    o_d32 = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(S)]
    o_d64 = [torch.empty((H, W), dtype=torch.float64, device=dev) for _ in range(S)]
    record = torch.empty((S, DepthImages.WORDS), dtype=torch.int64, device=dev)
    di = DepthImages(est, S)
    torch.cuda.synchronize()

    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    i64 = lambda xs: (C.c_int64 * S)(*xs)  # noqa: E731
    head = (di._di, vp(maps), vp(index), i64([int(t.numel()) for t in index]), vp(cams), i64([N] * S),
            coeffs.ctypes.data_as(C.POINTER(C.c_float)), vp(masks))
    t_type, t_d32, t_d64, rec_p = vp(o_type), vp(o_d32), vp(o_d64), int(record.data_ptr())
    lib = est._lib
    grids = {"full": di.grid(None), "step4": di.grid((0, 0, 4, 4))}

    def render(grid, f64):
        def fn():
            for _ in range(calls):
                di._check(lib.mld_depth_images_render_device(*head, *grids[grid], t_d64 if f64 else None, t_d32, t_type, rec_p))
            est.synchronize()
        return fn

    variants = {"full": render("full", False), "full_f64": render("full", True), "step4": render("step4", False),
                "step4_f64": render("step4", True)}

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

    for name in ("step4_f64", "step4", "full"):  # (warm-up as well)
        variants[name]()
    variants["full_f64"]()
    depths()
    types = t_out_d[0].cpu().numpy()
    ref = d_out[0].cpu().numpy()
    got_t = o_type[0].cpu().numpy().reshape(-1).astype(np.int32)
    got_d = o_d64[0].cpu().numpy().reshape(-1)
    assert np.array_equal(got_t, types), "result types differ from the depth call"
    assert np.array_equal(got_d[types != 16], ref[types != 16]), "main-path depths are not bit-equal to the depth call"
    road_dev = float(np.abs(got_d - ref)[types == 16].max(initial=0.0))
    assert road_dev <= 1e-4, f"road depths differ by {road_dev}"
    assert np.array_equal(o_d32[0].cpu().numpy().reshape(-1), got_d.astype(np.float32)), "depth32 is not (float)depth"
    recs = DepthImages.records(record)
    mix = {capi.RESULT_TYPE_NAMES[t] if hasattr(capi, "RESULT_TYPE_NAMES") else str(t): int(recs["counts"][:, t].sum())
           for t in range(21) if int(recs["counts"][:, t].sum())}

    times = {name: [] for name in variants}
    td = []
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(clock(fn) / calls)
        td.append(clock(depths))
    med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
    stat = lambda w: {"median_ms": round(med(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}  # noqa: E731
    idx_bytes = 4 * sum(int(t.numel()) for t in index)
    ms = lambda b: b / (COPY_TBS * 1e12) * 1e3  # noqa: E731
    res = {"S": S, "W": W, "H": H, "points": N, "rounds": rounds, "calls_per_round": calls, "depths_seqs": depth_seqs,
           "depths": stat(td), "depths_scaled_ms": round(med(td) * S / depth_seqs, 1), "road_deviation_seq0_m": road_dev,
           "pixels": int(recs["n_pixels"].sum()), "n_depth": int(recs["n_depth"].sum()),
           "n_cooperative": int(recs["n_cooperative"].sum()), "type_mix": mix}
    for name in variants:
        g = grids[name.split("_")[0]]
        n = g[4] * g[5]
        per_px = 1 + 4 + (8 if name.endswith("f64") else 0)
        floor = S * (4 * W * H + per_px * n) + idx_bytes
        res[name] = dict(stat(times[name]), grid=[g[4], g[5]], floor_bytes=floor, floor_ms=round(ms(floor), 4),
                         over_floor=round(med(times[name]) / ms(floor), 1))
    res["depths_scaled_over_full_f64"] = round(res["depths_scaled_ms"] / res["full_f64"]["median_ms"], 2)
    res["depths_scaled_over_full"] = round(res["depths_scaled_ms"] / res["full"]["median_ms"], 2)
    di.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5, help="timed passes per figure")
    ap.add_argument("--calls", type=int, default=4, help="calls queued per timed pass")
    ap.add_argument("--depth-seqs", type=int, default=2, help="frame slots of the depth-call route")
    ap.add_argument("--shape", choices=("config2", "small"), default="config2",
                    help="small: 16-beam clouds (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    r = measure(a.seqs, a.rounds, a.calls, a.depth_seqs, {"config2": synth.HDL64_KITTI, "small": synth.VLP16}[a.shape])
    cell = lambda k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    names = {"full": "every pixel, type + depth32", "full_f64": "every pixel, type + depth32 + depth",
             "step4": "step 4, type + depth32", "step4_f64": "step 4, type + depth32 + depth"}
    lines = [json.dumps(r), "",
             "| S | call | grid | ms per call | byte floor, MB | floor at 6.29 TB/s, ms | call / floor |",
             "|---|---|---|---|---|---|---|"]
    for k, label in names.items():
        lines.append(f"| {r['S']} | {label} | {r[k]['grid'][0]} x {r[k]['grid'][1]} | {cell(k)} | {r[k]['floor_bytes'] / 1e6:.1f} | "
                     f"{r[k]['floor_ms']:.3f} | {r[k]['over_floor']} |")
    lines += ["",
              f"mld_calculate_depths_device with W * H features on {r['depths_seqs']} slots: "
              f"{r['depths']['median_ms']:.3f} [{r['depths']['min_ms']:.3f} .. {r['depths']['max_ms']:.3f}] ms; scaled to "
              f"{r['S']} sequences {r['depths_scaled_ms']} ms = {r['depths_scaled_over_full_f64']} x the full render with depth, "
              f"{r['depths_scaled_over_full']} x the one without",
              f"result types over all sequences: {r['type_mix']}; {r['n_cooperative']} of {r['pixels']} pixels took the cooperative route"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
