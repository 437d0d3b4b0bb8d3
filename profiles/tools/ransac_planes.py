#!/usr/bin/env python3
"""RANSAC ground planes for a batch on BASELINE config 5's shape (S sequences x 524 288 points, 128 x 4096) and config
2's (S x 131 072, 64 x 2048), parameters C0.

Figures from ONE process, one library, one context and stream, the same clouds in GPU memory:
  batched    one mld_ransac_planes_estimate_device call for the S sequences, the synchronisation and the read-back of
             its 32 * S bytes of records, as TrackletBatch.ransac_planes makes them
  per_slot   (a) S calls of mld_estimate_ground_plane, one per frame slot (one synchronisation each) - the only other
             path a caller of the two-bank slot layout has; the slots' clouds are set beforehand (that projection is
             not timed: the batched call needs none)
  in_context (b) the k_rs_batch leg of mld_set_clouds_estimate_planes_device: that call and a synchronisation, minus
             mld_set_clouds_planes_device with the planes supplied (the same projection without the estimation).
             Reported, not compared against a bound.
Each is a host clock around work that ends in a synchronise; one untimed pass of each as warm-up, then `--rounds` timed
passes, alternating; median with the smallest and largest.  The batched records are compared (bit for bit) with the
one-slot path's before anything is timed.  Prints one JSON line and a markdown row; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, RansacPlanes, capi, synth  # noqa: E402


def measure(S, rounds, scanner):
    import torch
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    U = 4
    clouds_h = [synth.make_cloud(scanner, seed=5, frame=f) for f in range(U)]
    N = clouds_h[0].shape[0]
    words = (N + 31) // 32
    clouds = torch.empty((S, N, 4), dtype=torch.float32, device=dev)  # distinct HBM per sequence
    for q in range(S):
        clouds[q].copy_(torch.from_numpy(clouds_h[q % U]))
    masks = torch.empty((S, words), dtype=torch.int32, device=dev)
    records = torch.empty((S, 8), dtype=torch.int32, device=dev)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    seeds = [1000 + 17 * q for q in range(S)]

    est = DepthEstimator(device=0, max_frames=S)
    est.InitConfig(capi.params_c0())
    est.Initialize(cam, synth.T_CAM_LIDAR)
    torch.cuda.synchronize()
    rp = RansacPlanes(est, S, N)
    est.synchronize()

    def batched():
        rp.estimate(rows(clouds), seeds, records, rows(masks))
        est.synchronize()
        return records.cpu().numpy()

    def project():  # what per_slot() works on
        for q in range(S):
            est.setInputCloud(clouds[q], None, slot=q, plane_given=False)
        est.synchronize()

    def per_slot():
        out = np.zeros((S, 8), dtype=np.int32)
        for q in range(S):
            c, n = est.estimateGroundPlane(q, seeds[q])
            out[q, :4] = c.view(np.int32)
            out[q, 4] = n
        return out

    def in_context():
        est.setInputCloudsEstimatePlanes(rows(clouds), seeds)
        est.synchronize()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    a = batched()  # (warm-up as well)
    project()
    b = per_slot()
    assert not a[:, 6].any(), "a sequence without a plane"
    assert np.array_equal(a[:, :5], b[:, :5]), "the two paths differ"
    m0 = masks[0].cpu().numpy().view(np.uint32)
    inl = est.getGroundPlaneInliers(0)
    assert np.array_equal(np.flatnonzero(np.unpackbits(m0.view(np.uint8), bitorder="little")), inl)
    coeffs = np.ascontiguousarray(a[:, :4]).view(np.float32)

    c_ptrs = (C.c_void_p * S)(*[int(clouds[q].data_ptr()) for q in range(S)])
    m_ptrs = (C.c_void_p * S)(*[int(masks[q].data_ptr()) for q in range(S)])
    c_n = (C.c_int64 * S)(*([N] * S))

    def supplied():
        est._check(est._lib.mld_set_clouds_planes_device(est._ctx, S, c_ptrs, c_n, 16,
                                                         coeffs.ctypes.data_as(C.POINTER(C.c_float)), m_ptrs))
        est.synchronize()

    in_context()
    supplied()
    tb, ts, tc, tp = [], [], [], []
    for _ in range(rounds):
        tb.append(clock(batched))
        project()
        ts.append(clock(per_slot))
        tc.append(clock(in_context))
        tp.append(clock(supplied))
    med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
    stat = lambda w: {"median_ms": round(med(w), 3), "min_ms": round(min(w), 3), "max_ms": round(max(w), 3)}  # noqa: E731
    leg = [x - y for x, y in zip(tc, tp)]
    res = {"S": S, "points": N, "rounds": rounds, "batched": stat(tb), "per_slot": stat(ts), "estimate_in_context": stat(tc),
           "supplied_planes": stat(tp), "k_rs_batch_leg": stat(leg), "iterations_seq0": int(a[0, 5]), "n_inliers_seq0": int(a[0, 4])}
    res["per_slot_over_batched"] = round(med(ts) / med(tb), 2)
    res["batched_over_k_rs_batch_leg"] = round(med(tb) / med(leg), 2) if med(leg) > 0 else None
    rp.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7, help="timed passes per figure")
    ap.add_argument("--shape", choices=("config5", "config2", "small"), default="config5",
                    help="small: 16-beam clouds (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    r = measure(a.seqs, a.rounds, {"config5": synth.DENSE128, "config2": synth.HDL64, "small": synth.VLP16}[a.shape])
    cell = lambda k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    lines = [json.dumps(r), "",
             "| S | points | batched call + read-back, ms | (a) S one-slot calls, ms | (b) k_rs_batch leg, ms | (a) / batched | batched / (b) |",
             "|---|---|---|---|---|---|---|",
             f"| {r['S']} | {r['points']} | {cell('batched')} | {cell('per_slot')} | {cell('k_rs_batch_leg')} | "
             f"{r['per_slot_over_batched']} | {r['batched_over_k_rs_batch_leg']} |"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
