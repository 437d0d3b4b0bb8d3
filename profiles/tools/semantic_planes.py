#!/usr/bin/env python3
"""Semantic ground planes for a batch on BASELINE config 5's shape: S sequences x 524 288 points (128 x 4096), one
375 x 1242 label image per sequence, labels (6, 7, 8, 9), threshold 0.1.

Two figures from ONE process, one library, one context and stream, the same clouds and images in GPU memory:
  batched   one mld_semantic_planes_estimate_device call for the S sequences, the synchronisation and the read-back of
            its 32 * S bytes of records, as TrackletBatch.semantic_planes makes them
  per_slot  S calls of mld_estimate_semantic_plane_device, one per frame slot (four launches and one synchronisation
            each) - the only path to a semantic plane before the batched call; the slots' clouds are set beforehand
            (that projection is not timed: the batched call needs none)
Each is a host clock around work that ends in a synchronise; one untimed pass of each as warm-up, then `--rounds`
timed passes, alternating the two; median with the smallest and largest.  The results of the two paths are compared
(bit for bit) before anything is timed.  Prints one JSON line and a markdown row; run it on the GPU box."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, SemanticPlanes, capi, synth  # noqa: E402

LABELS = (6, 7, 8, 9)


def measure(S, rounds, thr=0.1, scanner=synth.DENSE128):
    import torch
    dev = torch.device("cuda", 0)
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    U = 4
    clouds_h = [synth.make_cloud(scanner, seed=5, frame=f) for f in range(U)]
    imgs_h = [synth.make_label_image(c) for c in clouds_h]
    N = clouds_h[0].shape[0]
    words = (N + 31) // 32
    clouds = torch.empty((S, N, 4), dtype=torch.float32, device=dev)  # distinct HBM per sequence
    images = torch.empty((S, synth.KITTI_H, synth.KITTI_W), dtype=torch.uint8, device=dev)
    for q in range(S):
        clouds[q].copy_(torch.from_numpy(clouds_h[q % U]))
        images[q].copy_(torch.from_numpy(imgs_h[q % U]))
    masks = torch.empty((S, words), dtype=torch.int32, device=dev)
    records = torch.empty((S, 8), dtype=torch.int32, device=dev)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731

    est = DepthEstimator(device=0, max_frames=S)
    est.InitConfig(capi.params_c0())
    est.Initialize(cam, synth.T_CAM_LIDAR)
    torch.cuda.synchronize()
    for q in range(S):
        est.setInputCloud(clouds[q], None, slot=q, plane_given=False)
    sp = SemanticPlanes(est, S, N)
    est.synchronize()

    def batched():
        sp.estimate(rows(clouds), rows(images), LABELS, thr, records, rows(masks))
        est.synchronize()
        return records.cpu().numpy()

    def per_slot():
        out = np.zeros((S, 8), dtype=np.int32)
        for q in range(S):
            c, n = est.estimateSemanticPlane(images[q], LABELS, thr, slot=q)
            out[q, :4] = c.view(np.int32)
            out[q, 5] = n
        return out

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    a, b = batched(), per_slot()  # (warm-up as well)
    assert not a[:, 6].any(), "a sequence without a plane"
    assert np.array_equal(a[:, :4], b[:, :4]) and np.array_equal(a[:, 5], b[:, 5]), "the two paths differ"
    m0 = masks[0].cpu().numpy().view(np.uint32)
    inl = est.getGroundPlaneInliers(0)
    assert int(np.unpackbits(m0.view(np.uint8)).sum()) == inl.size == a[0, 5]
    tb, ts = [], []
    for _ in range(rounds):
        tb.append(clock(batched))
        ts.append(clock(per_slot))
    stat = lambda w: {"median_ms": round(sorted(w)[len(w) // 2], 3), "min_ms": round(min(w), 3), "max_ms": round(max(w), 3)}  # noqa: E731
    res = {"S": S, "points": N, "image": [synth.KITTI_H, synth.KITTI_W], "rounds": rounds, "batched": stat(tb), "per_slot": stat(ts),
           "cloud_bytes_read_per_call": 2 * S * N * 16, "n_inliers_seq0": int(a[0, 5]), "n_candidates_seq0": int(a[0, 4])}
    # the two streaming passes read every cloud once each: what that is in bytes per second of the batched call
    res["batched_cloud_GBps"] = round(res["cloud_bytes_read_per_call"] / (res["batched"]["median_ms"] * 1e-3) / 1e9, 1)
    sp.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7, help="timed passes per figure")
    ap.add_argument("--small", action="store_true", help="16-beam clouds (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    r = measure(a.seqs, a.rounds, scanner=synth.VLP16 if a.small else synth.DENSE128)
    cell = lambda k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    lines = [json.dumps(r), "", "| S | points | batched call + read-back, ms | S one-slot calls, ms | cloud bytes of the batched call, GB/s |",
             "|---|---|---|---|---|", f"| {r['S']} | {r['points']} | {cell('batched')} | {cell('per_slot')} | {r['batched_cloud_GBps']} |"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
