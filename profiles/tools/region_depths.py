#!/usr/bin/env python3
"""Region depths for a batch at BASELINE config 5's clouds: S sequences of 1242 x 375 pixels, 128-beam clouds of 524 288
points, parameters C0, 64 boxes per sequence.

The boxes (seed 2024, every sequence its own draw): height h = exp(N(ln 45, 0.7)) pixels clipped to 8 .. 370, width
w = h * exp(N(ln 1.4, 0.45)) clipped to 8 .. 1200, centre x uniform over the image, centre y = N(190, 40) - cars and
pedestrians around the horizon, a few boxes of half the image.  Boxes may cross the image's border (the call clips them).

Figures from ONE process, one library, one context and stream, the arrays in GPU memory (the pixel maps, point indices
and camera-frame clouds as mld_projected_clouds_export_device wrote them for four distinct clouds, every sequence with
arrays of its own):
  masks, plain   mld_region_depths_collect_device with and without the ground masks (the analytic ground of the synthetic
                 frame).  Each: `--calls` calls queued back to back through the C-ABI with tables made beforehand, then
                 ONE synchronisation; a host clock around that, divided by the calls.  One untimed pass as warm-up, then
                 `--rounds` timed passes, alternating; median with the smallest and largest.
  floor          the bytes a box's cells and points hold - 4 per cell of the clipped box (map), 4 (index) + 8 (z) per
                 occupied cell, 4 more (mask word) with masks, 80 per record -, each read or written ONCE, and their time
                 at the 6.29 TB/s a float4 copy reaches on this GPU
  torch          a straightforward torch implementation of the same record on the same arrays: per box a slice of the map,
                 gathers, boolean filters, torch.sort for minimum / median / maximum, torch.bincount for the histogram
                 and one device-to-host copy of the bins for the scan with its early returns; on the boxes of
                 `--torch-seqs` sequences, checked bit for bit against the call's records, scaled to S
  order, alone   the same boxes without masks with every sequence's boxes sorted by clipped area, the largest first and the
                 largest last (blocks start in the caller's order), and a call of ONE full-image box per sequence: what a
                 long block costs and where it hurts
With --trace nothing is timed: one warm-up and three calls of each variant, masks first, for a rocprofv3 --kernel-trace
run.  Prints one JSON line and a markdown table; run it on the GPU box."""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, DepthEstimator, ProjectedClouds, RegionDepths, capi, synth  # noqa: E402

COPY_TBS = 6.29  # measured float4 copy bandwidth of the MI355X, TB/s
BOX_SEED = 2024


def draw_boxes(S, per_seq, W, H):
    rng = np.random.default_rng(BOX_SEED)
    h = np.clip(np.exp(rng.normal(math.log(45.0), 0.7, (S, per_seq))), 8, 370)
    w = np.clip(h * np.exp(rng.normal(math.log(1.4), 0.45, (S, per_seq))), 8, 1200)
    cx = rng.uniform(0, W, (S, per_seq))
    cy = rng.normal(190.0, 40.0, (S, per_seq))
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=-1)
    return np.ascontiguousarray(np.floor(b).astype(np.int32))


def torch_records(pm, index, cam, mask_bits, boxes, bin_w, min_count):
    """The straightforward implementation: one box at a time, torch operations on the device, one host read per box."""
    import torch
    H, W = pm.shape
    out = np.zeros(boxes.shape[0], dtype=RegionDepths.DTYPE)
    for i, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        r = out[i]
        r["nearest_orig"], r["clip"] = -1, -1
        r["flags"] = capi.MLD_REGION_FLAG_HAS_MASK if mask_bits is not None else 0
        for k in ("z_min", "z_max", "z_median", "hist_lower", "hist_higher"):
            r[k] = -1.0
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if x1 < x0 or y1 < y0 or cx1 < cx0 or cy1 < cy0:
            r["flags"] |= capi.MLD_REGION_FLAG_EMPTY_BOX
            continue
        r["clip"] = (cx0, cy0, cx1, cy1)
        m = pm[cy0:cy1 + 1, cx0:cx1 + 1].reshape(-1)
        orig = index[m[m >= 0].long()].long()
        z = cam[orig, 2]
        if mask_bits is not None:
            g = mask_bits[orig]
            r["n_ground"] = int(g.sum())
            orig, z = orig[~g], z[~g]
        n = int(z.numel())
        r["n_points"] = n
        if n == 0:
            continue
        zs, order = torch.sort(z, stable=True)
        r["z_min"], r["z_max"], r["z_median"] = float(zs[0]), float(zs[-1]), float(zs[(n - 1) // 2])
        r["nearest_orig"] = int(orig[order[0]])
        bin_count = int(math.ceil(float(zs[-1])) / bin_w + 1)
        if bin_count <= 1:
            continue
        idx = torch.clamp((torch.clamp(z, max=1e10) / bin_w).abs(), max=float(bin_count) - 1.0).long()
        counts = torch.bincount(idx, minlength=bin_count).cpu().numpy()
        best, best_val, value = -1, -1, 0
        for b in range(bin_count):
            last, value = value, int(counts[b])
            if value > best_val and value >= min_count:
                best_val, best = value, b
            elif value < best_val:
                break
            if last > 0 and value == 0:
                best = -1
                break
        if best < 0:
            continue
        lo, hi = best * bin_w - 0.0 * bin_w, best * bin_w + 1.0 * bin_w
        r["flags"] |= capi.MLD_REGION_FLAG_HIST_FOUND
        r["hist_lower"], r["hist_higher"] = lo, hi
        r["n_seg"] = int(((z >= lo) & (z < hi)).sum())
    return out


def measure(S, per_seq, rounds, calls, torch_seqs, scanner, trace):
    import torch
    dev = torch.device("cuda", 0)
    W, H = synth.KITTI_W, synth.KITTI_H
    cam = CameraPinhole(W, H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    P = capi.params_c0()
    U = 4
    clouds_h = [synth.make_cloud(scanner, seed=5, frame=f) for f in range(U)]
    planes_h = [synth.make_ground_plane(c) for c in clouds_h]
    N = clouds_h[0].shape[0]
    words = (N + 31) // 32

    est = DepthEstimator(device=0, max_frames=1, max_features=16)
    est.InitConfig(P)
    est.Initialize(cam, synth.T_CAM_LIDAR)
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
    del uv, src
    bits_h, masks_h = [], []
    for _, inl in planes_h:
        bits = np.zeros(words * 32, dtype=bool)
        bits[np.asarray(inl, dtype=np.int64)] = True
        bits_h.append(bits[:N].copy())
        masks_h.append(np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.int32).reshape(-1).copy())
    maps = [pmap[q % U].clone() for q in range(S)]
    index = [idx[q % U][:n_vis[q % U]].clone() for q in range(S)]
    cams = [camc[q % U].clone() for q in range(S)]
    masks = [torch.from_numpy(masks_h[q % U]).to(dev) for q in range(S)]
    boxes_h = draw_boxes(S, per_seq, W, H)
    boxes = [torch.from_numpy(boxes_h[q]).to(dev) for q in range(S)]
    rec = {k: [torch.empty((per_seq, RegionDepths.WORDS), dtype=torch.int64, device=dev) for _ in range(S)] for k in ("masks", "plain")}
    rd = RegionDepths(est, S, per_seq)
    torch.cuda.synchronize()

    vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
    i64 = lambda xs: (C.c_int64 * S)(*xs)  # noqa: E731
    head = (rd._rd, vp(maps), vp(index), i64([int(t.numel()) for t in index]), vp(cams), i64([N] * S))
    tail = (vp(boxes), i64([per_seq] * S))
    t_mask, t_rec = vp(masks), {k: vp(rec[k]) for k in rec}
    lib = est._lib

    def run(kind, n):
        for _ in range(n):
            rd._check(lib.mld_region_depths_collect_device(*head, t_mask if kind == "masks" else None, *tail, t_rec[kind]))
        est.synchronize()

    def clock(fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        return (time.perf_counter() - t0) * 1e3

    run("masks", 1)  # (warm-up as well)
    run("plain", 1)
    if trace:
        run("masks", 3)
        run("plain", 3)
        rd.close()
        est.close()
        return None
    got = {k: np.concatenate([RegionDepths.records(t) for t in rec[k]]) for k in rec}

    # the comparator, on the first sequences, checked against the call
    bw, mc = P.histogram_segmentation_bin_witdh, P.histogram_segmentation_min_pointcount
    bits_d = [torch.from_numpy(b).to(dev) for b in bits_h]
    torch.cuda.synchronize()

    def comparator(kind):
        out = []
        for q in range(torch_seqs):
            out.append(torch_records(maps[q], index[q], cams[q], bits_d[q % U] if kind == "masks" else None, boxes_h[q], bw, mc))
        torch.cuda.synchronize()
        return np.concatenate(out)

    cmp_ms = {}
    for kind in ("masks", "plain"):
        comparator(kind)  # (warm-up)
        t0 = time.perf_counter()
        mine = comparator(kind)
        cmp_ms[kind] = (time.perf_counter() - t0) * 1e3
        theirs = got[kind][:torch_seqs * per_seq]
        for name in RegionDepths.DTYPE.names:
            a, b = np.ascontiguousarray(mine[name]), np.ascontiguousarray(theirs[name])
            same = a.view(np.int64) == b.view(np.int64) if a.dtype.kind == "f" else a == b
            assert np.all(same), f"torch comparator and the call differ in {name} ({kind})"

    # the same boxes in another order, and one full-image box per sequence
    bb = boxes_h.astype(np.int64)
    area = (np.clip(np.minimum(bb[..., 2], W - 1) - np.maximum(bb[..., 0], 0) + 1, 0, None) *
            np.clip(np.minimum(bb[..., 3], H - 1) - np.maximum(bb[..., 1], 0) + 1, 0, None))
    extra = {}
    for name, key in (("first", -area), ("last", area)):
        order = np.argsort(key, axis=1, kind="stable")
        bx = [torch.from_numpy(np.ascontiguousarray(boxes_h[q][order[q]])).to(dev) for q in range(S)]
        extra[name] = (bx, vp(bx), i64([per_seq] * S))
    whole = [torch.tensor([[0, 0, W - 1, H - 1]], dtype=torch.int32, device=dev) for _ in range(S)]
    extra["alone"] = (whole, vp(whole), i64([1] * S))
    rec_x = [torch.empty((per_seq, RegionDepths.WORDS), dtype=torch.int64, device=dev) for _ in range(S)]
    t_rec_x = vp(rec_x)
    torch.cuda.synchronize()

    def run_extra(name, n):
        for _ in range(n):
            rd._check(lib.mld_region_depths_collect_device(*head, None, extra[name][1], extra[name][2], t_rec_x))
        est.synchronize()

    for name in extra:
        run_extra(name, 1)
    alone_rec = RegionDepths.records(rec_x[0])[0]
    tm, tp, tx = [], [], {name: [] for name in extra}
    for _ in range(rounds):
        tm.append(clock(run, "masks", calls) / calls)
        tp.append(clock(run, "plain", calls) / calls)
        for name in extra:
            tx[name].append(clock(run_extra, name, calls) / calls)
    med = lambda w: sorted(w)[len(w) // 2]  # noqa: E731
    stat = lambda w: {"median_ms": round(med(w), 4), "min_ms": round(min(w), 4), "max_ms": round(max(w), 4)}  # noqa: E731
    ms = lambda b: b / (COPY_TBS * 1e12) * 1e3  # noqa: E731
    res = {"S": S, "W": W, "H": H, "points": N, "boxes_per_seq": per_seq, "box_seed": BOX_SEED, "rounds": rounds,
           "calls_per_round": calls, "masks": stat(tm), "plain": stat(tp), "torch_seqs": torch_seqs,
           "plain_largest_first": stat(tx["first"]), "plain_largest_last": stat(tx["last"]), "full_image_alone": stat(tx["alone"]),
           "full_image_points": int(alone_rec["n_points"])}
    for kind in ("masks", "plain"):
        r = got[kind]
        clip = r["clip"].astype(np.int64)
        cells = np.where(r["flags"] & capi.MLD_REGION_FLAG_EMPTY_BOX, 0, (clip[:, 2] - clip[:, 0] + 1) * (clip[:, 3] - clip[:, 1] + 1))
        occupied = r["n_points"].astype(np.int64) + r["n_ground"]
        floor = int(4 * cells.sum() + (16 if kind == "masks" else 12) * occupied.sum() + 80 * r.size)
        res[kind].update(floor_bytes=floor, floor_ms=round(ms(floor), 4), over_floor=round(med(tm if kind == "masks" else tp) / ms(floor), 1),
                         torch_ms=round(cmp_ms[kind], 1), torch_scaled_ms=round(cmp_ms[kind] * S / torch_seqs, 0),
                         torch_over_call=round(cmp_ms[kind] * S / torch_seqs / med(tm if kind == "masks" else tp), 0))
        res[kind]["boxes"] = {"cells_total": int(cells.sum()), "cells_median": int(np.median(cells)), "cells_max": int(cells.max()),
                              "occupied_total": int(occupied.sum()), "points_median": int(np.median(r["n_points"])),
                              "points_max": int(r["n_points"].max()), "empty": int((cells == 0).sum()),
                              "no_point": int((r["n_points"] == 0).sum()),
                              "beyond_list": int((r["n_points"] > RegionDepths.LIST_CAPACITY).sum()),
                              "hist_found": int(((r["flags"] & capi.MLD_REGION_FLAG_HIST_FOUND) != 0).sum()),
                              "hist_capped": int(((r["flags"] & capi.MLD_REGION_FLAG_HIST_CAPPED) != 0).sum()),
                              "bad_input": int(((r["flags"] & capi.MLD_REGION_FLAG_BAD_INPUT) != 0).sum())}
    rd.close()
    est.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=64, help="boxes per sequence")
    ap.add_argument("--rounds", type=int, default=7, help="timed passes per figure")
    ap.add_argument("--calls", type=int, default=10, help="calls queued per timed pass")
    ap.add_argument("--torch-seqs", type=int, default=2, help="sequences the torch comparator works through")
    ap.add_argument("--shape", choices=("config5", "small"), default="config5",
                    help="small: 16-beam clouds (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--trace", action="store_true", help="a warm-up and three calls of each variant, masks first; nothing timed")
    ap.add_argument("--out", default=None, help="also write the JSON line and the table to this file")
    a = ap.parse_args()
    r = measure(a.seqs, a.boxes, a.rounds, a.calls, a.torch_seqs, {"config5": synth.DENSE128, "small": synth.VLP16}[a.shape], a.trace)
    if r is None:
        return
    cell = lambda k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}]"  # noqa: E731
    lines = [json.dumps(r), "",
             "| S | boxes | call | ms per call | byte floor, MB | floor at 6.29 TB/s, ms | call / floor | torch, scaled, ms | torch / call |",
             "|---|---|---|---|---|---|---|---|---|"]
    for kind, name in (("masks", "with masks"), ("plain", "without masks")):
        k = r[kind]
        lines.append(f"| {r['S']} | {r['S'] * r['boxes_per_seq']} | {name} | {cell(kind)} | {k['floor_bytes'] / 1e6:.1f} | {k['floor_ms']:.3f} | "
                     f"{k['over_floor']} | {k['torch_scaled_ms']:.0f} | {k['torch_over_call']:.0f} |")
    lines += ["", "| S | boxes | call (without masks) | ms per call |", "|---|---|---|---|",
              f"| {r['S']} | {r['S'] * r['boxes_per_seq']} | every sequence's largest boxes first | {cell('plain_largest_first')} |",
              f"| {r['S']} | {r['S'] * r['boxes_per_seq']} | every sequence's largest boxes last | {cell('plain_largest_last')} |",
              f"| {r['S']} | {r['S']} | one full-image box per sequence ({r['full_image_points']} points each) | {cell('full_image_alone')} |"]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
