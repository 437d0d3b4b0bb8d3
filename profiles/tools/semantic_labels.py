#!/usr/bin/env python3
"""What mld_labels_assign_device costs beside the tracklet step on BASELINE config 5's shapes: S sequences x 10 000 tracks,
one 375 x 1242 label image per sequence (synth.KITTI_H x synth.KITTI_W), roi 5 x 5 (the default: 4 x 4 pixels per track,
the row kernel) and 50 x 50 (the .rosif maximum: up to 2500 pixels per track, the wavefront kernel).

In ONE process, on the same context and stream:
  step     TrackletBatch.step (projection + mld_tracklets_step_device; 128 x 4096 clouds, 30 % new tracks per frame)
  labels   mld_labels_assign_device alone, with and without votes_out
each timed with a pair of events on the context's stream around `--reps` calls queued back to back, after a warm-up of
the same calls; the median of `--rounds` such windows is reported, with the spread.  The label call is then stated as a
share of the step.  Prints one JSON line per S and a markdown table; run it on the GPU box."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, TrackletBatch, capi, synth  # noqa: E402


def mask_words(inl, n):
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return m.view(np.int32)


def label_image(rng, rows, cols, n_values=19):
    """A segmentation-like image: patches of 24 x 32 pixels of one of 19 classes, 2 % single-pixel noise."""
    coarse = rng.integers(0, n_values, ((rows + 23) // 24, (cols + 31) // 32))
    img = np.repeat(np.repeat(coarse, 24, axis=0), 32, axis=1)[:rows, :cols]
    noise = rng.random((rows, cols)) < 0.02
    return np.where(noise, rng.integers(0, n_values, (rows, cols)), img).astype(np.uint8)


def measure(S, reps, rounds, n_tracks=10000, new_frac=0.3, history=16):
    import torch
    dev = torch.device("cuda", 0)
    P = capi.params_c0()
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
    rows_img, cols_img = synth.KITTI_H, synth.KITTI_W
    U, K = 4, 8
    clouds_h = [synth.make_cloud(synth.DENSE128, seed=5, frame=f) for f in range(U)]
    planes_h = [synth.make_ground_plane(c) for c in clouds_h]
    N = clouds_h[0].shape[0]
    all_clouds = torch.empty((2, S, N, 4), dtype=torch.float32, device=dev)  # two banks of S slots, distinct HBM per slot
    all_masks = torch.empty((2, S, (N + 31) // 32), dtype=torch.int32, device=dev)
    d_unique = [torch.from_numpy(c).to(dev) for c in clouds_h]
    m_unique = [torch.from_numpy(mask_words(p[1], N)).to(dev) for p in planes_h]
    for b in range(2):
        for q in range(S):
            all_clouds[b, q].copy_(d_unique[(b + 2 * q) % U])
            all_masks[b, q].copy_(m_unique[(b + 2 * q) % U])
    del d_unique, m_unique
    rng = np.random.default_rng(5)
    n_new = int(n_tracks * new_frac)
    sets_d = []
    for k in range(K):
        u0 = rng.uniform(0, cam.width, n_tracks).astype(np.float32)
        v0 = rng.uniform(100, cam.height, n_tracks).astype(np.float32)
        u1 = (u0 + rng.integers(-3, 4, n_tracks)).astype(np.float32)
        v1 = (v0 + rng.integers(-2, 3, n_tracks)).astype(np.float32)
        sets_d.append(tuple(torch.from_numpy(a).to(dev) for a in (u0, v0, u1, v1)))
    # a distinct image per sequence (distinct HBM), eight different contents
    images = torch.empty((S, rows_img, cols_img), dtype=torch.uint8, device=dev)
    img_unique = [torch.from_numpy(label_image(rng, rows_img, cols_img)).to(dev) for _ in range(K)]
    for q in range(S):
        images[q].copy_(img_unique[q % K])
    del img_unique
    # ids: every frame replaces 30 % of every sequence's tracks by fresh ids
    n_tables = reps * (rounds + 1) + 1  # one per step that is run
    ids_h, cur, next_id = [], np.tile(np.arange(n_tracks, dtype=np.int64), (S, 1)), n_tracks
    for t in range(n_tables):
        for q in range(S if t else 0):
            cur[q, rng.choice(n_tracks, n_new, replace=False)] = np.arange(next_id, next_id + n_new)
        next_id += n_new
        ids_h.append((cur + 7919 * np.arange(S)[:, None]).astype(np.int32))
    ids_d = [torch.from_numpy(i).to(dev) for i in ids_h]
    outs = [torch.empty((S, n_tracks), dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32, torch.int32)]
    label_out = torch.empty((S, n_tracks), dtype=torch.int16, device=dev)
    votes_out = torch.empty((S, n_tracks, 2), dtype=torch.int32, device=dev)
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    coeffs = [np.stack([planes_h[(b + 2 * q) % U][0] for q in range(S)]) for b in range(2)]
    pick = lambda b, j: [sets_d[(b + q) % K][j] for q in range(S)]  # noqa: E731

    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, n_tracks, list_capacity=(48, 24))
    tb.attach_store(history)
    tb.attach_labels()
    prep = [tb.prepare_step(rows(all_clouds[t % 2]), coeffs[t % 2], rows(all_masks[t % 2]), rows(ids_d[t]), pick(t % 2, 0),
                            pick(t % 2, 1), pick(t % 2, 2), pick(t % 2, 3), *[rows(o) for o in outs]) for t in range(n_tables)]
    stream = torch.cuda.ExternalStream(tb.est.stream, device=dev)
    torch.cuda.synchronize()
    frame = [0]

    def step():
        tb.step(prep[frame[0]])
        frame[0] += 1

    def window(fn, n):
        """ms per call of n calls between two events on the context's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        tb.est.synchronize()
        return e0.elapsed_time(e1) / n

    def timed(fn, n):
        window(fn, n)  # warm-up: the same calls, the same shapes
        w = sorted(window(fn, n) for _ in range(rounds))
        return {"median_ms": round(w[len(w) // 2], 4), "min_ms": round(w[0], 4), "max_ms": round(w[-1], 4)}

    label_tabs = (rows(images), rows(label_out), rows(votes_out))
    res = {"S": S, "n_tracks": n_tracks, "image": [rows_img, cols_img], "reps": reps, "rounds": rounds}
    step()  # (the first frame: every track is new)
    res["step"] = timed(step, reps)
    f = prep[frame[0] - 1]
    for name, roi, votes in (("labels_5x5", (5, 5), None), ("labels_5x5_votes", (5, 5), label_tabs[2]),
                             ("labels_50x50", (50, 50), None), ("labels_50x50_votes", (50, 50), label_tabs[2])):
        n = reps if roi[0] < 16 else max(1, reps // 4)
        res[name] = timed(lambda: tb.labels(f, label_tabs[0], roi, label_tabs[1], votes), n)
        res[name]["share_of_step"] = round(res[name]["median_ms"] / res["step"]["median_ms"], 5)
    # what the 5 x 5 call has to move at the least: u, v, 16 label bytes in four 4-byte pieces and the int16 result
    res["labels_5x5_min_bytes"] = S * n_tracks * (8 + 16 + 2)
    labelled = int((label_out >= 0).sum())
    assert labelled > 0.9 * S * n_tracks, labelled
    tb.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", default="256")
    ap.add_argument("--reps", type=int, default=8, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per figure")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the table to this file")
    a = ap.parse_args()
    res = [measure(int(s), a.reps, a.rounds) for s in a.seqs.split(",")]
    lines = [json.dumps(r) for r in res]
    lines += ["", "| S | step, ms | labels 5 x 5, ms (share of step) | with votes | labels 50 x 50, ms (share) | with votes |",
              "|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f}] ({100 * r[k]['share_of_step']:.2f} %)"  # noqa: E731
    lines += [f"| {r['S']} | {r['step']['median_ms']:.3f} [{r['step']['min_ms']:.3f} .. {r['step']['max_ms']:.3f}] | "
              f"{cell(r, 'labels_5x5')} | {cell(r, 'labels_5x5_votes')} | {cell(r, 'labels_50x50')} | {cell(r, 'labels_50x50_votes')} |"
              for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
