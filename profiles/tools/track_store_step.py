#!/usr/bin/env python3
"""What the GPU-resident tracklet store costs per step on BASELINE config 5's shapes (128 x 4096 clouds, 10 000 tracks
per sequence, 30 % new per frame), for S = 16, 64, 256 sequences per launch set:

  (a) TrackletBatch.run   the new-track masks already on the device: projection + mld_tracklets_depths_device
  (b) TrackletBatch.step  ids in: projection + mld_tracklets_step_device (look-up -> depths -> release + commit)
  (c) for scale only: the host side that (a) leaves to its caller for ONE frame of all sequences - numpy.isin of every
      sequence's ids against its previous frame's, and the upload of the masks
  (d) mld_tracks_export_device of every sequence's histories (S x 10 000 x max_history x 12 bytes written)

Wall time over `--steps` steps queued back to back, one synchronisation at the end, after a warm-up of the same length.
Prints one JSON line per S and a markdown table; run it on the GPU box."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from mono_lidar_depth_amd import CameraPinhole, TrackletBatch, capi, synth  # noqa: E402


def mask_words(inl, n):
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return m.view(np.int32)


def measure(S, steps, history, n_tracks=10000, new_frac=0.3):
    import torch
    dev = torch.device("cuda", 0)
    P = capi.params_c0()
    cam = CameraPinhole(synth.KITTI_W, synth.KITTI_H, synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV)
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
        u0 = rng.integers(0, cam.width, n_tracks).astype(np.float32)
        v0 = rng.integers(100, cam.height, n_tracks).astype(np.float32)
        u1 = (u0 + rng.integers(-3, 4, n_tracks)).astype(np.float32)
        v1 = (v0 + rng.integers(-2, 3, n_tracks)).astype(np.float32)
        new = np.zeros(n_tracks, dtype=np.uint8)
        new[rng.choice(n_tracks, n_new, replace=False)] = 1
        sets_d.append(tuple(torch.from_numpy(a).to(dev) for a in (u0, v0, u1, v1, new)))
    # ids: every frame replaces 30 % of every sequence's tracks by fresh ids (own id space per sequence)
    total = 2 * steps + 2
    ids_h, cur, next_id = [], np.tile(np.arange(n_tracks, dtype=np.int64), (S, 1)), n_tracks
    for t in range(total):
        if t:
            for q in range(S):
                cur[q, rng.choice(n_tracks, n_new, replace=False)] = np.arange(next_id, next_id + n_new)
            next_id += n_new
        ids_h.append((cur + 7919 * np.arange(S)[:, None]).astype(np.int32))
    ids_d = [torch.from_numpy(i).to(dev) for i in ids_h]
    outs = [torch.empty((S, n_tracks), dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32, torch.int32)]
    rows = lambda t: [t[q] for q in range(S)]  # noqa: E731
    coeffs = [np.stack([planes_h[(b + 2 * q) % U][0] for q in range(S)]) for b in range(2)]
    pick = lambda b, j: [sets_d[(b + q) % K][j] for q in range(S)]  # noqa: E731

    def timed(fn, first):
        for it in range(first, first + steps):
            fn(it)
        tb.est.synchronize()
        t0 = time.perf_counter()
        for it in range(first + steps, first + 2 * steps):
            fn(it)
        tb.est.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    # (a) the masks on the device
    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, n_tracks, list_capacity=(48, 24))
    prep_a = [tb.prepare(rows(all_clouds[b]), coeffs[b], rows(all_masks[b]), pick(b, 0), pick(b, 1), pick(b, 2), pick(b, 3),
                         pick(b, 4), *[rows(o) for o in outs]) for b in range(2)]
    torch.cuda.synchronize()
    tb.run(prep_a[0])  # (both banks hold a cloud before either path is timed)
    ms_a = timed(lambda it: tb.run(prep_a[(it + 1) % 2]), 0)
    tb.close()

    # (b) the store decides
    tb = TrackletBatch(P, cam, synth.T_CAM_LIDAR, S, n_tracks, list_capacity=(48, 24))
    store = tb.attach_store(history)
    prep_b = [tb.prepare_step(rows(all_clouds[t % 2]), coeffs[t % 2], rows(all_masks[t % 2]), rows(ids_d[t]), pick(t % 2, 0),
                              pick(t % 2, 1), pick(t % 2, 2), pick(t % 2, 3), *[rows(o) for o in outs]) for t in range(total)]
    torch.cuda.synchronize()
    tb.step(prep_b[0])  # (the first frame: every track is new)
    ms_b = timed(lambda it: tb.step(prep_b[it + 1]), 0)
    counts = store.counts()
    # (d) export
    fp = torch.empty((S, n_tracks, history, 3), dtype=torch.float32, device=dev)
    ln = torch.empty((S, n_tracks), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    store.export(rows(fp), rows(ln))
    tb.est.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        store.export(rows(fp), rows(ln))
    tb.est.synchronize()
    ms_d = (time.perf_counter() - t0) / steps * 1e3
    assert int(ln.min()) == 2 and int(ln.max()) <= min(history, total)
    assert (counts[:, 0] == n_tracks).all() and (counts[:, 1] == n_new).all() and (counts[:, 5] == 0).all()
    tb.close()

    # (c) the host's share of (a), one frame: membership of every sequence's ids in its previous frame's + mask upload
    reps = []
    for t in range(1, min(total, 4)):
        t0 = time.perf_counter()
        mask = np.stack([~np.isin(ids_h[t][q], ids_h[t - 1][q]) for q in range(S)]).astype(np.uint8)
        t1 = time.perf_counter()
        torch.from_numpy(mask).to(dev)
        torch.cuda.synchronize()
        reps.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        assert int(mask.sum()) == S * n_new
    ms_c_isin, ms_c_up = (float(np.median([r[k] for r in reps])) for k in range(2))
    assoc = S * (n_tracks + n_new)
    return {"S": S, "steps": steps, "max_history": history, "n_tracks": n_tracks, "new_frac": new_frac,
            "a_run_ms": round(ms_a, 4), "b_step_ms": round(ms_b, 4), "b_minus_a_ms": round(ms_b - ms_a, 4),
            "b_over_a": round(ms_b / ms_a, 4), "c_host_isin_ms": round(ms_c_isin, 3), "c_mask_upload_ms": round(ms_c_up, 3),
            "d_export_ms": round(ms_d, 4), "a_G_assoc_per_s": round(assoc / ms_a / 1e6, 3),
            "b_G_assoc_per_s": round(assoc / ms_b / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", default="16,64,256")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--history", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines and the table to this file")
    a = ap.parse_args()
    res = [measure(int(s), a.steps, a.history) for s in a.seqs.split(",")]
    lines = [json.dumps(r) for r in res]
    lines += ["", "| S | (a) run, ms/step | (b) step, ms/step | (b) - (a) | (b) / (a) | (c) host isin + mask upload, ms/frame | (d) export, ms |",
              "|---|---|---|---|---|---|---|"]
    lines += [f"| {r['S']} | {r['a_run_ms']:.3f} | {r['b_step_ms']:.3f} | {r['b_minus_a_ms']:+.3f} | {r['b_over_a']:.3f} | "
              f"{r['c_host_isin_ms']:.1f} + {r['c_mask_upload_ms']:.2f} | {r['d_export_ms']:.3f} |" for r in res]
    print("\n".join(lines), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
