"""The rule of mld_sweep_merge (include/mld.h) in NumPy: what the GPU tests compare against, bit for bit.

Per sweep: x, y, z at floats 0, 1, 2 of a record, the intensity where mld_pack_points_host takes it (float 3 of a 4-float
record, float 4 of an 8-float one) as raw bits; the 3x4 matrix in float64 with explicit parentheses,
    x' = float32(T[3] + (T[0] x + (T[1] y + T[2] z))),
a missing matrix leaving the bits as they are; NON-FINITE where one of x', y', z' is not finite; otherwise OUT OF RANGE
where r2 = x' x' + (y' y' + z' z') in float32 fails lo2 <= r2 <= hi2 with lo2, hi2 the float32 squares of the ranges.  The
kept records of sweep 0 in their order, then those of sweep 1, and so on.  TEST INFRASTRUCTURE."""
import numpy as np

from mono_lidar_depth_amd import capi

DTYPE = np.dtype(capi.MldSweepMergeRecord)
MAX_SWEEPS = capi.MLD_SWEEP_MAX_SWEEPS


def transform_sweep(cloud, T):
    """(xyz' float32 [n, 3], intensity bits uint32 [n]) of one sweep: float32 [n, 4] or [n, 8]; T: None or 12+ float64."""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    bits = cloud.view(np.uint32)[:, 3 if cloud.shape[1] == 4 else 4].copy()
    if T is None:
        return cloud[:, :3].copy(), bits
    T = np.asarray(T, dtype=np.float64).reshape(-1)[:12]
    x, y, z = (cloud[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        out = [(T[4 * r + 3] + ((T[4 * r] * x) + ((T[4 * r + 1] * y) + (T[4 * r + 2] * z)))).astype(np.float32) for r in range(3)]
    return np.stack(out, axis=1), bits


def verdicts(xyz, min_range, max_range):
    """0 kept, 1 non-finite, 2 out of range, per record."""
    lo2 = np.float32(min_range) * np.float32(min_range)
    hi2 = np.float32(max_range) * np.float32(max_range)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        r2 = (x * x) + ((y * y) + (z * z))  # (float32 throughout)
        inside = (lo2 <= r2) & (r2 <= hi2)
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    return np.where(~finite, 1, np.where(inside, 0, 2)).astype(np.int32)


def merge_sequence(sweeps, transforms=None, min_range=0.0, max_range=np.inf, capacity=None):
    """One sequence: sweeps a list of float32 [n, 4] / [n, 8] arrays (None: empty), transforms None or a list of None /
    matrices.  Returns a dict: merged (uint32 [n_written, 4], the records' bits), sweep (uint8), orig (int32), record (a
    DTYPE scalar)."""
    parts, sw, og = [], [], []
    rec = np.zeros((), dtype=DTYPE)
    for j, cloud in enumerate(sweeps):
        if cloud is None or len(cloud) == 0:
            continue
        xyz, bits = transform_sweep(cloud, transforms[j] if transforms is not None else None)
        v = verdicts(xyz, min_range, max_range)
        keep = np.flatnonzero(v == 0)
        rec["n_in"] += len(v)
        rec["n_nonfinite"] += int((v == 1).sum())
        rec["n_out_of_range"] += int((v == 2).sum())
        rec["kept"][j] = len(keep)
        parts.append(np.concatenate([xyz[keep].view(np.uint32), bits[keep, None]], axis=1))
        sw.append(np.full(len(keep), j, dtype=np.uint8))
        og.append(keep.astype(np.int32))
    merged = np.concatenate(parts) if parts else np.zeros((0, 4), np.uint32)
    sw = np.concatenate(sw) if sw else np.zeros(0, np.uint8)
    og = np.concatenate(og) if og else np.zeros(0, np.int32)
    n_kept = len(merged)
    cap = n_kept if capacity is None else int(capacity)
    rec["n_kept"] = n_kept
    rec["n_written"] = min(n_kept, cap)
    rec["flags"] = capi.MLD_SWEEP_FLAG_TRUNCATED if n_kept > cap else 0
    w = int(rec["n_written"])
    return {"merged": np.ascontiguousarray(merged[:w]), "sweep": sw[:w], "orig": og[:w], "record": rec}


def merged_cloud(result) -> np.ndarray:
    """The merged records of merge_sequence() as a float32 [n, 4] cloud."""
    return np.ascontiguousarray(result["merged"]).view(np.float32)


def merge_by_loop(sweeps, transforms=None, min_range=0.0, max_range=np.inf):
    """The same rule one record at a time in plain Python arithmetic on NumPy scalars: (list of 4-tuples of bits, list of
    sweeps, list of indices, counts (n_nonfinite, n_out_of_range))."""
    lo2 = np.float32(min_range) * np.float32(min_range)
    hi2 = np.float32(max_range) * np.float32(max_range)
    out, sw, og, n_nf, n_or = [], [], [], 0, 0
    with np.errstate(all="ignore"):
        for j, cloud in enumerate(sweeps):
            if cloud is None:
                continue
            T = None if transforms is None or transforms[j] is None else [np.float64(t) for t in np.asarray(transforms[j]).reshape(-1)[:12]]
            for i, row in enumerate(np.asarray(cloud, dtype=np.float32)):
                p = [np.float32(row[0]), np.float32(row[1]), np.float32(row[2])]
                if T is not None:
                    x, y, z = np.float64(p[0]), np.float64(p[1]), np.float64(p[2])
                    p = [np.float32(T[4 * r + 3] + (T[4 * r] * x + (T[4 * r + 1] * y + T[4 * r + 2] * z))) for r in range(3)]
                if not all(np.isfinite(c) for c in p):
                    n_nf += 1
                    continue
                r2 = np.float32(p[0] * p[0]) + np.float32(np.float32(p[1] * p[1]) + np.float32(p[2] * p[2]))
                if not (lo2 <= r2 <= hi2):
                    n_or += 1
                    continue
                w = np.float32(row[3 if len(row) == 4 else 4])
                out.append(tuple(int(np.float32(c).view(np.uint32)) for c in (*p, w)))
                sw.append(j)
                og.append(i)
    return out, sw, og, (n_nf, n_or)
