"""What mld_region_depths_collect_device must write, restated in NumPy: the clipped box scanned in row-major order, the
counted points, count / minimum / maximum / exact median / nearest point, and the borders of
PointHistogram::FilterPointsMinDistBlob (HistogramPointDepth.cpp:30-100) with the binning of Histogram::AddElement
(Histogram.cpp:29-30).  Nothing here is compared with a tolerance: the records are integers and float bits."""
import math

import numpy as np

from mono_lidar_depth_amd import capi

DTYPE = np.dtype(capi.MldRegionDepth)
BAD_INPUT, EMPTY_BOX, HIST_FOUND, HIST_CAPPED, HAS_MASK = 1, 2, 4, 8, 16
LIST_CAPACITY, HIST_BINS = capi.MLD_REGION_LIST_CAPACITY, capi.MLD_REGION_HIST_BINS
INT_MAX = 2147483647


def bin_index(z, bin_width, bin_count):
    """Histogram.cpp:29-30: (int)min(|min(value, 1e10) / binWidth|, bins - 1) for every z."""
    z = np.asarray(z, dtype=np.float64)
    q = np.abs(np.minimum(z, 1e10) / np.float64(bin_width))
    return np.minimum(q, np.float64(bin_count) - 1.0).astype(np.int64)  # (>= 0: astype truncates like (int))


def bin_counts(z, bin_width, bin_count):
    """binElemCount of every bin after AddElement of every z."""
    return np.bincount(bin_index(z, bin_width, bin_count), minlength=bin_count).astype(np.int32)


def histogram_frame(z_max, bin_width):
    """HistogramPointDepth.cpp:36-43: `int maxDist` = ceil of the largest depth (it is > 0 here), binCount = (int)(maxDist /
    binWidth + 1).  A double beyond the int range saturates (the reference's conversion is undefined there)."""
    up = math.ceil(z_max) if math.isfinite(z_max) else math.inf
    max_dist = INT_MAX if up >= 2147483648.0 else int(up)
    bc = np.float64(max_dist) / np.float64(bin_width) + 1.0
    return INT_MAX if bc >= 2147483648.0 else int(bc)


def blob_borders(z, bin_width, min_count, hist_bins=HIST_BINS):
    """(flags, lower, higher) of the counted depths z (all > 0, at least one): HIST_FOUND with the borders of the first
    local-maximum bin, HIST_CAPPED when the scan would have to look beyond hist_bins bins from the bin of the smallest z,
    else 0; -1 / -1 without a bin.  The scan starts at the lowest bin with a point: the empty bins ahead of it never
    change binMaxId for good (a maximum of 0 points, possible with min_count <= 0, is overtaken by the first point)."""
    z = np.asarray(z, dtype=np.float64)
    bin_count = histogram_frame(float(z.max()), bin_width)
    if bin_count <= 1:  # :53
        return 0, -1.0, -1.0
    idx = bin_index(z, bin_width, bin_count)
    b0 = int(idx.min())
    rel = idx - b0
    counts = np.bincount(rel[rel < hist_bins], minlength=hist_bins)
    bin_max_id, bin_max_val, value = -1, -1, 0
    for i in range(b0, bin_count):  # :70-85
        if i - b0 >= hist_bins:
            return HIST_CAPPED, -1.0, -1.0
        last, value = value, int(counts[i - b0])
        if value > bin_max_val and value >= min_count:
            bin_max_val, bin_max_id = value, i
        elif value < bin_max_val:
            break
        if last > 0 and value == 0:
            return 0, -1.0, -1.0
    if bin_max_id < 0:  # :95
        return 0, -1.0, -1.0
    bw = np.float64(bin_width)
    lower = np.float64(bin_max_id) * bw - np.float64(np.float32(0.0)) * bw   # :99
    higher = np.float64(bin_max_id) * bw + np.float64(np.float32(1.0)) * bw  # :100
    return HIST_FOUND, float(lower), float(higher)


def clip_box(box, W, H):
    """The clipped box (x0, y0, x1, y1), or None for an EMPTY one: NeighborFinderPixel.cpp:70-79 for integer edges."""
    x0, y0, x1, y1 = (int(v) for v in box)
    cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if x1 < x0 or y1 < y0 or cx1 < cx0 or cy1 < cy0:
        return None
    return cx0, cy0, cx1, cy1


def order_statistics(z, orig):
    """(z_min, z_max, z_median, nearest_orig) of the counted points in scan order, through the bit patterns: positive
    doubles order as their bits.  The median is the element of rank (n - 1) // 2; the nearest point is the first of the
    smallest in scan order."""
    bits = np.ascontiguousarray(z, dtype=np.float64).view(np.uint64)
    srt = np.sort(bits)
    order = np.lexsort((np.arange(bits.size), bits))  # by z, then by scan position
    as_f = lambda b: float(np.array([b], dtype=np.uint64).view(np.float64)[0])  # noqa: E731
    return as_f(srt[0]), as_f(srt[-1]), as_f(srt[(bits.size - 1) // 2]), int(orig[order[0]])


def region_record(pixel_map, index, cam, n_points, box, bin_width, min_count, mask_bits=None, index_len=None,
                  hist_bins=HIST_BINS):
    """The record (DTYPE scalar) of one box.  pixel_map [H, W] int32, index int32, cam [n, 3] float64; mask_bits: bool per
    original point, or None (the sequence has no mask)."""
    pm = np.asarray(pixel_map)
    H, W = pm.shape
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    n_idx = index.size if index_len is None else int(index_len)
    cam = np.asarray(cam, dtype=np.float64).reshape(-1, 3)
    rec = np.zeros((), dtype=DTYPE)
    rec["flags"] = HAS_MASK if mask_bits is not None else 0
    rec["nearest_orig"] = -1
    rec["clip"] = -1
    for name in ("z_min", "z_max", "z_median", "hist_lower", "hist_higher"):
        rec[name] = -1.0
    clip = clip_box(box, W, H)
    if clip is None:
        rec["flags"] |= EMPTY_BOX
        return rec
    rec["clip"] = clip
    m = pm[clip[1]:clip[3] + 1, clip[0]:clip[2] + 1].reshape(-1).astype(np.int64)  # row-major scan order
    m = m[m != -1]
    ok = (m >= 0) & (m < n_idx)
    bad = bool((~ok).any())
    orig = index[m[ok]]
    ok = (orig >= 0) & (orig < n_points)
    bad |= bool((~ok).any())
    orig = orig[ok]
    z = cam[orig, 2]
    ok = z > 0.0  # (false for NaN)
    bad |= bool((~ok).any())
    orig, z = orig[ok], z[ok]
    if mask_bits is not None:
        ground = np.asarray(mask_bits, dtype=bool)[orig]
        rec["n_ground"] = int(ground.sum())
        orig, z = orig[~ground], z[~ground]
    if bad:
        rec["flags"] |= BAD_INPUT
    rec["n_points"] = z.size
    if z.size == 0:
        return rec
    rec["z_min"], rec["z_max"], rec["z_median"], rec["nearest_orig"] = order_statistics(z, orig)
    flag, lower, higher = blob_borders(z, bin_width, min_count, hist_bins)
    rec["flags"] |= flag
    rec["hist_lower"], rec["hist_higher"] = lower, higher
    if flag == HIST_FOUND:
        rec["n_seg"] = int(((z >= lower) & (z < higher)).sum())
    return rec


def region_records(pixel_map, index, cam, n_points, boxes, bin_width, min_count, mask_bits=None, index_len=None):
    """The records of the boxes ([n, 4]) of one sequence."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    out = np.zeros(boxes.shape[0], dtype=DTYPE)
    for i, b in enumerate(boxes):
        out[i] = region_record(pixel_map, index, cam, n_points, b, bin_width, min_count, mask_bits, index_len)
    return out


def same_records(got, want):
    """Equality of two record arrays, field by field: integers, and the raw bits of the doubles.  Returns the names of the
    fields that differ."""
    bad = []
    for name in DTYPE.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        same = a.view(np.int64) == b.view(np.int64) if a.dtype.kind == "f" else a == b
        if not np.all(same):
            bad.append(name)
    return bad


def window_box(x, y, half_x, half_y, W, H):
    """The box equal to the window of NeighborFinderPixel::getNeighbors at the integer pixel (x, y): the edges clamped in
    f64, truncated with (int) (NeighborFinderPixel.cpp:70-76)."""
    left, right = max(float(x) - half_x, 0.0), min(float(x) + half_x, float(W - 1))
    top, bottom = max(float(y) - half_y, 0.0), min(float(y) + half_y, float(H - 1))
    return int(left), int(top), int(right), int(bottom)
