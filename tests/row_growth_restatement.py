"""What mld_row_growth_segment_device and mld_row_growth_collect_*_device must write, restated on the CPU loop for loop from
the reference (HelperLidarRowSegmentation.cpp, DepthEstimator.cpp:509-558, :687-724), with plain Python floats and math.sqrt:
  segment_rows      SegmentPoints: the starts of the rows of a visible list
  window_list       the narrow window's neighbours in scan order (NeighborFinderPixel.cpp:60-95), as gather_window reads them
  seed_fold         CalculateNearestPoint's fold with its float accumulator (through np.float32)
  neighbor_points   calculateNeighborPoints: the second seed, getMaxDist, getSelectionFromSeed twice
  tail              CalculateDepthSegmented on the grown list: nearest_depth_restatement.main_path (the oracle's parts) with
                    the count test and the histogram switched off
  records           all of it, as the 72-byte record
ONE copy of every rule.  `repaired`: names of quirks to replace by what their author presumably meant - only for the tests
that show that the literal rule and the repaired one differ; the records are the literal rules (repaired empty).
Nothing here is compared with a tolerance: the records are integers and float bits."""
import math

import numpy as np

from mono_lidar_depth_amd import capi

import nearest_depth_restatement as N

DTYPE = np.dtype(capi.MldRowGrowth)
CLOUD_DTYPE = np.dtype(capi.MldRowGrowthCloud)
BAD_INPUT, NONFINITE = capi.MLD_ROW_GROWTH_FLAG_BAD_INPUT, capi.MLD_ROW_GROWTH_FLAG_NONFINITE_FEATURE
ROWS_TRUNCATED, LIST_CAPPED = capi.MLD_ROW_GROWTH_FLAG_ROWS_TRUNCATED, capi.MLD_ROW_GROWTH_FLAG_LIST_CAPPED
MAX_LIST = capi.MLD_ROW_GROWTH_MAX_LIST
INT_MIN = float(-2 ** 31)
QUIRKS = ("float_fold", "strict_50", "tie_bottom", "pc_pc1", "swapped_roles", "last_kept", "merge_either", "half_count",
          "max_dist_start")
LITERAL = frozenset()


def growth(thr, s2s, s2s_grad, n2s, n2s_grad, nb, nb_grad, count):
    """A parameter set in the order calculateNeighborPoints takes its arguments (test_monolidar_fusion.cpp:236-243)."""
    return capi.MldRowGrowthParams(depth_segmentation_max_treshold_gradient=thr,
                                   depth_segmentation_max_seedpoint_to_seedpoint_distance=s2s,
                                   depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient=s2s_grad,
                                   depth_segmentation_max_neighbor_to_seedpoint_distance=n2s,
                                   depth_segmentation_max_neighbor_to_seedpoint_distance_gradient=n2s_grad,
                                   depth_segmentation_max_neighbor_distance=nb,
                                   depth_segmentation_max_neighbor_distance_gradient=nb_grad,
                                   depth_segmentation_max_pointcount=count)


# ---- SegmentPoints (HelperLidarRowSegmentation.cpp:18-46) ----------------------------------------------------------------

def segment_rows(xs, repaired=LITERAL):
    """The visible indices at which a row starts; point 0 always opens row 0."""
    starts, last = [], INT_MIN
    for i, x in enumerate(xs):
        x = float(x)
        opens = x >= last + 50 if "strict_50" in repaired else x > last + 50
        if opens or i == 0:
            starts.append(i)
        last = x
    return starts


def cloud_record(xs, row_capacity, guard=-7):
    """(the 16-byte record, row_start [row_capacity + 1] with `guard` where nothing is written) of a visible list."""
    starts = segment_rows(xs)
    n, n_rows = len(xs), len(starts)
    ends = starts[1:] + [n]
    rec = np.zeros(1, dtype=CLOUD_DTYPE)[0]
    rec["n_rows"], rec["n_vis"] = n_rows, n
    rec["longest_row"] = max((e - s for s, e in zip(starts, ends)), default=0)
    rec["flags"] = ROWS_TRUNCATED if n_rows > row_capacity else 0
    row_start = np.full(row_capacity + 1, guard, dtype=np.int32)
    k = min(n_rows, row_capacity + 1)
    row_start[:k] = starts[:k]
    if n_rows <= row_capacity:
        row_start[n_rows] = n
    return rec, row_start


# ---- the arrays of one sequence, as the collect calls read them --------------------------------------------------------

class Sequence:
    """pm [H, W] int32; index (index_len entries count); cam [n_points, 3]; vis_uv [>= index_len, 2]; row_start
    [row_capacity + 1]; n_rows, n_vis: the segment call's record."""

    def __init__(self, pm, index, index_len, cam, vis_uv, row_start, n_rows, n_vis, row_capacity):
        self.pm, self.index, self.index_len = np.asarray(pm), np.asarray(index), int(index_len)
        self.cam = np.asarray(cam, dtype=np.float64).reshape(-1, 3)
        self.n_points = self.cam.shape[0]
        self.vis_uv = np.asarray(vis_uv, dtype=np.float64).reshape(-1, 2)
        self.row_start = np.asarray(row_start)
        self.n_rows, self.n_vis, self.row_capacity = int(n_rows), int(n_vis), int(row_capacity)
        self.lim = min(max(self.n_vis, 0), self.index_len)
        self.bad = False

    def point3(self, p):
        """get3DPointFromCut, or None where the index lies outside the cloud."""
        o = int(self.index[p])
        if o < 0 or o >= self.n_points:
            return None
        return tuple(float(c) for c in self.cam[o])

    def point2(self, p):
        return float(self.vis_uv[p, 0]), float(self.vis_uv[p, 1])

    def row_range(self, r):
        s, e = int(self.row_start[r]), int(self.row_start[r + 1])
        if s < 0 or e > self.lim or s > e:
            self.bad = True
            return 0, 0
        return s, e


def from_visible(pm, index, cam, vis_uv, row_capacity=64):
    """A sequence whose rows are the segmentation of its own visible list."""
    vis_uv = np.asarray(vis_uv, dtype=np.float64).reshape(-1, 2)
    rec, row_start = cloud_record(vis_uv[:, 0], row_capacity)
    return Sequence(pm, index, len(index), cam, vis_uv, row_start, rec["n_rows"], rec["n_vis"], row_capacity)


def window_list(seq, P, u, v):
    """The visible indices of the narrow window's neighbours in row-major scan order (NeighborFinderPixel.cpp:60-95: half
    sizes and clamping in f64, (int) truncation).  A cell whose map value or index lies outside the arrays is empty and
    sets seq.bad."""
    H, W = seq.pm.shape
    hx = float(P.pixelarea_search_witdh) * 0.5 * 1.0
    hy = float(P.pixelarea_search_height) * 0.5 * 1.0
    x0, x1 = int(max(u - hx, 0.0)), int(min(u + hx, float(W - 1)))
    y0, y1 = int(max(v - hy, 0.0)), int(min(v + hy, float(H - 1)))
    out = []
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            m = int(seq.pm[y, x])
            if m == -1:
                continue
            if m < 0 or m >= seq.index_len or not 0 <= int(seq.index[m]) < seq.n_points:
                seq.bad = True
                continue
            out.append(m)
    return out


# ---- CalculateNearestPoint (DepthEstimator.cpp:687-724) ------------------------------------------------------------------

def seed_fold(zs, repaired=LITERAL):
    """The position of the nearest point, or -1: `float m = +inf; if (z_i < m) { m = z_i; idx = i; }`."""
    idx = -1
    if "float_fold" in repaired:
        m = math.inf
        for i, z in enumerate(zs):
            if float(z) < m:
                m, idx = float(z), i
        return idx
    m = np.float32(np.inf)
    with np.errstate(over="ignore"):
        for i, z in enumerate(zs):
            if float(z) < float(m):
                m, idx = np.float32(z), i
    return idx


# ---- calculateNeighborPoints (HelperLidarRowSegmentation.cpp:68-375) ------------------------------------------------------

def dist3(a, b):
    """PointcloudData::CalcDistance: pow(d, 2) is d * d, summed left to right."""
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def sqdist2(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return dx * dx + dy * dy


def get_max_dist(thr, start, grad, z_seed, repaired=LITERAL):
    if z_seed <= thr:
        return start
    delta = z_seed - (thr if "max_dist_start" in repaired else start)
    return start + delta * grad


def single_neighbor_row_point(seq, row, f, repaired=LITERAL):
    """getSingleNeighborRowPoint on the row [s, e): a visible index or -1."""
    s, e = row
    last, cur = (INT_MIN, 0.0), (0.0, 0.0)
    i_cur = i_last = -1
    found = False
    for p in range(s, e):
        i_cur, cur = p, seq.point2(p)
        if cur[0] < f[0] and last[0] >= f[0]:
            found = True
            break
        i_last, last = i_cur, cur
    if not found:
        return -1
    if i_last == -1:
        return i_cur
    d_cur = sqdist2(cur, f)
    d_last = sqdist2(last, f) if "pc_pc1" in repaired else sqdist2(cur, last)
    return i_cur if d_cur < d_last else i_last


def selection_from_seed(seq, row, p0, max_distance_neighbor, max_distance_seed, out, count, repaired=LITERAL):
    """getSelectionFromSeed: grows the row [s, e) from the seed at p0 onto `out`."""
    s, e = row
    seed = seq.point3(p0)
    last = seed
    if count < 0:
        for step in (1, -1):
            p = p0
            if step == -1 and "last_kept" in repaired:
                last = seed
            while True:
                p += step
                if p >= e or p < s:
                    break
                pt = seq.point3(p)
                if pt is None:
                    seq.bad = True
                    break
                if dist3(pt, seed) > max_distance_seed:
                    break
                if dist3(pt, last) > max_distance_neighbor:
                    break
                last = pt
                out.append(p)
        return
    pos, neg = p0 + 1, p0 - 1
    while True:
        if "half_count" in repaired and len(out) >= count:
            break
        up_out, down_out = pos >= e, neg < s
        if "merge_either" in repaired:
            if up_out and down_out:
                break
        elif up_out or down_out:
            break
        pt_pos = None if up_out else seq.point3(pos)
        pt_neg = None if down_out else seq.point3(neg)
        if (pt_pos is None and not up_out) or (pt_neg is None and not down_out):
            seq.bad = True
            break
        d_pos = math.inf if up_out else dist3(pt_pos, seed)
        d_neg = math.inf if down_out else dist3(pt_neg, seed)
        if d_pos <= d_neg and not up_out:
            p, d = pos, d_pos
            pos += 1
        else:
            p, d = neg, d_neg
            neg -= 1
        if d > max_distance_seed:
            break
        out.append(p)
        if len(out) >= count:
            break


def neighbor_points(seq, G, f, seed_vis, repaired=LITERAL):
    """calculateNeighborPoints behind getNearestPoint for the feature f = (u, v) and the seed: a dict with state, seed_row,
    second_vis, second_row, n_first and the grown list (visible indices, complete).  state 0 with seq.bad: the rows do not
    hold the seed."""
    out = dict(state=0, seed_row=-1, second_vis=-1, second_row=-1, n_first=0, grown=[])
    if seq.n_rows < 1 or seed_vis >= seq.lim:
        seq.bad = True
        return out
    lo, hi = 0, seq.n_rows  # getRowFromPoint: the largest r with row_start[r] <= seed_vis
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if int(seq.row_start[mid]) <= seed_vis:
            lo = mid
        else:
            hi = mid
    r = out["seed_row"] = lo
    row1 = seq.row_range(r)
    if not row1[0] <= seed_vis < row1[1]:
        seq.bad = True
        return out
    seed = seq.point3(seed_vis)
    # getNeighborRowPoint
    top = seq.row_range(r - 1) if r >= 1 else (0, 0)
    bottom = seq.row_range(r + 1) if r + 1 < seq.n_rows else (0, 0)
    i_top = single_neighbor_row_point(seq, top, f, repaired)
    i_bottom = single_neighbor_row_point(seq, bottom, f, repaired)
    if i_top < 0 and i_bottom < 0:
        out["state"] = -1
        return out
    if i_bottom < 0:
        cands = (i_top, -1)
    elif i_top < 0:
        cands = (i_bottom, -1)
    else:
        d_top, d_bottom = sqdist2(seq.point2(i_top), f), sqdist2(seq.point2(i_bottom), f)
        top_first = d_top <= d_bottom if "tie_bottom" in repaired else d_top < d_bottom
        cands = (i_top, i_bottom) if top_first else (i_bottom, i_top)
    z = seed[2]
    thr = G.depth_segmentation_max_treshold_gradient
    max_s2s = get_max_dist(thr, G.depth_segmentation_max_seedpoint_to_seedpoint_distance,
                           G.depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient, z, repaired)
    second = -1
    for cand in cands:  # selectRowIndex
        if cand < 0 or second >= 0:
            continue
        pt = seq.point3(cand)
        if pt is None:
            seq.bad = True
        elif dist3(seed, pt) <= max_s2s:
            second = cand
    if second < 0:
        out["state"] = -2
        return out
    out["second_vis"] = second
    out["second_row"] = r - 1 if second == i_top else r + 1
    row2 = top if second == i_top else bottom
    max_n2s = get_max_dist(thr, G.depth_segmentation_max_neighbor_to_seedpoint_distance,
                           G.depth_segmentation_max_neighbor_to_seedpoint_distance_gradient, z, repaired)
    max_nb = get_max_dist(thr, G.depth_segmentation_max_neighbor_distance, G.depth_segmentation_max_neighbor_distance_gradient,
                          z, repaired)
    # the call sites pass (maxDistNeighborToSeed, maxDistNeighbor) into (maxDistanceNeighbor, maxDistanceSeed)
    a, b = (max_nb, max_n2s) if "swapped_roles" in repaired else (max_n2s, max_nb)
    count = int(G.depth_segmentation_max_pointcount)
    if count == -1:
        first_count = -1
    elif "half_count" in repaired:
        first_count = (count + 1) // 2
    else:
        first_count = int(count / 2)  # C++ int division
    grown = out["grown"]
    selection_from_seed(seq, row1, seed_vis, a, b, grown, first_count, repaired)
    out["n_first"] = len(grown)
    selection_from_seed(seq, row2, second, a, b, grown, count, repaired)
    out["state"] = -3 if len(grown) == out["n_first"] else 1
    return out


# ---- the tail and the record ----------------------------------------------------------------------------------------------

def tail(frame, P, u, v, points):
    """CalculateDepthSegmented on `points` ([n, 3] in list order): nearest_depth_restatement.main_path without the count
    test and the histogram.  (type, depth, corners: positions in the list or None)."""
    mp = N.main_path(frame, P.replace(do_use_histogram_segmentation=0, radiusSearch_count_min=0), u, v, points)
    return mp["type"], mp["depth"], mp["corners"]


def records(frame, P, G, seq, uv, tracks=False):
    """(records [F] of DTYPE, lists: per feature the int32 visible indices of its grown list, complete) for the features uv
    [F, 2] on `seq`; frame: an OracleDepthEstimator with the calibration (its cloud is not looked at).  tracks: the
    coordinates go through float32 and truncf first."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    if tracks:
        uv = np.trunc(uv.astype(np.float32)).astype(np.float64)
    rec = np.zeros(uv.shape[0], dtype=DTYPE)
    lists = []
    for i, (u, v) in enumerate(uv):
        u, v = float(u), float(v)
        r = rec[i]
        r["seed_vis"] = r["second_vis"] = r["seed_row"] = r["second_row"] = -1
        r["corner_vis"] = -1
        r["depth"], r["seed_z"] = -1.0, np.nan
        lists.append(np.empty(0, np.int32))
        if seq.n_rows > seq.row_capacity:
            r["flags"] = ROWS_TRUNCATED
            continue
        if not (math.isfinite(u) and math.isfinite(v)):
            r["flags"], r["type"] = NONFINITE, 2
            continue
        seq.bad = False
        nb = window_list(seq, P, u, v)
        r["n_nb"] = len(nb)
        flags = 0
        if len(nb) < (int(P.radiusSearch_count_min) & 0xFFFFFFFF):
            r["type"] = 2
        else:
            zs = [seq.point3(m)[2] for m in nb]
            at = seed_fold(zs)
            if at < 0:
                r["type"] = 3
            else:
                r["seed_vis"], r["seed_z"] = nb[at], zs[at]
                if zs[at] > float(P.treshold_depth_max):
                    r["type"] = 4
                else:
                    g = neighbor_points(seq, G, (u, v), nb[at])
                    grown = g["grown"]
                    lists[-1] = np.asarray(grown, dtype=np.int32)
                    r["state"], r["seed_row"] = g["state"], g["seed_row"]
                    r["second_vis"], r["second_row"] = g["second_vis"], g["second_row"]
                    r["n_first"], r["n_grown"] = g["n_first"], len(grown)
                    if len(grown) > MAX_LIST:
                        flags |= LIST_CAPPED
                    elif g["state"] == 1:
                        pts = np.array([seq.point3(p) for p in grown], dtype=np.float64)
                        t, depth, corners = tail(frame, P, u, v, pts)
                        r["grown_type"] = t
                        if corners is not None:
                            r["corner_vis"] = [grown[c] for c in corners]
                        if t == 1:
                            r["type"], r["depth"] = 20, depth
        if seq.bad:
            flags |= BAD_INPUT
        r["flags"] = flags
    return rec, lists


def decides(rec):
    """Where the stage's result stands in for the product's (type 20, the early 4, the early 3)."""
    return np.isin(rec["type"], (20, 4, 3))


def same_records(got, want):
    """The names of the fields in which two record arrays differ: integers, and the raw bits of the doubles (the sign of a
    zero included); a NaN equals a NaN whatever its payload."""
    bad = []
    for name in DTYPE.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.dtype.kind == "f":
            same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
        else:
            same = a == b
        if not same.all():
            bad.append(name)
    return bad
