"""What mld_feature_traces_collect_*_device must write, built from the existing oracle alone:
  OracleDepthEstimator.trace_feature on a frame WITH the plane   the lists, the corner positions, the plane
  a second oracle frame WITHOUT a plane, calculate_depth          main_type and main_depth of every feature
  oracle.filter_points_min_dist_blob                               the borders of the chosen bin
  calibration(), cloud_camera_cs(), point_index()                  the f32 distance test restated in NumPy, which tells
                                                                   FAR_NEIGHBOUR from FEW_INLIERS
Nothing here is compared with a tolerance: the records are integers and float bits."""
import numpy as np

from mono_lidar_depth_amd import capi
from oracle import oracle

from helpers import make_oracle

DTYPE = np.dtype(capi.MldFeatureTrace)
NOT_REACHED, FEW_NEIGHBOURS, FAR_NEIGHBOUR, FEW_INLIERS, FIT = 0, 1, 2, 3, 4
BAD_INPUT, NONFINITE = 1, 2
LISTS = ("nb", "seg", "road", "road_inl")


def far_mask(Tinv, coeffs, pts, thr):
    """DepthEstimator.cpp:810-815 for the rows of pts ([k, 3] camera frame): the f64 camera->lidar transform with the
    fixed-size product order, the cast to float, the un-normalised float distance, distance > thr."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    lid = [(Tinv[r, 3] + (Tinv[r, 0] * x + (Tinv[r, 1] * y + Tinv[r, 2] * z))).astype(np.float32) for r in range(3)]
    c = np.asarray(coeffs, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = np.abs(((c[0] * lid[0] + c[1] * lid[1]) + c[2] * lid[2]) + c[3])
    assert d.dtype == np.float32
    return d.astype(np.float64) > thr


class Restatement:
    """The frame of one sequence: cloud [n, 4 or 8] float32, plane = (coeffs, inlier indices) or None."""

    def __init__(self, params, cloud, plane=None, camera=None, T=None):
        self.P = params
        self.plane = plane
        self.bare = make_oracle(params, camera, T)
        self.bare.set_cloud(cloud)
        self.bare.set_ground_plane(None, None)
        self.ref = self.bare
        if plane is not None:
            self.ref = make_oracle(params, camera, T)
            self.ref.set_cloud(cloud)
            self.ref.set_ground_plane(*plane)
        self.Tinv, _ = self.bare.calibration()
        self.cam = np.ascontiguousarray(self.bare.cloud_camera_cs().T)  # [n, 3]
        self.index = self.bare.point_index()
        self.pixel_map = self.bare.pixel_map()
        self.n_points = int(cloud.shape[0])

    def mask_words(self):
        """The plane's inlier bitmask as mld_set_clouds_planes_range_device takes it (None without a plane)."""
        if self.plane is None:
            return None
        bits = np.zeros(((self.n_points + 31) // 32) * 32, dtype=bool)
        bits[np.asarray(self.plane[1], dtype=np.int64)] = True
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()

    def trace(self, uv):
        """(records [F] of DTYPE, lists: per feature a dict nb / seg / road / road_inl of int32 arrays, the oracle's
        final (types, depths) with the plane)."""
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        F = uv.shape[0]
        P = self.P
        main_depth, main_type = self.bare.calculate_depth(uv) if F else (np.empty(0), np.empty(0, np.int32))
        rec = np.zeros(F, dtype=DTYPE)
        lists, final_t, final_d = [], np.zeros(F, np.int32), np.zeros(F)
        for i in range(F):
            u, v = float(uv[i, 0]), float(uv[i, 1])
            t = self.ref.trace_feature(u, v)
            final_t[i], final_d[i] = t["type"], t["depth"]
            r = rec[i]
            nb, seg = t["nb_idx"], t["seg_pos"]
            r["main_type"], r["main_depth"] = main_type[i], main_depth[i]
            r["n_nb"], r["n_seg"] = nb.size, seg.size
            r["flags"] = 0 if np.isfinite(u) and np.isfinite(v) else NONFINITE
            r["hist_lower"] = r["hist_higher"] = -1.0
            if P.do_use_histogram_segmentation and main_type[i] != 2:
                z = np.minimum(self.cam[self.index[nb], 2], 999.0)  # DepthEstimator.cpp:743
                ok, keep, lo, hi = oracle.filter_points_min_dist_blob(z, P.histogram_segmentation_bin_witdh,
                                                                      P.histogram_segmentation_min_pointcount)
                if ok:
                    assert np.array_equal(keep, seg)
                else:
                    assert seg.size == 0 and main_type[i] == 3 and lo == -1.0 and hi == -1.0
                r["hist_lower"], r["hist_higher"] = lo, hi
            cp = np.asarray(t["corner_pos"], dtype=np.int32)
            r["corner_pos"] = cp
            r["corner_vis"] = -1
            r["corners"] = np.nan
            r["plane_n"] = np.nan
            r["plane_offset"] = np.nan
            if cp[0] >= 0:
                vis = nb[seg[cp]]
                r["corner_vis"] = vis
                r["corners"] = self.cam[self.index[vis]].reshape(-1)
                if main_type[i] != 8:  # (TriangleNotPlanar leaves before Hyperplane::Through)
                    r["plane_n"], r["plane_offset"] = t["plane_n"], t["plane_offset"]
            road, road_inl = t["road_idx"], t["road_pos"]
            state = NOT_REACHED
            if t["reached_road"]:
                assert main_type[i] not in (1, 2)
                if road.size < (int(P.radiusSearch_count_min) & 0xFFFFFFFF):  # :585-586, compared as unsigned
                    state = FEW_NEIGHBOURS
                elif far_mask(self.Tinv, self.plane[0], self.cam[self.index[road]],
                              P.ransac_plane_point_distance_treshold).any():
                    state = FAR_NEIGHBOUR
                    assert road_inl.size == 0
                else:
                    state = FEW_INLIERS if road_inl.size < 3 else FIT
                if state in (FAR_NEIGHBOUR, FEW_INLIERS):
                    assert t["type"] == main_type[i] and t["depth"] == -1.0
            else:
                assert t["type"] == main_type[i]
            r["road_state"], r["n_road"], r["n_road_inl"] = state, road.size, road_inl.size
            lists.append(dict(nb=nb.astype(np.int32), seg=seg.astype(np.int32), road=road.astype(np.int32),
                              road_inl=road_inl.astype(np.int32)))
        return rec, lists, (final_t, final_d)


def same_records(got, want):
    """Equality of two record arrays, field by field: integers, and the raw bits of the floats (the sign of a zero
    included); where one side holds a NaN the other must hold one too, whatever its payload - a NaN that arithmetic made
    carries the sign the machine gives it.  Returns the names of the fields that differ."""
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


# ---- the small frames both test files use: a 64 x 64 camera with identity T (x_cam = x_lidar) ----------------------
SMALL_W = SMALL_H = 64
SMALL_F, SMALL_C = 64.0, 32.0


def pixel_cloud(pixels, depths):
    """One point in the middle of every pixel of `pixels` ([k, 2] integers x, y) at the camera-frame depth depths[k]."""
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    z = np.asarray(depths, dtype=np.float64).reshape(-1)
    cl = np.zeros((px.shape[0], 4), dtype=np.float32)
    cl[:, 0] = (px[:, 0] + 0.5 - SMALL_C) / SMALL_F * z
    cl[:, 1] = (px[:, 1] + 0.5 - SMALL_C) / SMALL_F * z
    cl[:, 2] = z
    return cl


def sparse_cloud(seed=1, density=0.04):
    """Few points: windows of the C0 search area hold 0, 1, 2, 3 ... of them.  Two thirds of the depths lie in one
    histogram bin (10.21 .. 10.45 m), the rest anywhere in 4 .. 30 m."""
    rng = np.random.default_rng(4100 + seed)
    ys, xs = np.nonzero(rng.random((SMALL_H, SMALL_W)) < density)
    order = rng.permutation(xs.size)  # (cloud order is not scan order)
    z = np.where(rng.random(xs.size) < 0.67, rng.uniform(10.21, 10.45, xs.size), rng.uniform(4.0, 30.0, xs.size))
    return pixel_cloud(np.stack([xs, ys], axis=1)[order], z)


def dense_cloud(seed=2, holes=0.1):
    """One point per pixel but for a tenth of them.  The upper half of the image lies in ONE histogram bin of width 0.3
    (10.21 .. 10.45 m: bin 34), so that whole windows survive the segmentation; the lower half is scattered over
    8 .. 13 m, where the segmentation, the planarity test and the thresholds reject."""
    rng = np.random.default_rng(4200 + seed)
    ys, xs = np.nonzero(rng.random((SMALL_H, SMALL_W)) >= holes)
    z = np.where(ys < SMALL_H // 2, rng.uniform(10.21, 10.45, xs.size), rng.uniform(8.0, 13.0, xs.size))
    return pixel_cloud(np.stack([xs, ys], axis=1), z)


COLLINEAR_CAM = (16, 16, 16.0, 8.0, 8.0)  # CameraPinhole(width, height, focal length, principal point)
COLLINEAR_PIXEL = (9, 8)


def collinear_cloud():
    """Three points p, p + d, p + 2 d on the identity transform, every coordinate and every difference exact in f32 and f64:
    the cross product of the triangle's edges is exactly zero, so Hyperplane::Through takes its degenerate branch (the
    smallest eigenvector).  On the 16 x 16 camera COLLINEAR_CAM they fall into the pixels (8, 7), (9, 8) and (10, 8), all of
    them in the narrow C0 window of COLLINEAR_PIXEL, and nothing else is in the cloud."""
    cl = np.zeros((3, 4), dtype=np.float32)
    cl[:, :3] = [(0.25, -0.5, 9.5), (1.0, 0.0, 10.0), (1.75, 0.5, 10.5)]
    return cl


def collinear_parameters():
    """C0 with the planarity check off (it would reject the triangle before the plane), the histogram off, no road fallback;
    triangle maximisation stays on."""
    P = capi.params_c0().replace(do_check_triangleplanar_condition=0, do_use_histogram_segmentation=0, do_use_ransac_plane=0)
    assert P.do_use_triangle_size_maximation == 1
    return P


def small_features(n, seed=0):
    """The four corners and borders of the image, positions outside it, NaN and +-inf first; then random ones, every
    other one on an integer pixel."""
    special = [(0.0, 0.0), (63.0, 63.0), (0.0, 63.0), (63.0, 0.0), (31.5, 0.0), (0.0, 31.25), (63.9, 20.0), (20.0, 63.9),
               (-3.0, 10.0), (70.0, 70.0), (10.0, -20.0), (np.nan, 10.0), (np.inf, 10.0), (10.0, -np.inf), (np.nan, np.nan),
               (66.5, 5.0), (64.0, 64.0), (-0.0, -0.0), (3.0, 3.0), (2.0, 40.0)]
    rng = np.random.default_rng(4300 + seed)
    uv = np.stack([rng.uniform(-2.0, 66.0, n), rng.uniform(-2.0, 66.0, n)], axis=1)
    uv[::2] = np.floor(uv[::2])
    k = min(n, len(special))
    uv[:k] = np.asarray(special[:k], dtype=np.float64).reshape(k, 2)
    return np.ascontiguousarray(uv)


def small_plane(cloud, seed=0, offset=10.3, fraction=0.5):
    """A plane z = offset in the lidar (= camera) frame and a random half of the cloud as its inliers."""
    rng = np.random.default_rng(4400 + seed)
    inl = np.nonzero(rng.random(cloud.shape[0]) < fraction)[0].astype(np.int32)
    return np.array([0.0, 0.0, 1.0, -offset], dtype=np.float32), inl


def dense_features():
    """Every fourth integer pixel of the 64 x 64 image (256 features: windows cut by the borders and full ones), then
    the special positions of small_features()."""
    g = np.arange(0.0, SMALL_W, 4.0)
    grid = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([grid, small_features(20)]))
