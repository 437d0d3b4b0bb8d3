"""What the depth-image tests share: the frames, the oracle's arrays of a frame as the inputs of
mld_depth_images_render_device, and the oracle's answer on a grid.  No GPU is used here."""
import numpy as np

from mono_lidar_depth_amd import CameraPinhole, capi

import feature_trace_restatement as R
from helpers import make_oracle

SMALL_CAM = CameraPinhole(64, 64, 64.0, 32.0, 32.0)
SMALL_T = np.eye(4)[:3].copy()
# include/mld.h, mld_depth_image_record: (field, offset, bytes)
LAYOUT = [("counts", 0, 168), ("n_pixels", 168, 8), ("n_depth", 176, 8), ("n_cooperative", 184, 8), ("flags", 192, 4),
          ("pad_", 196, 4)]
DTYPE = np.dtype(capi.MldDepthImageRecord)
BAD_INPUT, HAS_PLANE = 1, 2


def camera(W, H):
    """A W x H image with the focal length and the principal point of the 64 x 64 camera: R.pixel_cloud puts a point into
    the middle of pixel (x, y) for it, whatever the image size."""
    return CameraPinhole(W, H, 64.0, 32.0, 32.0)


def grid_of(W, H, grid=None):
    """(x0, y0, step_x, step_y, grid_w, grid_h): None is every pixel, four values take as many pixels as fit."""
    if grid is None:
        return 0, 0, 1, 1, W, H
    if len(grid) == 4:
        x0, y0, sx, sy = grid
        return x0, y0, sx, sy, (W - 1 - x0) // sx + 1, (H - 1 - y0) // sy + 1
    return tuple(grid)


def grid_uv(g):
    """The features of a grid, [grid_w * grid_h, 2] float64 in output order (i + j * grid_w)."""
    x0, y0, sx, sy, gw, gh = g
    xs = x0 + sx * np.arange(gw, dtype=np.float64)
    ys = y0 + sy * np.arange(gh, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2))


class Frame:
    """One sequence: the oracle on (P, cam, T, cloud, plane) and its arrays - pixel map, point index, camera-frame cloud,
    the plane's bit mask - which are the inputs of a render call.  plane: (coeffs, inliers) or None."""

    def __init__(self, P, cam, T, cloud, plane):
        self.P, self.cam_model, self.T, self.cloud, self.plane = P, cam, T, cloud, plane
        st = cam.as_struct()
        self.W, self.H = int(st.width), int(st.height)
        self.ref = make_oracle(P, cam, T)
        self.ref.set_cloud(cloud)
        if plane is None:
            self.ref.set_ground_plane(None, None)
        else:
            self.ref.set_ground_plane(*plane)
        self.n_points = int(cloud.shape[0])
        self.pm = np.ascontiguousarray(self.ref.pixel_map().reshape(self.H, self.W)).copy()
        self.index = np.ascontiguousarray(self.ref.point_index()).copy()
        self.cam = np.ascontiguousarray(self.ref.cloud_camera_cs().T).copy() if self.n_points else np.zeros((0, 3))
        self.coeffs = np.asarray(plane[0], dtype=np.float32) if plane is not None else np.zeros(4, dtype=np.float32)
        self._full = {}

    def mask_words(self):
        if self.plane is None:
            return None
        bits = np.zeros(((self.n_points + 31) // 32) * 32, dtype=bool)
        bits[np.asarray(self.plane[1], dtype=np.int64)] = True
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.int32).reshape(-1).copy()

    def expected(self, grid=None, n_threads=8):
        """(depth [gh, gw] float64, types [gh, gw] int32) of the oracle on the grid; the full grid is computed once."""
        g = grid_of(self.W, self.H, grid)
        if "full" not in self._full:
            d, t = self.ref.calculate_depth(grid_uv(grid_of(self.W, self.H)), n_threads)
            self._full["full"] = (d.reshape(self.H, self.W), t.reshape(self.H, self.W))
        d, t = self._full["full"]
        x0, y0, sx, sy, gw, gh = g
        ys = y0 + sy * np.arange(gh)
        xs = x0 + sx * np.arange(gw)
        return d[np.ix_(ys, xs)].copy(), t[np.ix_(ys, xs)].copy()


def pixel_frame(W, H, density, seed, P=None, plane=True):
    """R.pixel_cloud with one point in a fraction `density` of the pixels of a W x H image, on the identity transform: the
    upper half in one histogram bin, the rest anywhere in 8 .. 13 m, in shuffled order, and a plane z = 10.3 m with a
    random half of the points as inliers."""
    rng = np.random.default_rng(7700 + seed)
    ys, xs = np.nonzero(rng.random((H, W)) < density)
    order = rng.permutation(xs.size)
    xs, ys = xs[order], ys[order]
    z = np.where(ys < H // 2, rng.uniform(10.21, 10.45, xs.size), rng.uniform(8.0, 13.0, xs.size))
    cl = R.pixel_cloud(np.stack([xs, ys], axis=1), z)
    pl = None
    if plane:
        pl = (np.array([0.0, 0.0, 1.0, -10.3], dtype=np.float32), np.nonzero(rng.random(xs.size) < 0.5)[0].astype(np.int32))
    return Frame(P if P is not None else capi.params_c0(), camera(W, H), SMALL_T, cl, pl)


def mixed_frame():
    from test_coverage_maps_cpu import mixed_cloud
    cl = mixed_cloud()
    return Frame(capi.params_c0(), SMALL_CAM, SMALL_T, cl, R.small_plane(cl))


def golden_frame():
    from test_golden import load_case
    g = load_case("c0")
    cam = CameraPinhole(g["cam"].width, g["cam"].height, g["cam"].focal_length, g["cam"].principal_point_x, g["cam"].principal_point_y)
    return Frame(g["P"], cam, g["T"], g["cloud"], g["plane"])
