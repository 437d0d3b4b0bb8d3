"""Random configurations for the batch units (depth images, feature traces, coverage maps, nearest depths, row growth): the
parameter set, camera, mounting and scanner of test_randomized_gpu._random_setup(seed), with the camera scaled down so that the
oracle can answer at EVERY pixel in well under a second and the windows hold enough returns to overflow a lane's 32-entry
list, and the parameters changed only where the unit's refuse_config says so.  No GPU is used here."""
import functools

import numpy as np

from mono_lidar_depth_amd import CameraPinhole, synth

from test_randomized_gpu import _random_setup

# Fixed numbers: what they reach together is asserted in test_batch_units_randomized_cpu.py.
SEEDS = tuple(range(12))
UNITS = ("images", "traces", "coverage", "nearest", "rows")
# What a unit's refuse_config refuses of what _random_setup can draw.
ADAPT = {"images": dict(do_use_PCA=0, plane_estimator_use_triangle_maximation=0, plane_estimator_use_mestimator=1),
         "traces": dict(do_use_PCA=0), "coverage": dict(do_use_PCA=0), "nearest": dict(do_use_PCA=0),
         "rows": dict(do_use_PCA=0, set_all_depths_to_zero=0)}


def wide_window(P, W, H):
    """Upper bound on the (columns, rows) of the wide window (2.0 x 1.5 the search area) on a W x H image: floor(2 half) +
    2, and no more than the image has - the bound the units' refusals use."""
    nx = int(np.floor(2.0 * (P.pixelarea_search_witdh * 0.5 * 2.0))) + 2
    ny = int(np.floor(2.0 * (P.pixelarea_search_height * 0.5 * 1.5))) + 2
    return min(nx, W), min(ny, H)


@functools.lru_cache(maxsize=None)
def _frame(seed):
    """The seed's cloud and plane, made once and read-only."""
    cloud = synth.make_cloud(_random_setup(seed)[3], seed=200 + seed, frame=seed % 5)
    coeffs, inliers = synth.make_ground_plane(cloud)
    for a in (cloud, coeffs, inliers):
        a.setflags(write=False)
    return cloud, (coeffs, inliers)


def setup(seed, unit):
    """(P, camera, T, cloud, plane) of `seed` for `unit` (one of UNITS); plane = (coeffs, inlier indices)."""
    P, cam, T, _, _ = _random_setup(seed)
    cloud, plane = _frame(seed)
    k = 8 if cam.width > 1242 else 4
    camera = CameraPinhole(cam.width // k, cam.height // k, cam.focal_length / k, cam.principal_point_x / k,
                           cam.principal_point_y / k)
    P = P.replace(**ADAPT[unit])
    nx, ny = wide_window(P, camera.width, camera.height)
    if unit == "coverage":
        assert nx <= 64 and ny <= 64, (seed, nx, ny)  # (more is refused: no seed may need it)
    else:
        assert nx * ny <= 1024, (seed, nx, ny)
    return P, camera, T, cloud, plane
