"""NumPy restatement of mld_plane_inliers_export_device: the inlier list, the lidar-frame matrix and the camera-frame
cloud of a ground plane, from the cloud and the plane's inlier bitmask.  The camera coordinates come from the oracle
(the way expected() in test_projected_clouds_gpu.py obtains them); everything else is np.unpackbits and a comparison."""
import numpy as np

from mono_lidar_depth_amd import capi

from helpers import make_oracle


def mask_bits(words, n):
    """The first n bits of the mask words as booleans: bit i of word i / 32 is point i (whatever lies beyond n is cut)."""
    w = np.ascontiguousarray(words).view(np.uint32).astype("<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def words_of(bits):
    """The mask words of a boolean array (the bits beyond its length are 0)."""
    n = len(bits)
    padded = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def camera_cs(cloud, camera=None, T=None):
    """[n, 3] f64: the oracle's camera-frame cloud (getCloudCameraCs)."""
    if cloud.shape[0] == 0:
        return np.empty((0, 3))
    ref = make_oracle(capi.params_c0(), camera, T)
    ref.set_cloud(np.ascontiguousarray(cloud[:, :4], dtype=np.float32))
    return np.ascontiguousarray(ref.cloud_camera_cs().T)


def restate(cloud, words, use_camx=False, thr=0.0, camera=None, T=None, cam=None):
    """{n_inliers, n_cloud, index int32 [k], lidar f32 [k, 3], cam f64 [m, 3], keep bool [k]} of one sequence.  `cam`: the
    camera-frame cloud where the caller has it already."""
    n = cloud.shape[0]
    index = np.flatnonzero(mask_bits(words, n)).astype(np.int32)
    if cam is None:
        cam = camera_cs(cloud, camera, T)
    picked = cam[index]
    if use_camx:
        with np.errstate(invalid="ignore"):
            keep = ~(~(np.abs(picked[:, 0]) <= thr))  # NaN fails (DepthEstimator.cpp:300-307)
    else:
        keep = np.ones(index.size, dtype=bool)
    out = dict(n_inliers=int(index.size), n_cloud=int(keep.sum()), index=index,
               lidar=np.ascontiguousarray(cloud[index, :3], dtype=np.float32), cam=np.ascontiguousarray(picked[keep]), keep=keep)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
