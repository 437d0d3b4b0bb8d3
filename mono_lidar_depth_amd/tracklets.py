"""Python mirror of tracklets_depth::TrackletDepthModule around the DepthEstimator boundary.

Reference: tracklets_depth/src/tracklet_depth_module.cpp — process :261-396, ExractNewTrackletFrames :23-61,
CalculateFeatureDepthsCurFrame :63-82, CalculateFeatureDepthsLastFrame :84-117, SaveFeatureDepths :119-169,
TidyUpTracklets :171-193.  The ROS message plumbing is out of scope; tracks arrive as arrays.

What runs on the GPU: the feature gather (newest feature of every track, previous feature of NEW tracks, truncated
to integer pixels), both CalculateDepth calls and the float32 scatter — one C-ABI call, `mld_tracklets_depth*`.
The previous frame is NOT re-projected as the reference does (:115 -> setInputCloud): its frame slot (cloud, pixel
map, ground plane) is kept and the two slots ping-pong.  The tracklet map itself (ids seen so far, per-track
history) is host bookkeeping in the one-frame TrackletDepthModule, kept here in Python; at batch size it lives on the
GPU: TrackletStore (mld_tracks_*) decides the new tracks, keeps the histories, drops the dead tracks, exports the
stored tracks in message order and takes a packed export back in (import_packed: a store continues in another store,
on another context or GPU), and TrackletBatch.step runs a whole frame of every sequence with it - the sequences being
lanes that start, restart (restart=...) and resume (set_previous) independently.  SemanticLabels
(mld_labels_*) is the node that follows tracklets_depth in the reference's launch files: the label of every track by
majority vote in a window of a label image (matches_conversion_ros_tool, semantic_labels.cpp:50-72).  SemanticPlanes
(mld_semantic_planes_*) is the ground plane process() builds from the label image of every frame (:269-284), for all
sequences of a batch in one call and ahead of the projection.  ProjectedClouds (mld_projected_clouds_*) is the frame's
PointcloudData - visible list, point index, camera-frame cloud, pixel map - of all sequences as device tensors.
DepthReports (mld_depth_reports_*) is the depth-calculation statistics (getDepthCalcStats) and the interpolated cloud
(getCloudInterpolated) of all sequences, from device tensors into device tensors.  PlaneInliers (mld_plane_inliers_*) is
the inlier index list, lidar-frame matrix and camera-frame cloud of the ground planes of all sequences, from their masks.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import capi
from .depth_estimator import (NO_PLANE, CameraPinhole, DepthEstimator, DepthEstimatorError, ExceptionPclInvalid,
                              GroundPlane, RansacPlane, SemanticPlane, _is_torch_cuda)


class TrackletDepthModule:
    def __init__(self, parameters, camera: CameraPinhole, transform_lidar_to_cam, device: int = 0,
                 keep_history: bool = True):
        self._est = DepthEstimator(device=device, max_frames=2)
        self._est.InitConfig(parameters)
        self._est.Initialize(camera, transform_lidar_to_cam)
        self._slot_cur = 0
        self._have_last = False  # _cloud_last_frame != nullptr
        self._keep_history = keep_history
        self.one_call = True  # process() = one C call (mld_tracklets_frame); False: setInputCloud + mld_tracklets_depth
        # _trackletMap: id -> list of (u, v, depth), newest first (feature_tracking::Tracklet::push_front)
        self._tracklet_map: Dict[int, List[Tuple[int, int, float]]] = {}

    @property
    def estimator(self) -> DepthEstimator:
        return self._est

    def known_ids(self):
        return self._tracklet_map.keys()

    def process(self, cloud, ids, u_new, v_new, u_old, v_old, ground_plane: Optional[GroundPlane], img=None):
        """One frame (tracklet_depth_module.cpp:261-396).  With a semantic label image `img` (the 4-argument
        overload, :261-284) the ground plane is a SemanticPlane with labels {6,7,8,9} and the inlier threshold
        ransac_plane_refinement_treshold, and `ground_plane` is ignored.

        ids: track ids; u_new/v_new: newest feature of every track (feature_points[0]); u_old/v_old: previous
        feature (feature_points[1]; only read for tracks that are new to the module).  Returns
        (d_cur, d_last, is_new): float32 depths of the newest features, float32 depths of the previous features
        (NaN where the track is not new) and the new-track mask.
        """
        est, lib = self._est, self._est._lib
        ids = np.asarray(ids, dtype=np.int64)
        n = int(ids.size)
        known = self._tracklet_map
        is_new = np.fromiter((int(i) not in known for i in ids), dtype=np.uint8, count=n)  # :31
        slot_cur = self._slot_cur
        slot_last = (1 - slot_cur) if self._have_last else -1
        import time
        t_abi = time.perf_counter()
        if img is not None:
            ground_plane = SemanticPlane(img, (6, 7, 8, 9), est.getParameters().ransac_plane_refinement_treshold)
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (u_new, v_new, u_old, v_old)]
        d_cur = np.empty(n, dtype=np.float32)
        d_last = np.full(n, np.nan, dtype=np.float32)
        t_cur = np.empty(n, dtype=np.int32)
        t_last = np.zeros(n, dtype=np.int32)
        n_new = C.c_int64(0)
        if self.one_call and not _is_torch_cuda(cloud) and self._frame_call(cloud, ground_plane, slot_cur, slot_last, arrs,
                                                                            is_new, n, d_cur, d_last, t_cur, t_last, n_new):
            pass  # the whole GPU side of process() was ONE C call (mld_tracklets_frame)
        else:
            est.setInputCloud(cloud, ground_plane, slot=slot_cur)  # the only projection of this frame
            est._check(lib.mld_tracklets_depth(est._ctx, slot_cur, slot_last, *[a.ctypes.data for a in arrs],
                                               is_new.ctypes.data, n, d_cur.ctypes.data, d_last.ctypes.data,
                                               t_cur.ctypes.data, t_last.ctypes.data, C.byref(n_new)))
        self.last_types = (t_cur, t_last)
        self.last_abi_seconds = time.perf_counter() - t_abi  # C-ABI calls only (copies, kernels, synchronise)
        # SaveFeatureDepths (:119-169) + TidyUpTracklets (:171-193)
        updated = {}
        ui0, vi0 = arrs[0].astype(np.int32), arrs[1].astype(np.int32)
        ui1, vi1 = arrs[2].astype(np.int32), arrs[3].astype(np.int32)
        for i in range(n):
            tid = int(ids[i])
            hist = known.get(tid)
            if hist is None:
                hist = [(int(ui1[i]), int(vi1[i]), float(d_last[i]))]
            elif not self._keep_history:
                hist = []
            hist.insert(0, (int(ui0[i]), int(vi0[i]), float(d_cur[i])))
            updated[tid] = hist
        self._tracklet_map = updated  # tracks without an update this frame are dropped
        # remember cloud / plane: the current slot becomes the previous one (:348, :357)
        self._have_last = True
        self._slot_cur = 1 - slot_cur
        return d_cur, d_last, is_new.astype(bool)

    def _frame_call(self, cloud, gp, slot_cur, slot_last, arrs, is_new, n, d_cur, d_last, t_cur, t_last, n_new) -> bool:
        """The GPU side of process() as one C call: upload, ground plane (estimated inside the call when it is not
        segmented yet - what the reference does every frame, tracklet_depth_module.cpp:269-284), projection, feature
        marshalling, both CalculateDepth calls, scatter.  False: not applicable (device inputs)."""
        est, lib = self._est, self._est._lib
        road = bool(est.getParameters().do_use_ransac_plane)
        if road and gp is None:
            gp = RansacPlane()
        ptr, npts, stride, keep = est._cloud_view(cloud)
        req = None
        coeffs = inl = None
        n_inl = 0
        hold = None
        if road and gp is not NO_PLANE:
            if isinstance(gp, RansacPlane) and not gp.isSegmented():
                req = capi.MldPlaneRequest()
                req.kind, req.seed = capi.MLD_PLANE_RANSAC, gp.seed & 0xFFFFFFFF
                if isinstance(gp, SemanticPlane):
                    if _is_torch_cuda(gp.img):
                        return False
                    im = np.ascontiguousarray(gp.img, dtype=np.uint8)
                    lab = np.ascontiguousarray(gp.groundplane_label, dtype=np.int32)
                    hold = (im, lab)
                    req.kind = capi.MLD_PLANE_SEMANTIC
                    req.label_image, req.rows, req.cols, req.row_stride_bytes = im.ctypes.data, im.shape[0], im.shape[1], im.strides[0]
                    req.ground_labels, req.n_labels, req.inlier_threshold = lab.ctypes.data, lab.size, gp.inlier_threshold
            else:
                if not isinstance(gp, GroundPlane) or _is_torch_cuda(gp.inliers):
                    return False
                ii = gp.getInlinersIndex()
                if ii is None:
                    return False
                inl = np.ascontiguousarray(ii, dtype=np.int32)
                coeffs = (C.c_float * 4)(*[float(x) for x in gp.coeffs])
                n_inl = int(inl.size)
        res = capi.MldPlaneResult()
        rc = lib.mld_tracklets_frame(est._ctx, slot_cur, slot_last, ptr, npts, stride, C.byref(req) if req is not None else None,
                                     coeffs, inl.ctypes.data if inl is not None else None, n_inl,
                                     *[a.ctypes.data for a in arrs], is_new.ctypes.data, n, d_cur.ctypes.data,
                                     d_last.ctypes.data, t_cur.ctypes.data, t_last.ctypes.data, C.byref(n_new), C.byref(res))
        del hold, keep
        if rc == capi.MLD_ERR_CLOUD_TOO_SMALL:
            # the reference's process() catches ExceptionPclInvalid per frame (:318-347): the previous frame's features
            # are answered, the current frame continues with invalid depths, cloud and plane are forgotten
            raise ExceptionPclInvalid(rc, "In GroundPlane: Input pointcloud is invalid")
        est._check(rc)
        if req is not None:
            gp.coeffs = np.array(list(res.coeffs), dtype=np.float32)
            gp.inliers = None
            gp.n_inliers = int(res.n_inliers)
            gp.iterations = int(res.iterations)
            gp._segmented = True
            gp._owner = (est, slot_cur)
        return True

    def tracklet(self, track_id: int):
        return list(self._tracklet_map[track_id])


def mask_words(n_points: int) -> int:
    """32-bit words of the inlier mask of a cloud of n_points."""
    return (int(n_points) + 31) // 32


def _at(ts, s):
    """Entry s of a table that may be absent."""
    return ts[s] if ts is not None else None


def _entries(t, per: int = 1) -> int:
    """Whole groups of `per` elements a tensor holds (None: 0)."""
    return int(t.numel()) // per if t is not None else 0


def _holds(t, s, entries, size, name, required=False):
    """Tensor `t` of sequence s is contiguous, of `size`-byte elements and at least `entries` long.  None passes,
    unless `required` and entries > 0."""
    if t is None:
        if required and entries:
            raise ValueError(f"sequence {s}: {name} is missing")
        return
    if t.element_size() != size or not t.is_contiguous() or int(t.numel()) < entries:
        raise ValueError(f"sequence {s}: {name} must be contiguous, of {size}-byte elements, at least {entries} of them")


def _mask_room(t, s, n_points, name):
    """Tensor `t` has room for the inlier mask of n_points, counted in bytes whatever its element type."""
    if t is None or int(t.numel()) * t.element_size() < 4 * mask_words(n_points):
        raise ValueError(f"sequence {s}: {name} holds fewer than {mask_words(n_points)} words")


def _cloud_table(clouds, none_allowed=True):
    """(width, ns) of the clouds of a call: contiguous float32 [n, 4] or [n, 8] of one width.  An entry None is a
    sequence without points where `none_allowed`, else refused."""
    width = next((int(cl.shape[1]) for cl in clouds if cl is not None and cl.dim() == 2), 4)
    ns = []
    for s, cl in enumerate(clouds):
        if cl is None and not none_allowed:
            raise ValueError(f"sequence {s}: clouds is missing")
        if cl is not None and (cl.dim() != 2 or int(cl.shape[1]) != width or width not in (4, 8) or not cl.is_contiguous()
                               or cl.element_size() != 4):
            raise ValueError("clouds: contiguous float32 [n, 4] or [n, 8], one width for all sequences")
        ns.append(int(cl.shape[0]) if cl is not None else 0)
    return width, ns


def _capacities(capacity, ns, clamp=False):
    """The capacity of every sequence: capacity[s], or ns[s] without a table; a negative one is refused.  clamp: at most
    ns[s] - what TrackletBatch allocates."""
    caps = []
    for s, n in enumerate(ns):
        cap = n if capacity is None else int(capacity[s])
        if cap < 0:
            raise ValueError(f"sequence {s}: negative capacity")
        caps.append(min(cap, n) if clamp else cap)
    return caps


def _result_tensor(t, shape, size, name):
    """Tensor `t`, which receives the records of a call, is contiguous, of exactly `shape` and of `size`-byte elements."""
    if tuple(t.shape) != tuple(shape) or t.element_size() != size or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous int{8 * size} tensor {list(shape)}")


class _BatchObject:
    """What TrackletStore, SemanticLabels, SemanticPlanes, RansacPlanes, ProjectedClouds, DepthReports, PlaneInliers,
    FeatureTraces, CoverageMaps, DepthImages, RegionDepths, NearestDepths, SweepMerge and RowGrowth share: an object of the C-ABI (mld_<_NAME>_create / _destroy /
    _last_error) on an estimator's context, its handle in the attribute named _HANDLE, the tensors of the calls that may
    still be queued, and one copy of every argument check.  The helpers, here and above:

    _calibration     the parameter, camera and transform arguments of _create
    _create, close   the object of the C-ABI; _check raises its last error for a status that is not MLD_OK
    _lengths         every list given holds one entry per sequence
    _ptrs, _opt      the pointer table of S tensors; _opt: NULL for a table that is absent
    _i64             a table of S int64 (None: NULL)
    _plane_args      plane coefficients and masks, which come together or not at all
    _image_geometry  (rows, cols, row stride) the label images share
    _hold            keeps the tensors of a call alive for two calls
    _holds           a tensor is contiguous, of the element size and long enough; _mask_room: for a mask, in bytes
    _cloud_table     (width, ns) of the clouds
    _capacities      the capacity table, as given or clamped to the clouds
    _result_tensor   the fixed shape of a tensor that receives records
    _at, _entries    an entry of an optional table; the entries of an optional tensor
    mask_words       words of an inlier mask"""

    _NAME = _HANDLE = ""

    def _calibration(self, estimator: DepthEstimator, *parts, parameters=None):
        """The arguments of _create named in `parts`, in that order: "parameters" (the given ones, else the estimator's),
        "camera" (also sets self.width and self.height), "transform" (its first 12 doubles).  Each keeps its object alive."""
        out = []
        for part in parts:
            if part == "parameters":
                out.append(C.byref(parameters if parameters is not None else estimator.getParameters()))
            elif part == "camera":
                cam = estimator._camera.as_struct()
                self.width, self.height = int(cam.width), int(cam.height)
                out.append(C.byref(cam))
            else:
                T = np.ascontiguousarray(np.asarray(estimator._T, dtype=np.float64).reshape(-1)[:12])
                out.append(T.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def _create(self, estimator: DepthEstimator, *args):
        self._est, self._lib = estimator, estimator._lib
        st = C.c_int(0)
        handle = getattr(self._lib, f"mld_{self._NAME}_create")(estimator._ctx, *args, C.byref(st))
        setattr(self, self._HANDLE, handle)
        if not handle:
            raise DepthEstimatorError(st.value, self._last_error(None))
        self._keep = {}

    def _last_error(self, handle) -> str:
        return getattr(self._lib, f"mld_{self._NAME}_last_error")(handle).decode()

    def _check(self, rc: int):
        if rc != capi.MLD_OK:
            raise DepthEstimatorError(rc, self._last_error(getattr(self, self._HANDLE)))

    def _lengths(self, **lists):
        """Every list given holds one entry per sequence (None: the list is absent and not looked at)."""
        for name, ts in lists.items():
            if ts is not None and len(ts) != self.S:
                raise ValueError(f"{name}: expected {self.S} entries, one per sequence")

    def _ptrs(self, ts):
        """The table of the S device pointers of `ts` (an entry None: NULL)."""
        return (C.c_void_p * self.S)(*[int(t.data_ptr()) if t is not None else None for t in ts])

    def _opt(self, ts):
        """_ptrs of a table that may be absent (None: NULL)."""
        return self._ptrs(ts) if ts is not None else None

    def _i64(self, values):
        """The table of S int64 `values` (None: NULL)."""
        return (C.c_int64 * self.S)(*values) if values is not None else None

    def _plane_args(self, coeffs, masks):
        """(pointer to the float32 [S, 4] coefficients, mask table) of the planes of a call: both or neither."""
        if (coeffs is None) != (masks is None):
            raise ValueError("coeffs and masks come together or not at all")
        if coeffs is None:
            return None, None
        co = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(self.S, 4)
        return co.ctypes.data_as(C.POINTER(C.c_float)), self._ptrs(masks)

    def _hold(self, *now, call=None):
        """The arrays must outlive the asynchronous launches (the previous call's as well: it may still be queued).
        `now`: tensors, lists of tensors and Nones as the call took them."""
        prev = self._keep.get(call)
        self._keep[call] = (prev[1] if prev else None, [list(x) if isinstance(x, (list, tuple)) else x for x in now])

    @staticmethod
    def _image_geometry(images):
        """(rows, cols, row stride) that all label images of a call must share."""
        rows, cols = (int(x) for x in images[0].shape)
        stride = int(images[0].stride(0))
        for im in images:
            if tuple(im.shape) != (rows, cols) or (rows > 1 and int(im.stride(0)) != stride) or int(im.stride(1)) != 1:
                raise ValueError("images: one shape and row stride for all sequences, unit column stride")
        return rows, cols, stride

    def close(self):
        handle = getattr(self, self._HANDLE)
        if handle:
            getattr(self._lib, f"mld_{self._NAME}_destroy")(handle)
            setattr(self, self._HANDLE, None)
        self._keep = {}

    def __del__(self):
        try:
            if self._est._ctx is not None:  # (the estimator took the stream with it otherwise)
                self.close()
        except Exception:
            pass


class TrackletStore(_BatchObject):
    """`_trackletMap` of S independent sequences in GPU memory (mld_tracks_*, include/mld.h): begin = which ids are new
    (ExractNewTrackletFrames :23-61), commit = SaveFeatureDepths + TidyUpTracklets (:119-193), export =
    convert_tracklets_to_matches_msg (:209-259).  Histories hold at most `max_history` entries per track (the
    reference's deque is unbounded; export_leaving() hands out what falls off and the tracks that end, TrackArchive
    puts them together).  Lists of S torch CUDA tensors in and out; asynchronous on the estimator's stream,
    only counts() synchronises.  Close the store before its estimator."""

    COUNT_NAMES = ("live", "new", "old", "features_ok", "features_failed", "duplicates")
    _NAME, _HANDLE = "tracks", "_tr"

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_tracks: int, max_history: int):
        self.S, self.max_tracks, self.max_history = int(n_seq), int(max_tracks), int(max_history)
        self._create(estimator, self.S, self.max_tracks, self.max_history)

    def begin(self, ids, is_new_out=None):
        """ids: S int32 CUDA tensors; is_new_out: S uint8 CUDA tensors of the same lengths, or None (masks kept in
        the store).  The ids are read again by commit()."""
        self._lengths(ids=ids, is_new_out=is_new_out)
        self._check(self._lib.mld_tracks_begin_device(self._tr, self._opt(ids), self._i64(int(t.shape[0]) for t in ids),
                                                      self._opt(is_new_out)))
        self._hold(ids, is_new_out, call="begin")

    def commit(self, u_new, v_new, u_old, v_old, d_cur, d_last):
        """S float32 CUDA tensors each, indexed as the ids of begin(); d_cur / d_last: the depths of
        mld_tracklets_depths_device (d_last is read where the track is new)."""
        arrs = (u_new, v_new, u_old, v_old, d_cur, d_last)
        self._lengths(u_new=u_new, v_new=v_new, u_old=u_old, v_old=v_old, d_cur=d_cur, d_last=d_last)
        self._check(self._lib.mld_tracks_commit_device(self._tr, *[self._opt(a) for a in arrs]))
        self._hold(*arrs, call="commit")

    def export(self, fp_out, len_out):
        """fp_out: S float32 CUDA tensors [n_tracks, max_history, 3] ((u, v, d), newest first; rows beyond a track's
        length stay untouched), len_out: S int32 CUDA tensors [n_tracks]; the tracks of the last committed frame."""
        self._lengths(fp_out=fp_out, len_out=len_out)
        self._check(self._lib.mld_tracks_export_device(self._tr, self._opt(fp_out), self._opt(len_out)))
        self._hold(fp_out, len_out, call="export")

    def packed_capacity(self, n_tracks: int) -> int:
        """Entries an fp_out of export_packed() needs so that a sequence of n_tracks tracks is never truncated."""
        return int(n_tracks) * self.max_history

    def export_packed(self, fp_out, offsets_out):
        """The tracks of export() back to back (mld_tracks_export_packed_device).  offsets_out: S int64 CUDA tensors
        [n_tracks + 1] - track i of sequence s holds entries offsets[i] .. offsets[i + 1] - 1, offsets[n_tracks] is the
        sequence's total.  fp_out: None (offsets only), or S contiguous float32 CUDA tensors [capacity, 3] ((u, v, d),
        newest first within a track); entries at or beyond a tensor's capacity are dropped, which the caller sees from
        offsets[n_tracks] > capacity.  packed_capacity(n_tracks) never truncates."""
        self._lengths(fp_out=fp_out, offsets_out=offsets_out)
        cap = None
        if fp_out is not None:
            for t in fp_out:
                if not t.is_contiguous():
                    raise ValueError("fp_out: contiguous tensors")
            cap = [_entries(t, 3) for t in fp_out]
        self._check(self._lib.mld_tracks_export_packed_device(self._tr, self._opt(fp_out), self._i64(cap), self._opt(offsets_out)))
        self._hold(fp_out, offsets_out, call="export_packed")

    LEAVING_KEYS = ("ids", "offsets", "fp", "spill_ids", "spill_fp")

    def leaving_buffers(self, n_tracks, device=None) -> dict:
        """Output tensors of export_leaving() / set_leaving_sink() that never truncate sequences whose last committed
        frame holds n_tracks[s] tracks: {"ids", "offsets", "fp", "spill_ids", "spill_fp"} (lists of S) and "record"."""
        import torch
        dev = device if device is not None else torch.device("cuda", self._est._device)
        ns = [int(n) for n in n_tracks]
        self._lengths(n_tracks=ns)
        mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        return {"ids": [mk((n,), torch.int32) for n in ns], "offsets": [mk((n + 1,), torch.int64) for n in ns],
                "fp": [mk((n * self.max_history, 3), torch.float32) for n in ns],
                "spill_ids": [mk((n,), torch.int32) for n in ns], "spill_fp": [mk((n, 3), torch.float32) for n in ns],
                "record": mk((self.S, 4), torch.int64)}

    def _leaving_args(self, ids, offsets, fp, spill_ids, spill_fp, record):
        """(pointer tables, capacity tables and record pointer, what to keep alive) from lists of S tensors (an entry
        None: capacity 0).  The capacities are the tensors' sizes: ids [t], offsets [>= t + 1], fp [e, 3], spill_ids [p],
        spill_fp [>= p, 3]."""
        S = self.S
        lists = (ids, offsets, fp, spill_ids, spill_fp)
        self._lengths(**dict(zip(self.LEAVING_KEYS, lists)))
        for name, ts in zip(self.LEAVING_KEYS, lists):
            for t in ts:
                if t is not None and not t.is_contiguous():
                    raise ValueError(f"{name}: contiguous tensors")
        _holds(record, "*", 4 * S, 8, "record", required=True)
        tcap, ecap, scap = [], [], []
        for s in range(S):
            t = _entries(ids[s])
            if t and _entries(offsets[s]) < t + 1:
                raise ValueError(f"sequence {s}: offsets must hold one more entry than ids")
            p = _entries(spill_ids[s])
            if p and _entries(spill_fp[s], 3) < p:
                raise ValueError(f"sequence {s}: spill_fp must hold 3 floats per entry of spill_ids")
            tcap.append(t)
            ecap.append(_entries(fp[s], 3))
            scap.append(p)
        args = [self._ptrs(ts) for ts in lists] + [self._i64(tcap), self._i64(ecap), self._i64(scap),
                                                   C.c_void_p(int(record.data_ptr()))]
        return args, lists + (record,)

    def export_leaving(self, ids, offsets, fp, spill_ids, spill_fp, record, flush=None):
        """What the commit of the begun frame removes from the store (mld_tracks_export_leaving_device), between begin()
        and commit(): per sequence the tracks that end - ids [t] int32, offsets [t + 1] int64 and entries [e, 3] float32
        as export_packed() lays them out - and, for every continuing track with max_history entries, the id and the
        oldest entry that commit() overwrites (spill_ids [p], spill_fp [p, 3]).  Lists of S CUDA tensors (an entry None:
        capacity 0) whose sizes are the capacities; record: an int64 CUDA tensor [S, 4] that receives (n_ended,
        n_ended_entries, n_spilled, 0) complete, so that a count above a capacity tells a truncated sequence.
        leaving_buffers() makes a set that never truncates.  flush: None, or S flags - a flagged sequence gives all its
        tracks as ended and spills nothing; with every flag set no begun frame is needed."""
        args, keep = self._leaving_args(ids, offsets, fp, spill_ids, spill_fp, record)
        self._check(self._lib.mld_tracks_export_leaving_device(self._tr, self._select(flush), *args))
        self._hold(*keep, call="export_leaving")

    def set_leaving_sink(self, ids=None, offsets=None, fp=None, spill_ids=None, spill_fp=None, record=None):
        """The outputs of export_leaving() for the NEXT TrackletBatch.step() on this store
        (mld_tracks_set_leaving_sink): restarting lanes are flushed into them before they are emptied, the other lanes
        exported after the step's look-up.  One step consumes the sink.  Without arguments: the sink is taken away."""
        if all(a is None for a in (ids, offsets, fp, spill_ids, spill_fp, record)):
            self._check(self._lib.mld_tracks_set_leaving_sink(self._tr, *([None] * 9)))
            self._keep.pop("leaving_sink", None)
            return
        args, keep = self._leaving_args(ids, offsets, fp, spill_ids, spill_fp, record)
        self._check(self._lib.mld_tracks_set_leaving_sink(self._tr, *args))
        self._hold(*keep, call="leaving_sink")

    @classmethod
    def leaving_host(cls, buf) -> list:
        """The buffers of a finished export_leaving() on the host, per sequence {"ids", "offsets", "fp", "spill_ids",
        "spill_fp", "record"} trimmed to what was written - what TrackArchive.push() takes.  The caller has
        synchronised."""
        rec = buf["record"].cpu().numpy().reshape(-1, 4)
        out = []
        for s in range(rec.shape[0]):
            host = {k: (buf[k][s].cpu().numpy() if buf[k][s] is not None else None) for k in cls.LEAVING_KEYS}
            size = lambda k, per=1: host[k].size // per if host[k] is not None else 0  # noqa: E731
            t = min(int(rec[s, 0]), size("ids"))
            e = min(int(rec[s, 1]), size("fp", 3))
            p = min(int(rec[s, 2]), size("spill_ids"))
            out.append({"ids": host["ids"][:t] if t else np.zeros(0, np.int32),
                        "offsets": host["offsets"][:t + 1] if t else np.zeros(1, np.int64),
                        "fp": host["fp"].reshape(-1, 3)[:e] if e else np.zeros((0, 3), np.float32),
                        "spill_ids": host["spill_ids"][:p] if p else np.zeros(0, np.int32),
                        "spill_fp": host["spill_fp"].reshape(-1, 3)[:p] if p else np.zeros((0, 3), np.float32),
                        "record": rec[s].copy()})
        return out

    def _select(self, select):
        """The table of S flags (None: NULL, which selects all)."""
        self._lengths(select=select)
        return (C.c_uint8 * self.S)(*[1 if x else 0 for x in select]) if select is not None else None

    def import_packed(self, ids, offsets, fp, select=None):
        """The inverse of export_packed() (mld_tracks_import_packed_device): the committed frame of every selected
        sequence is replaced by the given tracks, as if a fresh store had been brought to that state.  ids: S int32 CUDA
        tensors [n]; offsets: S int64 CUDA tensors [n + 1]; fp: S contiguous float32 CUDA tensors [entries, 3] - what
        export_packed() of a store (of any max_tracks / max_history, on any context) wrote, with the ids of that frame.
        select: None (all), or S flags; the entries of a sequence that is not selected may be None and the sequence is
        not touched.  A selected sequence whose ids is None or empty is emptied.  Histories longer than max_history keep
        their newest entries; offsets are clamped to the entries fp holds.  A begun frame is abandoned."""
        self._lengths(ids=ids, offsets=offsets, fp=fp, select=select)
        nt, ne = [], []
        for s in range(self.S):
            on = select is None or bool(select[s])
            n = int(ids[s].shape[0]) if on and ids[s] is not None else 0
            if n:
                _holds(offsets[s], s, n + 1, 8, "offsets", required=True)
                if int(offsets[s].numel()) != n + 1:
                    raise ValueError(f"sequence {s}: offsets must hold {n + 1} entries")
                _holds(fp[s], s, 0, 4, "fp")
            nt.append(n)
            ne.append(_entries(fp[s], 3) if n else 0)
        ids, offsets, fp = ([t if nt[s] else None for s, t in enumerate(ts)] for ts in (ids, offsets, fp))
        self._check(self._lib.mld_tracks_import_packed_device(self._tr, self._select(select), self._ptrs(ids), self._i64(nt),
                                                              self._ptrs(offsets), self._ptrs(fp), self._i64(ne)))
        self._hold(ids, offsets, fp, call="import_packed")

    def reset(self, select=None):
        """Empties the selected sequences (None: all) - import_packed() of no tracks (mld_tracks_reset_device)."""
        self._check(self._lib.mld_tracks_reset_device(self._tr, self._select(select)))

    def counts(self) -> np.ndarray:
        """[S, 6] int64 of the last committed frame, columns COUNT_NAMES.  Synchronises."""
        out = np.zeros((self.S, 6), dtype=np.int64)
        self._check(self._lib.mld_tracks_counts(self._tr, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out


class SemanticLabels(_BatchObject):
    """assignLabels (matches_conversion_ros_tool/src/semantic_labels/semantic_labels.cpp:50-72) for S sequences per call
    (mld_labels_*, include/mld.h - the window arithmetic and the three defined cases are stated there).  Lists of S
    torch CUDA tensors in and out; asynchronous on the estimator's stream.  Close it before its estimator."""

    NO_LABEL = -2
    _NAME, _HANDLE = "labels", "_lb"

    def __init__(self, estimator: DepthEstimator, n_seq: int):
        self.S = int(n_seq)
        self._create(estimator, self.S)

    def assign(self, images, roi, u, v, label_out, votes_out=None):
        """images: S uint8 CUDA tensors [rows, cols] of one shape and row stride (unit column stride); roi: (width,
        height); u, v: S float32 CUDA tensors, the newest feature of every track; label_out: S int16 CUDA tensors of
        the same lengths; votes_out: None, or S int32 CUDA tensors [n, 2] (single entries may be None) that receive
        (count of the winning label, pixels in the clipped window)."""
        self._lengths(images=images, u=u, v=v, label_out=label_out, votes_out=votes_out)
        rows, cols, stride = self._image_geometry(images)
        for s in range(self.S):
            n = int(u[s].shape[0])
            if int(v[s].shape[0]) != n or int(label_out[s].shape[0]) != n:
                raise ValueError(f"sequence {s}: u, v and label_out differ in length")
            if _at(votes_out, s) is not None and tuple(votes_out[s].shape) != (n, 2):
                raise ValueError(f"sequence {s}: votes_out must be [{n}, 2]")
        vp = self._ptrs
        self._check(self._lib.mld_labels_assign_device(
            self._lb, vp(images), rows, cols, max(stride, cols), int(roi[0]), int(roi[1]), vp(u), vp(v),
            self._i64(int(t.shape[0]) for t in u), vp(label_out), self._opt(votes_out)))
        self._hold(images, u, v, label_out, votes_out)


class SemanticPlanes(_BatchObject):
    """SemanticPlane::CalculateInliersPlane (RansacPlane.cpp:195-274) for S sequences per call (mld_semantic_planes_*,
    include/mld.h): per sequence the plane of the refit, the candidate and inlier counts, a status (1 = the reference's
    ExceptionPclInvalid) and the inlier bitmask - bit for bit what DepthEstimator.estimateSemanticPlane gives for that
    cloud, without a frame slot and before the projection.  Lists of S torch CUDA tensors in and out; asynchronous on
    the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "semantic_planes", "_sp"
    mask_words = staticmethod(mask_words)

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_points: int):
        self.S, self.max_points = int(n_seq), int(max_points)
        self._create(estimator, self.S, self.max_points, *self._calibration(estimator, "camera", "transform"))

    def estimate(self, clouds, images, labels, inlier_threshold: float, result_out, masks_out):
        """clouds: S contiguous float32 CUDA tensors [n, 4] or [n, 8] of one width; images: S uint8 CUDA tensors
        [rows, cols] of one shape and row stride (unit column stride); labels: the ground labels; result_out: an int32
        CUDA tensor [S, 8] that receives the records (capi.MldSemanticPlaneResult: coefficients as float bits, then
        n_candidates, n_inliers, status, 0); masks_out: S int32 CUDA tensors of at least mask_words(n) entries."""
        self._lengths(clouds=clouds, images=images, masks_out=masks_out)
        width, ns = _cloud_table(clouds, none_allowed=False)
        for s, n in enumerate(ns):
            _mask_room(masks_out[s], s, n, "masks_out")
        rows, cols, stride = self._image_geometry(images)
        _result_tensor(result_out, (self.S, 8), 4, "result_out")
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        vp = self._ptrs
        self._check(self._lib.mld_semantic_planes_estimate_device(
            self._sp, vp(clouds), self._i64(ns), 4 * width, vp(images), rows, cols, max(stride, cols), lab.ctypes.data,
            int(lab.size), float(inlier_threshold), int(result_out.data_ptr()), vp(masks_out)))
        self._hold(clouds, images, result_out, masks_out)


class RansacPlanes(_BatchObject):
    """RansacPlane::CalculateInliersPlane (RansacPlane.cpp:41-140) for S sequences per call (mld_ransac_planes_*,
    include/mld.h): per sequence the plane, the inlier count, PCL's iteration count, a status (1 = the reference's
    ExceptionPclInvalid), the number of pass-through candidates and the inlier bitmask - bit for bit what
    DepthEstimator.estimateGroundPlane gives for that cloud and seed, without a frame slot and before the projection.
    `parameters` (default: the estimator's) is copied at creation.  Lists of S torch CUDA tensors in and out;
    asynchronous on the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "ransac_planes", "_rp"
    mask_words = staticmethod(mask_words)

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_points: int, parameters=None):
        self.S, self.max_points = int(n_seq), int(max_points)
        self._create(estimator, self.S, self.max_points, *self._calibration(estimator, "parameters", parameters=parameters))

    def estimate(self, clouds, seeds, result_out, masks_out):
        """clouds: S contiguous float32 CUDA tensors [n, 4] or [n, 8] of one width (an entry None: a sequence without
        points); seeds: S integers; result_out: an int32 CUDA tensor [S, 8] that receives the records
        (capi.MldRansacPlaneResult: coefficients as float bits, then n_inliers, iterations, status, n_candidates);
        masks_out: S int32 CUDA tensors of at least mask_words(n) entries (None where the cloud is)."""
        self._lengths(clouds=clouds, seeds=seeds, masks_out=masks_out)
        width, ns = _cloud_table(clouds)
        for s, n in enumerate(ns):
            if n:
                _mask_room(masks_out[s], s, n, "masks_out")
        _result_tensor(result_out, (self.S, 8), 4, "result_out")
        vp = self._ptrs
        self._check(self._lib.mld_ransac_planes_estimate_device(
            self._rp, vp(clouds), self._i64(ns), 4 * width, (C.c_uint32 * self.S)(*[int(x) & 0xFFFFFFFF for x in seeds]),
            int(result_out.data_ptr()), vp(masks_out)))
        self._hold(clouds, result_out, masks_out)


class ProjectedClouds(_BatchObject):
    """The frame's PointcloudData (DepthEstimator.cpp:155-218, NeighborFinderPixel.cpp:38-55) for S sequences per call
    (mld_projected_clouds_*, include/mld.h): per sequence the visible list (getPointsCloudImageCs), _pointIndex,
    getPointDepthCamVisible, the camera-frame cloud (getCloudCameraCs) and the reference-format pixel map - bit for bit
    what the one-slot getters (getPointsCloudImageCs ... getPixelMap) give for that cloud, without a frame slot and into
    device tensors.  Lists of S torch CUDA tensors in and out; asynchronous on the estimator's stream.  Close it before its
    estimator."""

    _NAME, _HANDLE = "projected_clouds", "_pc"

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_points: int):
        self.S, self.max_points = int(n_seq), int(max_points)
        self._create(estimator, self.S, self.max_points, *self._calibration(estimator, "camera", "transform"))

    def export(self, clouds, capacity, n_visible, uv, index, depth=None, cam=None, pixel_map=None):
        """clouds: S contiguous float32 CUDA tensors [n, 4] or [n, 8] of one width (an entry None: a sequence without
        points); capacity: S integers, or None (= n, never truncated); n_visible: an int64 CUDA tensor [S]; uv: S float64
        CUDA tensors of at least 2 * min(capacity, n) entries ((u, v) of visible point r at [2 r], [2 r + 1]: a
        contiguous [capacity, 2]); index: S int32 CUDA tensors of at least min(capacity, n) entries; depth: None, or S
        float64 CUDA tensors of that length; cam: None, or S float64 CUDA tensors of 3 * n entries (a contiguous [n, 3]);
        pixel_map: None, or S int32 CUDA tensors of height * width entries.  Single entries of uv and index may be None
        where min(capacity, n) is 0, of depth, cam and pixel_map anywhere.  Visible points at or beyond a sequence's
        capacity are dropped, which the caller sees from n_visible[s] > capacity[s]; the map is not affected."""
        self._lengths(clouds=clouds, capacity=capacity, uv=uv, index=index, depth=depth, cam=cam, pixel_map=pixel_map)
        _result_tensor(n_visible, (self.S,), 8, "n_visible")
        width, ns = _cloud_table(clouds)
        caps = _capacities(capacity, ns)
        for s, n in enumerate(ns):
            m = min(caps[s], n)
            _holds(_at(uv, s), s, 2 * m, 8, "uv", required=True)
            _holds(_at(index, s), s, m, 4, "index", required=True)
            _holds(_at(depth, s), s, m, 8, "depth")
            _holds(_at(cam, s), s, 3 * n, 8, "cam")
            _holds(_at(pixel_map, s), s, self.width * self.height, 4, "pixel_map")
        vp, opt = self._ptrs, self._opt
        self._check(self._lib.mld_projected_clouds_export_device(
            self._pc, vp(clouds), self._i64(ns), 4 * width, self._i64(caps), int(n_visible.data_ptr()), vp(uv), vp(index),
            opt(depth), opt(cam), opt(pixel_map)))
        self._hold(clouds, n_visible, uv, index, depth, cam, pixel_map)


class DepthReports(_BatchObject):
    """The depth-calculation statistics (getDepthCalcStats, DepthEstimator.cpp:1039-1090) and the interpolated cloud
    (getCloudInterpolated: the point (u - cu) / f * d, (v - cv) / f * d, d of every feature with depth >= 0, in feature
    order) for S sequences per call (mld_depth_reports_*, include/mld.h), from device tensors into device tensors.
    collect() takes the arrays of the DepthEstimator layer (float64 uv, float64 depths), collect_tracks() those of the
    tracklet layer (float32 u, v, depths of the CURRENT frame; u and v are truncated to the integer pixel).  Lists of S
    torch CUDA tensors in and out; asynchronous on the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "depth_reports", "_dr"
    WORDS = 24  # int64 words of a record (capi.MldDepthReport): counts[21], other, point_count, n_interpolated

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_features: int):
        self.S, self.max_features = int(n_seq), int(max_features)
        self._create(estimator, self.S, self.max_features, *self._calibration(estimator, "camera"))

    def _collect(self, fn, size, per, depth, types, report, capacity, points, feature, **coords):
        """Both calls: `coords` are the feature tables in front of depth, of `per` x n entries of `size` bytes each."""
        self._lengths(depth=depth, **coords)
        ns = []
        for s, d in enumerate(depth):
            n = _entries(d)
            _holds(d, s, n, size, "depth")
            for name, ts in coords.items():
                _holds(ts[s], s, per * n, size, name, required=True)
                if ts[s] is not None and int(ts[s].numel()) != per * n:
                    raise ValueError(f"sequence {s}: {name} must hold {per} x {n} entries, as depth does")
            ns.append(n)
        self._lengths(types=types, capacity=capacity, points=points, feature=feature)
        _result_tensor(report, (self.S, self.WORDS), 8, "report")
        for s, n in enumerate(ns):
            _holds(_at(types, s), s, n, 4, "types")
            if _at(types, s) is not None and int(types[s].numel()) != n:
                raise ValueError(f"sequence {s}: types must hold {n} entries")
        caps = None
        if points is not None:  # (without points neither the capacities nor the feature table are looked at or passed)
            caps = _capacities(capacity, ns)
            for s, n in enumerate(ns):
                m = min(caps[s], n)
                _holds(points[s], s, 3 * m, 8, "points", required=True)
                _holds(_at(feature, s), s, m, 4, "feature")
        tables = tuple(coords.values()) + (depth,)
        opt = self._opt
        self._check(fn(self._dr, *[self._ptrs(ts) for ts in tables], opt(types), self._i64(ns), self._i64(caps),
                       int(report.data_ptr()), opt(points), opt(feature) if points is not None else None))
        self._hold(*tables, types, report, points, feature)

    def collect(self, uv, depth, types, report, capacity=None, points=None, feature=None):
        """uv: S contiguous float64 CUDA tensors [n, 2] (an entry None: a sequence without features); depth: S float64
        CUDA tensors [n]; types: None, or S int32 CUDA tensors [n] (single entries may be None): without them counts
        and other are 0; report: an int64 CUDA tensor [S, 24] that receives the records (capi.MldDepthReport); points:
        None (statistics only), or S float64 CUDA tensors of at least 3 * min(capacity, n) entries (a contiguous
        [capacity, 3]); capacity: S integers, or None (= n, never truncated); feature: None, or S int32 CUDA tensors of
        at least min(capacity, n) entries (single entries may be None).  Points at or beyond a sequence's capacity are
        dropped, which the caller sees from n_interpolated > capacity."""
        self._collect(self._lib.mld_depth_reports_collect_device, 8, 2, depth, types, report, capacity, points, feature, uv=uv)

    def collect_tracks(self, u, v, depth, types, report, capacity=None, points=None, feature=None):
        """As collect(), on the tensors of TrackletBatch.prepare_step() / prepare(): u, v (u_new, v_new), depth (d_cur):
        S float32 CUDA tensors [n]; types (t_cur): None, or S int32 CUDA tensors [n]."""
        self._collect(self._lib.mld_depth_reports_collect_tracks_device, 4, 1, depth, types, report, capacity, points, feature,
                      u=u, v=v)


class PlaneInliers(_BatchObject):
    """What the reference keeps on a frame's ground plane besides the coefficients, for S sequences per call
    (mld_plane_inliers_*, include/mld.h), from the inlier bitmasks SemanticPlanes / RansacPlanes write: per sequence the
    ascending inlier indices (GroundPlane::getInlinersIndex), the lidar-frame float matrix of the inliers
    (getMatrixFromIndices) and the camera-frame inlier cloud filtered by ransac_plane_use_camx_treshold /
    ransac_plane_treshold_camx (getCloudRansacPlane) - bit for bit what getGroundPlaneInliers / getCloudRansacPlane give
    on a slot that holds that cloud and mask, without a frame slot and into device tensors.  `parameters` (default: the
    estimator's) is copied at creation.  Lists of S torch CUDA tensors in and out; asynchronous on the estimator's
    stream.  Close it before its estimator."""

    _NAME, _HANDLE = "plane_inliers", "_pi"
    mask_words = staticmethod(mask_words)

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_points: int, parameters=None):
        self.S, self.max_points = int(n_seq), int(max_points)
        self._create(estimator, self.S, self.max_points,
                     *self._calibration(estimator, "parameters", "transform", parameters=parameters))

    def export(self, clouds, masks, capacity, counts, index, lidar=None, cam=None):
        """clouds: S contiguous float32 CUDA tensors [n, 4] or [n, 8] of one width (an entry None: a sequence without
        points); masks: S int32 CUDA tensors of at least mask_words(n) entries (None where the cloud is); capacity: S
        integers, or None (= n, never truncated); counts: an int64 CUDA tensor [S, 2] that receives (n_inliers, n_cloud);
        index: S int32 CUDA tensors of at least min(capacity, n) entries; lidar: None, or S float32 CUDA tensors of 3 *
        min(capacity, n) entries (a contiguous [capacity, 3]); cam: None, or S float64 CUDA tensors of that length.
        Single entries of index may be None where min(capacity, n) is 0, of lidar and cam anywhere.  Inliers (cloud
        points) at or beyond a sequence's capacity are dropped, which the caller sees from the counts."""
        self._lengths(clouds=clouds, masks=masks, capacity=capacity, index=index, lidar=lidar, cam=cam)
        _result_tensor(counts, (self.S, 2), 8, "counts")
        width, ns = _cloud_table(clouds)
        caps = _capacities(capacity, ns)
        for s, n in enumerate(ns):
            m = min(caps[s], n)
            _holds(_at(masks, s), s, mask_words(n), 4, "masks", required=True)
            _holds(_at(index, s), s, m, 4, "index", required=True)
            _holds(_at(lidar, s), s, 3 * m, 4, "lidar")
            _holds(_at(cam, s), s, 3 * m, 8, "cam")
        vp, opt = self._ptrs, self._opt
        self._check(self._lib.mld_plane_inliers_export_device(
            self._pi, vp(clouds), self._i64(ns), 4 * width, vp(masks), self._i64(caps), int(counts.data_ptr()), vp(index),
            opt(lidar), opt(cam)))
        self._hold(clouds, masks, counts, index, lidar, cam)


class _FeatureUnit(_BatchObject):
    """What FeatureTraces, NearestDepths and RowGrowth share - one record per feature, on the tensors ProjectedClouds.export wrote:
    the feature tables of both forms with their refusals, what the exported cloud of a sequence with features must hold,
    the leading arguments of the C calls, and records().  WORDS: int64 words of a record, DTYPE: its fields."""

    @classmethod
    def records(cls, record) -> np.ndarray:
        """A record tensor (int64 [n, WORDS]) as a NumPy record array with the fields of DTYPE (copies to the host,
        which synchronises as usual)."""
        return np.ascontiguousarray(record.cpu().numpy()).reshape(-1).view(cls.DTYPE)

    def _uv_counts(self, uv):
        """The features of every sequence from the float64 table uv."""
        self._lengths(uv=uv)
        for s, t in enumerate(uv):
            _holds(t, s, 0, 8, "uv")
            if _entries(t) % 2:
                raise ValueError(f"sequence {s}: uv must be a contiguous float64 tensor [n, 2]")
        return [_entries(t, 2) for t in uv]

    def _track_counts(self, u, v):
        """The features of every sequence from the float32 tables u, v of the tracklet layer."""
        self._lengths(u=u, v=v)
        for s, (a, b) in enumerate(zip(u, v)):
            if (a is None) != (b is None):
                raise ValueError(f"sequence {s}: u and v come together")
            _holds(a, s, 0, 4, "u")
            _holds(b, s, 0, 4, "v")
            if _entries(b) != _entries(a):
                raise ValueError(f"sequence {s}: u and v must be contiguous float32 tensors of one length")
        return [_entries(a) for a in u]

    def _cloud_holds(self, ns, maps, index, cam, name, record, cap, lists):
        """The exported cloud of a sequence with features holds what it must, its record tensor `name` and, with a
        capacity, its rows of `lists` (name: table) as well."""
        for s, n in enumerate(ns):
            if n == 0:  # (nothing of a sequence without features is looked at)
                continue
            _holds(maps[s], s, self.width * self.height, 4, "pixel_map", required=True)
            _holds(index[s], s, 0, 4, "index")
            _holds(cam[s], s, 0, 8, "cam")
            _holds(record[s], s, self.WORDS * n, 8, name, required=True)
            for row, ts in lists.items():
                if cap:
                    _holds(_at(ts, s), s, cap * n, 4, row)

    def _cloud_args(self, ns, feats, maps, index, cam):
        """What both C calls of both units begin with behind the object: the feature tables, the counts, the cloud."""
        vp = self._ptrs
        return (*[vp(t) for t in feats], self._i64(ns), vp(maps), vp(index), self._i64(_entries(t) for t in index), vp(cam),
                self._i64(_entries(t, 3) for t in cam))


class FeatureTraces(_FeatureUnit):
    """Why a feature got the depth it got, for S sequences per call (mld_feature_traces_*, include/mld.h): per feature
    the record the reference calls DepthCalcStatsSinglePoint - neighbour and segmented counts, histogram borders, corner
    positions, the plane - with the triangle corners of getCloudTriangleCorners and the state the road fallback ended in,
    and, where asked for, the index lists behind the counts.  It runs on the tensors ProjectedClouds.export wrote
    (pixel_map, index, cam) and on the planes as prepare() / prepare_step() take them.  collect() takes float64 uv,
    collect_tracks() the float32 u, v of the tracklet layer (truncated to the integer pixel).  `parameters` (default: the
    estimator's) is copied at creation; do_use_PCA is refused.  Lists of S torch CUDA tensors in and out; asynchronous on
    the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "feature_traces", "_ft"
    WORDS = 23  # int64 words of a record (capi.MldFeatureTrace, 184 bytes)
    DTYPE = np.dtype(capi.MldFeatureTrace)
    MAX_LIST = 1024

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_features: int, parameters=None):
        self.S, self.max_features = int(n_seq), int(max_features)
        self._create(estimator, self.S, self.max_features,
                     *self._calibration(estimator, "parameters", "camera", "transform", parameters=parameters))

    def _collect(self, ns, feats, maps, index, cam, trace, coeffs, masks, list_capacity, lists):
        cap = int(list_capacity)
        lists = dict(zip(("nb", "seg", "road", "road_inl"), lists))
        self._lengths(pixel_map=maps, index=index, cam=cam, trace=trace, masks=masks, **lists)
        if not 0 <= cap <= self.MAX_LIST:
            raise ValueError(f"list_capacity must be in 0 .. {self.MAX_LIST}")
        planes = self._plane_args(coeffs, masks)
        self._cloud_holds(ns, maps, index, cam, "trace", trace, cap, lists)
        fn = self._lib.mld_feature_traces_collect_device if len(feats) == 1 else self._lib.mld_feature_traces_collect_tracks_device
        self._check(fn(self._ft, *self._cloud_args(ns, feats, maps, index, cam), *planes, cap, self._ptrs(trace),
                       *[self._opt(ts) for ts in lists.values()]))
        self._hold(*feats, maps, index, cam, trace, masks, *lists.values())

    def collect(self, uv, pixel_map, index, cam, trace, coeffs=None, masks=None, list_capacity: int = 0, nb=None, seg=None,
                road=None, road_inl=None):
        """uv: S contiguous float64 CUDA tensors [n, 2] (an entry None: a sequence without features); pixel_map, index,
        cam: the S tensors each that ProjectedClouds.export wrote for the clouds (int32 [height, width], int32 of a
        capacity that did not truncate, float64 [points, 3]); trace: S int64 CUDA tensors of at least 23 * n entries (a
        contiguous [n, 23]: capi.MldFeatureTrace, see records()); coeffs (float32 [S, 4], host) and masks (S int32 CUDA
        tensors, an entry None: that sequence has no plane): both or neither; nb, seg, road, road_inl: None, or S int32
        CUDA tensors of at least list_capacity * n entries (a contiguous [n, list_capacity]; single entries may be None).
        A row receives the first min(count, list_capacity) entries of its list; the counts of the record are complete."""
        self._collect(self._uv_counts(uv), (uv,), pixel_map, index, cam, trace, coeffs, masks, list_capacity,
                      (nb, seg, road, road_inl))

    def collect_tracks(self, u, v, pixel_map, index, cam, trace, coeffs=None, masks=None, list_capacity: int = 0, nb=None,
                       seg=None, road=None, road_inl=None):
        """As collect(), on the tensors of TrackletBatch.prepare_step() / prepare(): u, v (u_new, v_new): S float32 CUDA
        tensors [n]."""
        self._collect(self._track_counts(u, v), (u, v), pixel_map, index, cam, trace, coeffs, masks, list_capacity,
                      (nb, seg, road, road_inl))


class CoverageMaps(_BatchObject):
    """Where in the image a feature can get a depth, for S sequences per call (mld_coverage_maps_*, include/mld.h): at
    every integer pixel the neighbour counts of the narrow and the wide window (occupied, plane inliers, far points),
    the two reach bits - the feature is not type 2; the road estimator can run -, per sequence a record of totals, and
    per bucket of the image the pixel with the most neighbours.  It runs on the tensors ProjectedClouds.export wrote
    (pixel_map, index, cam) and on the planes as prepare() / prepare_step() take them.  `parameters` (default: the
    estimator's) is copied at creation.  Lists of S torch CUDA tensors in and out; asynchronous on the estimator's
    stream.  Close it before its estimator."""

    _NAME, _HANDLE = "coverage_maps", "_cm"
    WORDS = 8  # int64 words of a record (capi.MldCoverageRecord, 64 bytes)
    DTYPE = np.dtype(capi.MldCoverageRecord)
    MAPS = ("nb", "road", "road_inl", "road_far", "reach")

    def __init__(self, estimator: DepthEstimator, n_seq: int, parameters=None):
        self.S = int(n_seq)
        self._create(estimator, self.S, *self._calibration(estimator, "parameters", "camera", "transform", parameters=parameters))

    @classmethod
    def records(cls, record) -> np.ndarray:
        """A record tensor (int64 [S, 8]) as a NumPy record array with the fields of capi.MldCoverageRecord (copies to
        the host, which synchronises as usual)."""
        return np.ascontiguousarray(record.cpu().numpy()).reshape(-1).view(cls.DTYPE)

    def buckets(self, bucket_w: int, bucket_h: int) -> int:
        """Buckets of the image for buckets of this size: ceil(width / bucket_w) * ceil(height / bucket_h)."""
        return -(-self.width // int(bucket_w)) * -(-self.height // int(bucket_h))

    def collect(self, pixel_map, index, cam, record, coeffs=None, masks=None, nb=None, road=None, road_inl=None, road_far=None,
                reach=None, bucket=None, bucket_out=None):
        """pixel_map, index, cam: the S tensors each that ProjectedClouds.export wrote for the clouds (int32 [height,
        width], int32 of a capacity that did not truncate, float64 [points, 3]; index and cam entries may be None for an
        empty cloud); record: an int64 CUDA tensor of at least 8 * S entries (a contiguous [S, 8]:
        capi.MldCoverageRecord, see records()); coeffs (float32 [S, 4], host) and masks (S int32 CUDA tensors, an entry
        None: that sequence has no plane): both or neither; nb, road, road_inl, road_far, reach: None, or S uint8 CUDA
        tensors of at least width * height entries (a contiguous [height, width]; single entries may be None); bucket:
        None or (bucket_w, bucket_h) with bucket_out: S int32 CUDA tensors (a contiguous [capacity, 3] each, rows (x, y,
        n_nb); an entry None: capacity 0).  A sequence's first min(buckets, capacity) rows are written; n_buckets of the
        record is complete."""
        cells = self.width * self.height
        maps = (nb, road, road_inl, road_far, reach)
        self._lengths(pixel_map=pixel_map, index=index, cam=cam, masks=masks, bucket_out=bucket_out, **dict(zip(self.MAPS, maps)))
        planes = self._plane_args(coeffs, masks)
        if (bucket is None) != (bucket_out is None):
            raise ValueError("bucket and bucket_out come together or not at all")
        _holds(record, "*", self.WORDS * self.S, 8, "record", required=True)
        for s in range(self.S):
            _holds(pixel_map[s], s, cells, 4, "pixel_map", required=True)
            _holds(index[s], s, 0, 4, "index")
            _holds(cam[s], s, 0, 8, "cam")
            for name, ts in zip(self.MAPS, maps):
                _holds(_at(ts, s), s, cells, 1, name)
            _holds(_at(bucket_out, s), s, 0, 4, "bucket_out")
        bw, bh = (int(bucket[0]), int(bucket[1])) if bucket is not None else (0, 0)
        caps = [_entries(t, 3) for t in bucket_out] if bucket_out is not None else None
        vp, opt = self._ptrs, self._opt
        self._check(self._lib.mld_coverage_maps_collect_device(
            self._cm, vp(pixel_map), vp(index), self._i64(_entries(t) for t in index), vp(cam),
            self._i64(_entries(t, 3) for t in cam), *planes, *[opt(ts) for ts in maps], int(record.data_ptr()), bw, bh,
            self._i64(caps), opt(bucket_out)))
        self._hold(pixel_map, index, cam, record, masks, *maps, bucket_out)


class DepthImages(_BatchObject):
    """Dense depth images for S sequences per call (mld_depth_images_*, include/mld.h): the depth path - narrow window,
    histogram, triangle, thresholds, road fallback with its fit - at every pixel of a grid over the camera image: the
    result type, the depth as float32 and optionally as float64, and per sequence a record of counts.  It runs on the
    tensors ProjectedClouds.export wrote (pixel_map, index, cam) and on the planes as prepare() / prepare_step() take
    them; it needs no frame slot and no feature array.  `parameters` (default: the estimator's) is copied at creation.
    Lists of S torch CUDA tensors in and out; asynchronous on the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "depth_images", "_di"
    WORDS = 25  # int64 words of a record (capi.MldDepthImageRecord, 200 bytes)
    DTYPE = np.dtype(capi.MldDepthImageRecord)

    def __init__(self, estimator: DepthEstimator, n_seq: int, parameters=None):
        self.S = int(n_seq)
        self._create(estimator, self.S, *self._calibration(estimator, "parameters", "camera", "transform", parameters=parameters))

    @classmethod
    def records(cls, record) -> np.ndarray:
        """A record tensor (int64 [S, 25]) as a NumPy record array with the fields of capi.MldDepthImageRecord (copies
        to the host, which synchronises as usual)."""
        return np.ascontiguousarray(record.cpu().numpy()).reshape(-1).view(cls.DTYPE)

    def grid(self, grid=None):
        """(x0, y0, step_x, step_y, grid_w, grid_h) of `grid`: None (every pixel), (x0, y0, step_x, step_y) - as many
        grid pixels as fit into the image from (x0, y0) on - or all six."""
        if grid is None:
            return 0, 0, 1, 1, self.width, self.height
        g = [int(v) for v in grid]
        if len(g) == 4:
            x0, y0, sx, sy = g
            if sx < 1 or sy < 1 or not (0 <= x0 < self.width and 0 <= y0 < self.height):
                raise ValueError("grid: (x0, y0) inside the image and steps >= 1")
            return x0, y0, sx, sy, (self.width - 1 - x0) // sx + 1, (self.height - 1 - y0) // sy + 1
        if len(g) != 6:
            raise ValueError("grid: None, (x0, y0, step_x, step_y) or (x0, y0, step_x, step_y, grid_w, grid_h)")
        return tuple(g)

    def render(self, pixel_map, index, cam, record, coeffs=None, masks=None, grid=None, depth=None, depth32=None, type=None):
        """pixel_map, index, cam: the S tensors each that ProjectedClouds.export wrote for the clouds (int32 [height,
        width], int32 of a capacity that did not truncate, float64 [points, 3]; index and cam entries may be None for an
        empty cloud); record: an int64 CUDA tensor of at least 25 * S entries (a contiguous [S, 25]:
        capi.MldDepthImageRecord, see records()); coeffs (float32 [S, 4], host) and masks (S int32 CUDA tensors, an entry
        None: that sequence has no plane): both or neither; grid: see grid(); depth (float64), depth32 (float32), type
        (uint8): None, or S CUDA tensors of at least grid_w * grid_h entries (a contiguous [grid_h, grid_w]; single
        entries may be None)."""
        cells = self.width * self.height
        x0, y0, sx, sy, gw, gh = self.grid(grid)
        n = max(gw, 0) * max(gh, 0)
        self._lengths(pixel_map=pixel_map, index=index, cam=cam, masks=masks, depth=depth, depth32=depth32, type=type)
        planes = self._plane_args(coeffs, masks)
        _holds(record, "*", self.WORDS * self.S, 8, "record", required=True)
        for s in range(self.S):
            _holds(pixel_map[s], s, cells, 4, "pixel_map", required=True)
            _holds(index[s], s, 0, 4, "index")
            _holds(cam[s], s, 0, 8, "cam")
            _holds(_at(depth, s), s, n, 8, "depth")
            _holds(_at(depth32, s), s, n, 4, "depth32")
            _holds(_at(type, s), s, n, 1, "type")
        vp, opt = self._ptrs, self._opt
        self._check(self._lib.mld_depth_images_render_device(
            self._di, vp(pixel_map), vp(index), self._i64(_entries(t) for t in index), vp(cam),
            self._i64(_entries(t, 3) for t in cam), *planes, x0, y0, sx, sy, gw, gh, opt(depth), opt(depth32), opt(type),
            int(record.data_ptr())))
        self._hold(pixel_map, index, cam, record, masks, depth, depth32, type)


class RegionDepths(_BatchObject):
    """The foreground depth of image rectangles for S sequences per call (mld_region_depths_*, include/mld.h): per box
    - a detector's 2-D box, a label blob's bounding box, inclusive corners, any size - the number of points, the
    smallest, the largest and the exact median camera z, the nearest point, and the bin of the reference's
    first-local-maximum histogram (FilterPointsMinDistBlob) with the points inside it; optionally without the points of
    a ground plane.  It runs on the tensors ProjectedClouds.export wrote (pixel_map, index, cam) and on the masks as
    SemanticPlanes / RansacPlanes write them.  Of the estimator's parameters the histogram's bin width and minimal count
    are copied at creation.  Lists of S torch CUDA tensors in and out; asynchronous on the estimator's stream.  Close it
    before its estimator."""

    _NAME, _HANDLE = "region_depths", "_rd"
    WORDS = 10  # int64 words of a record (capi.MldRegionDepth, 80 bytes)
    DTYPE = np.dtype(capi.MldRegionDepth)
    LIST_CAPACITY, HIST_BINS = capi.MLD_REGION_LIST_CAPACITY, capi.MLD_REGION_HIST_BINS

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_boxes: int, parameters=None):
        self.S, self.max_boxes = int(n_seq), int(max_boxes)
        self._create(estimator, self.S, self.max_boxes, *self._calibration(estimator, "parameters", "camera", parameters=parameters))

    @classmethod
    def records(cls, record) -> np.ndarray:
        """A record tensor (int64 [n, 10]) as a NumPy record array with the fields of capi.MldRegionDepth (copies to
        the host, which synchronises as usual)."""
        return np.ascontiguousarray(record.cpu().numpy()).reshape(-1).view(cls.DTYPE)

    def collect(self, pixel_map, index, cam, boxes, record, masks=None):
        """pixel_map, index, cam: the S tensors each that ProjectedClouds.export wrote for the clouds (int32 [height,
        width], int32 of a capacity that did not truncate, float64 [points, 3]; index and cam entries may be None for an
        empty cloud); boxes: S int32 CUDA tensors (a contiguous [n, 4] each, rows (x0, y0, x1, y1), inclusive; an entry
        None: no box); record: S int64 CUDA tensors of at least 10 * n entries (a contiguous [n, 10]:
        capi.MldRegionDepth, see records(); None where boxes is); masks: None, or S int32 CUDA tensors (an entry None:
        that sequence excludes nothing)."""
        cells = self.width * self.height
        self._lengths(pixel_map=pixel_map, index=index, cam=cam, boxes=boxes, record=record, masks=masks)
        ns = [_entries(b, 4) for b in boxes]
        for s in range(self.S):
            if ns[s] > self.max_boxes:
                raise ValueError(f"sequence {s}: {ns[s]} boxes, the object was made for {self.max_boxes}")
            _holds(pixel_map[s], s, cells, 4, "pixel_map", required=True)
            _holds(index[s], s, 0, 4, "index")
            _holds(cam[s], s, 0, 8, "cam")
            _holds(boxes[s], s, 0, 4, "boxes")
            _holds(record[s], s, self.WORDS * ns[s], 8, "record", required=True)
            if _at(masks, s) is not None:
                _mask_room(masks[s], s, _entries(cam[s], 3), "masks")
        vp = self._ptrs
        self._check(self._lib.mld_region_depths_collect_device(
            self._rd, vp(pixel_map), vp(index), self._i64(_entries(t) for t in index), vp(cam),
            self._i64(_entries(t, 3) for t in cam), self._opt(masks), vp(boxes), self._i64(ns), vp(record)))
        self._hold(pixel_map, index, cam, boxes, record, masks)


class NearestDepths(_FeatureUnit):
    """The main path on the `count` closest returns of a feature within `radius` pixels, for S sequences per call
    (mld_nearest_depths_*, include/mld.h): an exact nearest-first search over the cells of the pixel map - ascending
    (squared pixel distance, y, x) - in place of the fixed pixelarea_search rectangle, so that the list follows the local
    density of the returns; then the count test, the histogram segmentation, the triangle and the intersection exactly as
    FeatureTraces runs them, with the viewing ray through the feature itself.  The reference's neighbor_search_mode 1
    (nnSearch_count nearest: `count` with a generous `radius`; radiusSearch_radius: `radius` with count MAX_COUNT).  No
    road fallback.  It runs on the tensors ProjectedClouds.export wrote (pixel_map, index, cam).  collect() takes float64
    uv, collect_tracks() the float32 u, v of the tracklet layer (truncated to the integer pixel).  `parameters` (default:
    the estimator's) is copied at creation; do_use_PCA and set_all_depths_to_zero are refused.  Lists of S torch CUDA
    tensors in and out; asynchronous on the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "nearest_depths", "_nd"
    WORDS = 8  # int64 words of a record (capi.MldNearestDepth, 64 bytes)
    DTYPE = np.dtype(capi.MldNearestDepth)
    MAX_RADIUS, MAX_COUNT = capi.MLD_NEAREST_MAX_RADIUS, capi.MLD_NEAREST_MAX_COUNT

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_features: int, radius: int, count: int, parameters=None):
        self.S, self.max_features, self.radius, self.count = int(n_seq), int(max_features), int(radius), int(count)
        self._create(estimator, self.S, self.max_features, self.radius, self.count,
                     *self._calibration(estimator, "parameters", "camera", parameters=parameters))

    def _collect(self, ns, feats, maps, index, cam, record, list_capacity, nb):
        cap = int(list_capacity)
        self._lengths(pixel_map=maps, index=index, cam=cam, record=record, nb=nb)
        if not 0 <= cap <= self.count:
            raise ValueError(f"list_capacity must be in 0 .. {self.count}")
        self._cloud_holds(ns, maps, index, cam, "record", record, cap, {"nb": nb})
        fn = self._lib.mld_nearest_depths_collect_device if len(feats) == 1 else self._lib.mld_nearest_depths_collect_tracks_device
        self._check(fn(self._nd, *self._cloud_args(ns, feats, maps, index, cam), cap, self._ptrs(record), self._opt(nb)))
        self._hold(*feats, maps, index, cam, record, nb)

    def collect(self, uv, pixel_map, index, cam, record, list_capacity: int = 0, nb=None):
        """uv: S contiguous float64 CUDA tensors [n, 2] (an entry None: a sequence without features); pixel_map, index,
        cam: the S tensors each that ProjectedClouds.export wrote for the clouds (int32 [height, width], int32 of a
        capacity that did not truncate, float64 [points, 3]); record: S int64 CUDA tensors of at least 8 * n entries (a
        contiguous [n, 8]: capi.MldNearestDepth, see records()); nb: None, or S int32 CUDA tensors of at least
        list_capacity * n entries (a contiguous [n, list_capacity]; single entries may be None): the visible indices of
        the list, nearest first.  A row receives the first min(n_nb, list_capacity) entries; list_capacity is at most
        `count`."""
        self._collect(self._uv_counts(uv), (uv,), pixel_map, index, cam, record, list_capacity, nb)

    def collect_tracks(self, u, v, pixel_map, index, cam, record, list_capacity: int = 0, nb=None):
        """As collect(), on the tensors of TrackletBatch.prepare_step() / prepare(): u, v (u_new, v_new): S float32 CUDA
        tensors [n]."""
        self._collect(self._track_counts(u, v), (u, v), pixel_map, index, cam, record, list_capacity, nb)


class RowGrowth(_FeatureUnit):
    """The reference's second depth segmentation - region growing along lidar rows, do_use_depth_segmentation: 1 - for S
    sequences per call (mld_row_growth_*, include/mld.h): segment() cuts the visible list of every cloud into rows (once
    per cloud), collect() / collect_tracks() find per feature the nearest return of its search window, a second seed in a
    neighbouring row, grow both rows and run the triangle path on the grown points (type 20, SuccessRegionGrowing).  The
    record says what the stage decided (type 20, the early 4 and 3) or that it decided nothing (type 0); with depth and
    types given, the decided entries are merged into the product's outputs in place, which then hold what CalculateDepth
    returns in that mode.  It runs on the tensors ProjectedClouds.export wrote (uv, n_visible, pixel_map, index, cam).
    `growth` (default: capi.row_growth_params_default(), the header values; capi.row_growth_params_yaml(): the shipped
    file's) and `parameters` (default: the estimator's) are copied at creation; do_use_PCA and set_all_depths_to_zero are
    refused.  Lists of S torch CUDA tensors in and out; asynchronous on the estimator's stream.  Close it before its
    estimator."""

    _NAME, _HANDLE = "row_growth", "_rg"
    WORDS = 9  # int64 words of a record (capi.MldRowGrowth, 72 bytes)
    DTYPE = np.dtype(capi.MldRowGrowth)
    CLOUD_DTYPE = np.dtype(capi.MldRowGrowthCloud)
    MAX_COUNT, MAX_LIST, MAX_ROWS = capi.MLD_ROW_GROWTH_MAX_COUNT, capi.MLD_ROW_GROWTH_MAX_LIST, capi.MLD_ROW_GROWTH_MAX_ROWS

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_features: int, max_points: int, row_capacity: int,
                 growth=None, parameters=None):
        self.S, self.max_features, self.max_points = int(n_seq), int(max_features), int(max_points)
        self.row_capacity = int(row_capacity)
        self.growth = growth if growth is not None else capi.row_growth_params_default()
        par, cam, T = self._calibration(estimator, "parameters", "camera", "transform", parameters=parameters)
        self._create(estimator, self.S, self.max_features, self.max_points, self.row_capacity, par, C.byref(self.growth), cam, T)

    @classmethod
    def cloud_records(cls, cloud) -> np.ndarray:
        """The tensor segment() wrote (int32 [S, 4]) as a NumPy record array with the fields of CLOUD_DTYPE (copies to
        the host, which synchronises as usual)."""
        return np.ascontiguousarray(cloud.cpu().numpy()).reshape(-1).view(cls.CLOUD_DTYPE)

    def segment(self, uv, n_visible, row_start, cloud):
        """The cloud stage, once per cloud.  uv: S float64 CUDA tensors [capacity, 2] and n_visible: the int64 CUDA tensor
        [S], both as ProjectedClouds.export wrote them (an entry of uv None: a sequence without capacity); row_start: S
        int32 CUDA tensors of at least row_capacity + 1 entries; cloud: an int32 CUDA tensor [S, 4]
        (capi.MldRowGrowthCloud, see cloud_records())."""
        self._lengths(uv=uv, row_start=row_start)
        _result_tensor(n_visible, (self.S,), 8, "n_visible")
        _result_tensor(cloud, (self.S, 4), 4, "cloud")
        caps = []
        for s in range(self.S):
            _holds(uv[s], s, 0, 8, "uv")
            _holds(row_start[s], s, self.row_capacity + 1, 4, "row_start", required=True)
            caps.append(_entries(uv[s], 2))
        self._check(self._lib.mld_row_growth_segment_device(self._rg, self._ptrs(uv), self._i64(caps), int(n_visible.data_ptr()),
                                                            self._ptrs(row_start), int(cloud.data_ptr())))
        self._hold(uv, n_visible, row_start, cloud, call="segment")

    def _collect(self, ns, feats, maps, index, cam, vis_uv, row_start, cloud, record, list_capacity, grown, depth, types):
        cap = int(list_capacity)
        self._lengths(pixel_map=maps, index=index, cam=cam, vis_uv=vis_uv, row_start=row_start, record=record, grown=grown,
                      depth=depth, types=types)
        if not 0 <= cap <= self.MAX_LIST:
            raise ValueError(f"list_capacity must be in 0 .. {self.MAX_LIST}")
        _result_tensor(cloud, (self.S, 4), 4, "cloud")
        self._cloud_holds(ns, maps, index, cam, "record", record, cap, {"grown": grown})
        tracks = len(feats) == 2
        for s, n in enumerate(ns):
            if n == 0:
                continue
            _holds(vis_uv[s], s, 2 * _entries(index[s]), 8, "vis_uv", required=True)
            _holds(row_start[s], s, self.row_capacity + 1, 4, "row_start", required=True)
            _holds(_at(depth, s), s, n, 4 if tracks else 8, "depth")
            _holds(_at(types, s), s, n, 4, "types")
        fn = self._lib.mld_row_growth_collect_tracks_device if tracks else self._lib.mld_row_growth_collect_device
        self._check(fn(self._rg, *self._cloud_args(ns, feats, maps, index, cam), self._ptrs(vis_uv), self._ptrs(row_start),
                       int(cloud.data_ptr()), cap, self._ptrs(record), self._opt(grown), self._opt(depth), self._opt(types)))
        self._hold(*feats, maps, index, cam, vis_uv, row_start, cloud, record, grown, depth, types)

    def collect(self, uv, pixel_map, index, cam, vis_uv, row_start, cloud, record, list_capacity: int = 0, grown=None,
                depth=None, types=None):
        """uv: S contiguous float64 CUDA tensors [n, 2] (an entry None: a sequence without features); pixel_map, index,
        cam: as NearestDepths.collect takes them; vis_uv, row_start, cloud: what segment() read and wrote for these
        clouds; record: S int64 CUDA tensors of at least 9 * n entries (a contiguous [n, 9]: capi.MldRowGrowth, see
        records()); grown: None, or S int32 CUDA tensors of at least list_capacity * n entries (a contiguous [n,
        list_capacity]; single entries may be None): the visible indices of the grown list in its order, the first
        min(n_grown, list_capacity) of them; depth, types: None, or S float64 / int32 CUDA tensors [n] (single entries
        may be None), the outputs of the depth call for these features: overwritten where the record decides, untouched
        elsewhere."""
        self._collect(self._uv_counts(uv), (uv,), pixel_map, index, cam, vis_uv, row_start, cloud, record, list_capacity, grown,
                      depth, types)

    def collect_tracks(self, u, v, pixel_map, index, cam, vis_uv, row_start, cloud, record, list_capacity: int = 0, grown=None,
                       depth=None, types=None):
        """As collect(), on the tensors of TrackletBatch.prepare_step() / prepare(): u, v (u_new, v_new): S float32 CUDA
        tensors [n]; depth: float32 [n] (d_cur)."""
        self._collect(self._track_counts(u, v), (u, v), pixel_map, index, cam, vis_uv, row_start, cloud, record, list_capacity,
                      grown, depth, types)


class SweepMerge(_BatchObject):
    """The last few lidar sweeps of S sequences carried into the current lidar frame and concatenated, current sweep first
    (mld_sweep_merge_*, include/mld.h - the transform's operation order and the two drop tests are stated there): every
    record is transformed by its sweep's 3x4 matrix, dropped when the result is not finite or outside [min_range,
    max_range], and the rest written as packed 16-byte records in the order (sweep, index within the sweep) - the order in
    which the pixel map, whose cells keep their FIRST return, prefers the current sweep.  Up to max_sweeps sweeps of up to
    max_points points each per sequence, max_sweeps * max_points <= 8 388 607.  Lists of torch CUDA tensors in and out;
    asynchronous on the estimator's stream.  Close it before its estimator."""

    _NAME, _HANDLE = "sweep_merge", "_sm"
    WORDS = 14  # int64 words of a record (capi.MldSweepMergeRecord, 112 bytes)
    DTYPE = np.dtype(capi.MldSweepMergeRecord)
    MAX_SWEEPS = capi.MLD_SWEEP_MAX_SWEEPS

    def __init__(self, estimator: DepthEstimator, n_seq: int, max_sweeps: int, max_points: int):
        self.S, self.max_sweeps, self.max_points = int(n_seq), int(max_sweeps), int(max_points)
        self._create(estimator, self.S, self.max_sweeps, self.max_points)

    @classmethod
    def records(cls, record) -> np.ndarray:
        """A record tensor (int64 [S, 14]) as a NumPy record array with the fields of capi.MldSweepMergeRecord (copies
        to the host, which synchronises as usual)."""
        return np.ascontiguousarray(record.cpu().numpy()).reshape(-1).view(cls.DTYPE)

    def merge(self, sweeps, transforms, capacity, merged, record, sweep_out=None, orig_out=None, min_range: float = 0.0,
              max_range: float = float("inf")):
        """sweeps: S lists of one length n_sweeps (1 .. max_sweeps), sweep 0 the current one, of contiguous float32 CUDA
        tensors [n, 4] or [n, 8] of one width (an entry None: a sweep without points); transforms: None (identity
        throughout), or S lists of n_sweeps entries, each None (identity: the coordinates bit for bit) or at least 12
        float64 values, the row-major 3x4 matrix (a 4x4 passes) from that sweep's lidar frame to the current one;
        capacity: S integers, or None (= the sequence's points, never truncated); merged: S float32 CUDA tensors of at
        least 4 * min(capacity, points) entries (a contiguous [capacity, 4]; None where that is 0); record: an int64 CUDA
        tensor [S, 14] that receives the records (capi.MldSweepMergeRecord, see records()); sweep_out: None, or S uint8
        CUDA tensors of at least min(capacity, points) entries (single entries may be None): the sweep a written record
        came from; orig_out: likewise int32: its index within its sweep.  Kept records at or beyond a sequence's
        capacity are dropped, which the caller sees from the record (n_kept > n_written, MLD_SWEEP_FLAG_TRUNCATED)."""
        self._lengths(sweeps=sweeps, transforms=transforms, capacity=capacity, merged=merged, sweep_out=sweep_out,
                      orig_out=orig_out)
        _result_tensor(record, (self.S, self.WORDS), 8, "record")
        k = len(sweeps[0])
        if any(len(row) != k for row in sweeps) or (transforms is not None and any(len(row) != k for row in transforms)):
            raise ValueError("sweeps, transforms: one number of sweeps for all sequences")
        if not 1 <= k <= self.max_sweeps:
            raise ValueError(f"sweeps: 1 .. {self.max_sweeps} sweeps per sequence")
        flat = [cl for row in sweeps for cl in row]
        width, ns = _cloud_table(flat)
        items = [sum(ns[s * k:(s + 1) * k]) for s in range(self.S)]
        caps = _capacities(capacity, items)
        for s, n in enumerate(items):
            m = min(caps[s], n)
            _holds(merged[s], s, 4 * m, 4, "merged", required=True)
            _holds(_at(sweep_out, s), s, m, 1, "sweep_out")
            _holds(_at(orig_out, s), s, m, 4, "orig_out")
        mats, T = [], None
        if transforms is not None:
            for s, row in enumerate(transforms):
                for t in row:
                    a = None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1)[:12])
                    if a is not None and a.size != 12:
                        raise ValueError(f"sequence {s}: a transform holds at least 12 values (row-major 3x4)")
                    mats.append(a)
            T = (C.c_void_p * len(mats))(*[a.ctypes.data if a is not None else None for a in mats])
        pts = (C.c_void_p * len(flat))(*[int(t.data_ptr()) if t is not None else None for t in flat])
        self._check(self._lib.mld_sweep_merge_run_device(
            self._sm, k, pts, (C.c_int64 * len(ns))(*ns), 4 * width, T, float(min_range), float(max_range), self._i64(caps),
            self._ptrs(merged), self._opt(sweep_out), self._opt(orig_out), int(record.data_ptr())))
        del mats  # (the matrices are consumed before the call returns)
        self._hold(flat, merged, record, sweep_out, orig_out)


class TrackletBatch:
    """The tracklet layer for S independent sequences at once (mld_set_clouds_planes_range_device +
    mld_tracklets_depths_device): the estimator's frame slots are two banks of S slots, sequence s keeps its current
    frame in slot bank * S + s and its previous frame, still resident, in the other bank.  Device tensors in, device
    tensors out; asynchronous.  run() takes the new-track masks from the caller, who then keeps the tracklet maps
    (as TrackletDepthModule does); step() takes the track ids and keeps the maps on the GPU in a TrackletStore.

    The sequences are LANES that start, restart and resume independently: `lane_has_last[s]` says whether the previous
    bank holds a previous frame of lane s (every lane has one after a step; set_previous() gives one to a resumed lane),
    and step(restart=...) / run(restart=...) start a new recording in a lane - the construction of a new
    TrackletDepthModule.  `have_last` is true when every lane has a previous frame; assigning it sets every lane.

    The objects of _ATTACHABLE hang on the batch under their attribute (None until attach_*() made them)."""

    # attribute: (class, its attach method, attributes of the batch that follow (estimator, S) in the constructor).  The
    # attach_* methods, the guard of the methods that need an object and close(), in this order, go by this table.
    _ATTACHABLE = {"semantic_labels": (SemanticLabels, "attach_labels", ()),
                   "store": (TrackletStore, "attach_store", ("max_tracks",)),
                   "planes": (SemanticPlanes, "attach_planes", ()),
                   "rplanes": (RansacPlanes, "attach_ransac_planes", ()),
                   "pclouds": (ProjectedClouds, "attach_projected_clouds", ()),
                   "depth_reports": (DepthReports, "attach_reports", ("max_tracks",)),
                   "inliers": (PlaneInliers, "attach_plane_inliers", ()),
                   "feature_traces": (FeatureTraces, "attach_traces", ("max_tracks",)),
                   "coverage_maps": (CoverageMaps, "attach_coverage", ()),
                   "depth_image_maps": (DepthImages, "attach_depth_images", ()),
                   "region_depth_boxes": (RegionDepths, "attach_region_depths", ()),
                   "nearest_depth_lists": (NearestDepths, "attach_nearest_depths", ("max_tracks",)),
                   "sweep_merger": (SweepMerge, "attach_sweep_merge", ()),
                   "row_growth_lists": (RowGrowth, "attach_row_growth", ("max_tracks",))}

    def __init__(self, parameters, camera: CameraPinhole, transform_lidar_to_cam, n_seq: int, max_tracks: int,
                 device: int = 0, list_capacity=None):
        self.S = int(n_seq)
        self.est = DepthEstimator(device=device, max_frames=2 * self.S, max_features=max_tracks)
        self.est.InitConfig(parameters)
        self.est.Initialize(camera, transform_lidar_to_cam)
        if list_capacity:
            self.est.setListCapacity(*list_capacity)
        self.bank = 0
        self.lane_has_last = [False] * self.S
        self._keep = None
        self._keep_previous = ([], [])  # tensors of set_previous(): held like `_keep`, until their slot is overwritten
        self._slot_set = [[False] * self.S, [False] * self.S]  # per bank and lane: has the slot ever held a cloud?
        self.max_tracks = int(max_tracks)
        for attr in self._ATTACHABLE:
            setattr(self, attr, None)

    def _attach(self, attr, *args):
        """The object of `attr`, made on the first call from (estimator, S, the table's attributes, *args)."""
        if getattr(self, attr, None) is None:
            cls, _, own = self._ATTACHABLE[attr]
            setattr(self, attr, cls(self.est, self.S, *[getattr(self, a) for a in own], *args))
        return getattr(self, attr)

    def _attached(self, attr, method):
        """The object of `attr` for `method`, which cannot run without it."""
        obj = getattr(self, attr, None)
        if obj is None:
            raise DepthEstimatorError(capi.MLD_ERR_NOT_INITIALIZED,
                                      f"TrackletBatch.{method} without {self._ATTACHABLE[attr][1]}")
        return obj

    @property
    def have_last(self) -> bool:
        return all(self.lane_has_last)

    @have_last.setter
    def have_last(self, value):
        self.lane_has_last = [bool(value)] * self.S

    def _lane_flags(self, restart):
        """(uniform have_last or None, have_last flags, restart flags or None) of the next step() / run()."""
        S = self.S
        if restart is not None and len(restart) != S:
            raise ValueError(f"restart: expected {S} flags, one per lane")
        again = [bool(x) for x in restart] if restart is not None else [False] * S
        last = [h and not r for h, r in zip(self.lane_has_last, again)]
        if not any(again) and all(x == last[0] for x in last):
            return last[0], None, None
        return None, (C.c_uint8 * S)(*last), (C.c_uint8 * S)(*again) if any(again) else None

    def _project(self, f, last):
        """setInputCloud of the current bank from the tables `f`.  A call with mixed flags checks the previous-bank slot
        of every lane though it reads nothing of a lane without a previous frame (include/mld.h); where such a slot
        never held a cloud - a batch's first step only - it takes the lane's current cloud and plane, which satisfies
        the check and is never read."""
        S, est, lib = self.S, self.est, self.est._lib
        co = f["coeffs"].ctypes.data_as(C.POINTER(C.c_float))
        est._check(lib.mld_set_clouds_planes_range_device(est._ctx, self.bank * S, S, f["clouds"], f["n"], 16, co, f["masks"]))
        self._slot_set[self.bank] = [True] * S
        for q in range(S if last is not None else 0):
            if not last[q] and not self._slot_set[1 - self.bank][q]:
                est._check(lib.mld_set_clouds_planes_range_device(
                    est._ctx, (1 - self.bank) * S + q, 1, (C.c_void_p * 1)(f["clouds"][q]), (C.c_int64 * 1)(f["n"][q]), 16,
                    f["coeffs"][q].ctypes.data_as(C.POINTER(C.c_float)), (C.c_void_p * 1)(f["masks"][q])))
                self._slot_set[1 - self.bank][q] = True

    def _release(self, nxt, handover):
        """Lets the batch `nxt` (None or this one: nobody) start behind what this one has queued so far - at the end of
        this projection, or behind this step's classification kernel (include/mld.h "Two contexts")."""
        if nxt is not None and nxt is not self:
            if handover == "classify":
                nxt.est.orderAfterClassify(self.est)
            else:
                nxt.est.orderAfter(self.est)

    def _stepped(self, f):
        """The arrays must outlive the asynchronous launches; the previous frame's clouds stay referenced by their slots."""
        self._keep = (self._keep[1] if self._keep else None, f)
        self._keep_previous = (self._keep_previous[1], [])
        self.bank = 1 - self.bank
        self.have_last = True

    def set_previous(self, lane: int, cloud, coeffs, mask):
        """Gives lane `lane` a previous frame without a step - for a lane whose store was loaded with
        store.import_packed(): setInputCloud(cloud, plane) on the ONE slot (1 - bank) * S + lane
        (mld_set_clouds_planes_range_device), and the lane counts as having a previous frame.  cloud: a float32 CUDA
        tensor [n, 4]; coeffs: 4 floats (host); mask: the int32 inlier bitmask."""
        S, est, lib = self.S, self.est, self.est._lib
        if not 0 <= int(lane) < S:
            raise ValueError(f"lane must be in 0 .. {S - 1}")
        co = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(4)
        est._after_torch(cloud)
        est._check(lib.mld_set_clouds_planes_range_device(est._ctx, (1 - self.bank) * S + int(lane), 1,
                                                          (C.c_void_p * 1)(int(cloud.data_ptr())), (C.c_int64 * 1)(int(cloud.shape[0])),
                                                          16, co.ctypes.data_as(C.POINTER(C.c_float)),
                                                          (C.c_void_p * 1)(int(mask.data_ptr()))))
        self._keep_previous[1].append((cloud, mask))
        self._slot_set[1 - self.bank][int(lane)] = True
        self.lane_has_last[int(lane)] = True

    def attach_planes(self, max_points: int = 1 << 19) -> SemanticPlanes:
        """The semantic ground plane estimator of the S sequences that semantic_planes() runs ahead of a step, for clouds
        of up to max_points points (default: 128 beams x 4096, 320 KB of scratch per sequence)."""
        return self._attach("planes", max_points)

    def _estimated_planes(self, clouds, estimate):
        """estimate(result_out, masks_out) on fresh tensors for `clouds`, then ONE device-to-host copy of 32 * S bytes and
        one synchronisation: (coeffs float32 [S, 4], masks, the int32 [S, 8] records on the host)."""
        import torch
        dev = clouds[0].device
        masks = [torch.empty(max(1, mask_words(c.shape[0])), dtype=torch.int32, device=dev) for c in clouds]
        res = torch.empty((self.S, 8), dtype=torch.int32, device=dev)
        self.est._after_torch(clouds[0])
        estimate(res, masks)
        host = np.empty((self.S, 8), dtype=np.int32)
        self.est._check(self.est._lib.mld_synchronize(self.est._ctx))
        host[:] = res.cpu().numpy()
        return np.ascontiguousarray(host[:, :4]).view(np.float32), masks, host

    def semantic_planes(self, clouds, images, labels=(6, 7, 8, 9), threshold: Optional[float] = None):
        """The ground planes process() builds from the label images (tracklet_depth_module.cpp:269-284: labels 6..9,
        threshold ransac_plane_refinement_treshold) for this frame's clouds, ready for prepare_step() / prepare():
        returns (coeffs float32 [S, 4], masks: S int32 CUDA tensors, status int32 [S], counts int32 [S, 2] =
        (n_candidates, n_inliers)).  One call on the GPU, then ONE device-to-host copy of 32 * S bytes and one
        synchronisation per batch: mld_set_clouds_planes_range_device takes the coefficients from the host.  A
        sequence with status 1 (the reference's ExceptionPclInvalid) has zero coefficients and an empty mask; what to do
        with its frame is the caller's decision.  attach_planes() first."""
        planes = self._attached("planes", "semantic_planes")
        if threshold is None:
            threshold = self.est.getParameters().ransac_plane_refinement_treshold
        coeffs, masks, host = self._estimated_planes(
            clouds, lambda res, masks: planes.estimate(clouds, images, labels, threshold, res, masks))
        return coeffs, masks, host[:, 6].copy(), host[:, 4:6].copy()

    def attach_ransac_planes(self, max_points: int = 1 << 19) -> RansacPlanes:
        """The RANSAC ground plane estimator of the S sequences that ransac_planes() runs ahead of a step - for frames
        without a label image -, for clouds of up to max_points points (default: 128 beams x 4096, 66 KB of scratch per
        sequence).  It takes the estimator's parameters as they are now."""
        return self._attach("rplanes", max_points)

    def ransac_planes(self, clouds, seeds):
        """The ground planes setInputCloud estimates by default (RansacPlane::CalculateInliersPlane, parameters
        ransac_plane_*) for this frame's clouds, ready for prepare_step() / prepare(): returns (coeffs float32 [S, 4],
        masks: S int32 CUDA tensors, status int32 [S], counts int32 [S, 3] = (n_candidates, n_inliers, iterations)).
        One call on the GPU, then ONE device-to-host copy of 32 * S bytes and one synchronisation per batch, as
        semantic_planes().  A sequence with status 1 (the reference's ExceptionPclInvalid) has zero coefficients and an
        empty mask; what to do with its frame is the caller's decision.  attach_ransac_planes() first."""
        rplanes = self._attached("rplanes", "ransac_planes")
        coeffs, masks, host = self._estimated_planes(clouds, lambda res, masks: rplanes.estimate(clouds, seeds, res, masks))
        return coeffs, masks, host[:, 6].copy(), np.ascontiguousarray(host[:, [7, 4, 5]])

    def attach_projected_clouds(self, max_points: int = 1 << 19) -> ProjectedClouds:
        """The export of the projected clouds of the S sequences that projected_clouds() runs, for clouds of up to
        max_points points (default: 128 beams x 4096, 66 KB of scratch per sequence)."""
        return self._attach("pclouds", max_points)

    def projected_clouds(self, clouds, depth: bool = False, cam: bool = False, pixel_map: bool = False, capacity=None):
        """The PointcloudData of this frame's clouds as device tensors - what the ROS layer's PublishImageProjectionCloud
        (uv) and PublishPointCloudCameraCs (cam) read: returns a dict with n_visible (int64 [S]), uv (S float64 [capacity,
        2]), index (S int32 [capacity]) and, where asked for, depth (S float64 [capacity]), cam (S float64 [n, 3]) and
        pixel_map (S int32 [height, width]); the rows at and beyond n_visible[s] are not written.  capacity: S integers,
        or None (= n, never truncated).  One call on the GPU and no synchronisation: torch's current stream is made to
        wait for the export, so torch operations may consume the tensors at once; a host read synchronises as usual.
        attach_projected_clouds() first."""
        import torch
        pc = self._attached("pclouds", "projected_clouds")
        dev = next((c.device for c in clouds if c is not None), torch.device("cuda", self.est._device))
        ns = [int(c.shape[0]) if c is not None else 0 for c in clouds]
        caps = _capacities(capacity, ns, clamp=True)
        out = {"n_visible": torch.empty(self.S, dtype=torch.int64, device=dev),
               "uv": [torch.empty((m, 2), dtype=torch.float64, device=dev) for m in caps],
               "index": [torch.empty(m, dtype=torch.int32, device=dev) for m in caps],
               "depth": [torch.empty(m, dtype=torch.float64, device=dev) for m in caps] if depth else None,
               "cam": [torch.empty((n, 3), dtype=torch.float64, device=dev) for n in ns] if cam else None,
               "pixel_map": [torch.empty((pc.height, pc.width), dtype=torch.int32, device=dev) for _ in ns] if pixel_map else None}
        self.est._after_torch(*[c for c in clouds if c is not None][:1])
        pc.export(clouds, caps, out["n_visible"], out["uv"], out["index"], out["depth"], out["cam"], out["pixel_map"])
        self.est.orderTorchAfter()
        return out

    def attach_plane_inliers(self, max_points: int = 1 << 19) -> PlaneInliers:
        """The export of the ground-plane inliers of the S sequences that plane_inliers() runs, for clouds of up to
        max_points points (default: 128 beams x 4096, 4 KB of scratch per sequence, 68 KB with the camx filter on).  It
        takes the estimator's parameters as they are now."""
        return self._attach("inliers", max_points)

    def plane_inliers(self, clouds, masks, lidar: bool = False, cam: bool = False, capacity=None):
        """The inliers of this frame's ground planes as device tensors, from the masks exactly as semantic_planes() /
        ransac_planes() return them: returns a dict with counts (int64 [S, 2] = (n_inliers, n_cloud)), index (S int32
        [capacity]: GroundPlane::getInlinersIndex) and, where asked for, lidar (S float32 [capacity, 3]:
        getMatrixFromIndices) and cam (S float64 [capacity, 3]: getCloudRansacPlane, filtered by
        ransac_plane_use_camx_treshold / ransac_plane_treshold_camx); the rows at and beyond the counts are not written.
        capacity: S integers, or None (= n, never truncated).  One call on the GPU and no synchronisation: torch's
        current stream is made to wait for the export, so torch operations may consume the tensors at once; a host read
        synchronises as usual.  attach_plane_inliers() first."""
        import torch
        inliers = self._attached("inliers", "plane_inliers")
        dev = next((c.device for c in clouds if c is not None), torch.device("cuda", self.est._device))
        ns = [int(c.shape[0]) if c is not None else 0 for c in clouds]
        caps = _capacities(capacity, ns, clamp=True)
        out = {"counts": torch.empty((self.S, 2), dtype=torch.int64, device=dev),
               "index": [torch.empty(m, dtype=torch.int32, device=dev) for m in caps],
               "lidar": [torch.empty((m, 3), dtype=torch.float32, device=dev) for m in caps] if lidar else None,
               "cam": [torch.empty((m, 3), dtype=torch.float64, device=dev) for m in caps] if cam else None}
        self.est._after_torch(*[c for c in clouds if c is not None][:1])
        inliers.export(clouds, masks, caps, out["counts"], out["index"], out["lidar"], out["cam"])
        self.est.orderTorchAfter()
        return out

    def attach_reports(self) -> DepthReports:
        """The statistics and interpolated clouds of the S sequences that reports() queues behind a step, for up to
        max_tracks tracks per sequence."""
        return self._attach("depth_reports")

    def reports(self, f, points: bool = False, capacity=None):
        """The depth-calculation statistics of the tracks of table `f` (prepare_step() / prepare()) and, with points, their
        interpolated clouds - what the ROS layer's PublishDepthCalcStats and PublishPointCloudInterpolated read -, queued
        on the estimator's stream behind the step() / run() of `f` when called after it: DepthReports.collect_tracks on
        the table's u_new, v_new, d_cur and t_cur (t_cur None: counts and other are 0).  Returns a dict with report
        (int64 [S, 24]: counts[21], other, point_count, n_interpolated), points (S float64 [capacity, 3], or None) and
        feature (S int32 [capacity]: the track each point belongs to, or None); rows at and beyond n_interpolated are
        not written.  capacity: S integers, or None (= the number of tracks, never truncated).  No synchronisation:
        torch's current stream is made to wait for the call, so torch operations may consume the tensors at once; a
        host read synchronises as usual.  attach_reports() first."""
        import torch
        reports = self._attached("depth_reports", "reports")
        u_new, v_new = f["features"]
        d_cur, t_cur = f["current"]
        dev = next((t.device for t in d_cur if t is not None), torch.device("cuda", self.est._device))
        caps = _capacities(capacity, [int(t.numel()) for t in d_cur], clamp=True)
        out = {"report": torch.empty((self.S, DepthReports.WORDS), dtype=torch.int64, device=dev),
               "points": [torch.empty((m, 3), dtype=torch.float64, device=dev) for m in caps] if points else None,
               "feature": [torch.empty(m, dtype=torch.int32, device=dev) for m in caps] if points else None}
        self.est._after_torch(*d_cur[:1])
        reports.collect_tracks(u_new, v_new, d_cur, t_cur, out["report"], caps if points else None, out["points"], out["feature"])
        self.est.orderTorchAfter()
        return out

    def attach_traces(self) -> FeatureTraces:
        """The per-feature traces of the S sequences that traces() runs, for up to max_tracks tracks per sequence.  It
        takes the estimator's parameters as they are now."""
        return self._attach("feature_traces")

    def _feature_tables(self, f, clouds):
        """The opening of traces() and nearest_depths(): `clouds` holds what the units read; the u_new, v_new of table
        `f`, whose writers the call will wait for, their device and the tracks of every sequence."""
        import torch
        if clouds.get("cam") is None or clouds.get("pixel_map") is None:
            raise ValueError("clouds: projected_clouds(cam=True, pixel_map=True) of this frame")
        u_new, v_new = f["features"]
        dev = next((t.device for t in u_new if t is not None), torch.device("cuda", self.est._device))
        self.est._after_torch(*[t for t in u_new if t is not None][:1])
        return u_new, v_new, dev, [_entries(t) for t in u_new]

    def traces(self, f, clouds, list_capacity: int = 0, planes: bool = True):
        """Why the tracks of table `f` (prepare_step() / prepare()) got their depths on this frame's clouds:
        FeatureTraces.collect_tracks on the table's u_new, v_new, its planes and masks (planes=False: traced without a
        plane) and on `clouds`, the dict projected_clouds(cam=True, pixel_map=True) returned for the same clouds with
        a capacity that did not truncate.  Returns a dict with trace (S int64 [n, 23]: capi.MldFeatureTrace, see
        FeatureTraces.records()) and, with list_capacity > 0, nb, seg, road and road_inl (S int32 [n, list_capacity]
        each; a row holds the first min(count, list_capacity) entries of its list, the rest is not written).  No
        synchronisation: torch's current stream is made to wait for the call; a host read synchronises as usual.
        attach_traces() first."""
        import torch
        traces = self._attached("feature_traces", "traces")
        u_new, v_new, dev, ns = self._feature_tables(f, clouds)
        cap = int(list_capacity)
        names = ("nb", "seg", "road", "road_inl")
        out = {"trace": [torch.empty((n, FeatureTraces.WORDS), dtype=torch.int64, device=dev) for n in ns]}
        for name in names:
            out[name] = [torch.empty((n, cap), dtype=torch.int32, device=dev) for n in ns] if cap else None
        traces.collect_tracks(u_new, v_new, clouds["pixel_map"], clouds["index"], clouds["cam"], out["trace"],
                              f["coeffs"] if planes else None, list(f["keep"][1]) if planes else None, cap,
                              *[out[name] for name in names])
        self.est.orderTorchAfter()
        return out

    def attach_coverage(self) -> CoverageMaps:
        """The coverage maps of the S sequences that coverage() runs.  It takes the estimator's parameters as they are
        now."""
        return self._attach("coverage_maps")

    def coverage(self, clouds, coeffs=None, masks=None, maps=CoverageMaps.MAPS, bucket=None, capacity=None):
        """Where a feature of this frame can get a depth: CoverageMaps.collect on `clouds`, the dict
        projected_clouds(cam=True, pixel_map=True) returned for this frame's clouds with a capacity that did not
        truncate, and on the planes as prepare() / prepare_step() take them (coeffs float32 [S, 4] on the host, masks S
        int32 CUDA tensors; both None: without planes).  maps: which of nb, road, road_inl, road_far and reach to make;
        bucket: None or (bucket_w, bucket_h); capacity: S integers, or None (= every bucket).  Returns a dict with record
        (int64 [S, 8]: capi.MldCoverageRecord, see CoverageMaps.records()), the maps asked for (S uint8 [height, width]
        each, the others None) and buckets (S int32 [capacity, 3], rows (x, y, n_nb), or None).  No synchronisation:
        torch's current stream is made to wait for the call; a host read synchronises as usual.  attach_coverage()
        first."""
        import torch
        cm = self._attached("coverage_maps", "coverage")
        if clouds.get("cam") is None or clouds.get("pixel_map") is None:
            raise ValueError("clouds: projected_clouds(cam=True, pixel_map=True) of this frame")
        unknown = [m for m in maps if m not in CoverageMaps.MAPS]
        if unknown:
            raise ValueError(f"maps: unknown {unknown}")
        dev = clouds["pixel_map"][0].device
        out = {"record": torch.empty((self.S, CoverageMaps.WORDS), dtype=torch.int64, device=dev), "buckets": None}
        for name in CoverageMaps.MAPS:
            out[name] = [torch.empty((cm.height, cm.width), dtype=torch.uint8, device=dev) for _ in range(self.S)] if name in maps else None
        if bucket is not None:
            caps = _capacities(capacity, [cm.buckets(*bucket)] * self.S, clamp=True)
            out["buckets"] = [torch.empty((m, 3), dtype=torch.int32, device=dev) for m in caps]
        self.est._after_torch(clouds["pixel_map"][0])
        cm.collect(clouds["pixel_map"], clouds["index"], clouds["cam"], out["record"], coeffs, masks,
                   *[out[name] for name in CoverageMaps.MAPS], bucket=bucket, bucket_out=out["buckets"])
        self.est.orderTorchAfter()
        return out

    def attach_depth_images(self) -> DepthImages:
        """The depth images of the S sequences that depth_images() runs.  It takes the estimator's parameters as they
        are now."""
        return self._attach("depth_image_maps")

    def depth_images(self, clouds, coeffs=None, masks=None, grid=None, f64=False):
        """The depth path at every pixel of a grid over this frame's image: DepthImages.render on `clouds`, the dict
        projected_clouds(cam=True, pixel_map=True) returned for this frame's clouds with a capacity that did not
        truncate, and on the planes as prepare() / prepare_step() take them (coeffs float32 [S, 4] on the host, masks S
        int32 CUDA tensors; both None: without planes).  grid: None (every pixel), (x0, y0, step_x, step_y) or all six
        of DepthImages.grid().  Returns a dict with record (int64 [S, 25]: capi.MldDepthImageRecord, see
        DepthImages.records()), type (S uint8 [grid_h, grid_w]), depth32 (S float32 [grid_h, grid_w]) and depth (S
        float64 [grid_h, grid_w] with f64, else None).  No synchronisation: torch's current stream is made to wait for
        the call; a host read synchronises as usual.  attach_depth_images() first."""
        import torch
        di = self._attached("depth_image_maps", "depth_images")
        if clouds.get("cam") is None or clouds.get("pixel_map") is None:
            raise ValueError("clouds: projected_clouds(cam=True, pixel_map=True) of this frame")
        g = di.grid(grid)
        dev = clouds["pixel_map"][0].device
        make = lambda dtype: [torch.empty((g[5], g[4]), dtype=dtype, device=dev) for _ in range(self.S)]
        out = {"record": torch.empty((self.S, DepthImages.WORDS), dtype=torch.int64, device=dev), "type": make(torch.uint8),
               "depth32": make(torch.float32), "depth": make(torch.float64) if f64 else None}
        self.est._after_torch(clouds["pixel_map"][0])
        di.render(clouds["pixel_map"], clouds["index"], clouds["cam"], out["record"], coeffs, masks, grid=g, depth=out["depth"],
                  depth32=out["depth32"], type=out["type"])
        self.est.orderTorchAfter()
        return out

    def attach_region_depths(self, max_boxes: int) -> RegionDepths:
        """The region depths of the S sequences that region_depths() runs, for up to max_boxes boxes per sequence.  It
        takes the estimator's parameters as they are now."""
        return self._attach("region_depth_boxes", max_boxes)

    def region_depths(self, clouds, boxes, masks=None):
        """How far away is what lies in the rectangles `boxes` (S int32 CUDA tensors [n, 4], rows (x0, y0, x1, y1),
        inclusive; an entry None: no box) of this frame: the projected-clouds export, then RegionDepths.collect on what
        it wrote.  clouds: this frame's clouds (S float32 CUDA tensors: projected_clouds(cam=True, pixel_map=True) runs
        first; attach_projected_clouds() for that), or the dict such a call returned for them with a capacity that did not
        truncate.  masks: None, or the S int32 CUDA tensors of the ground planes as semantic_planes() / ransac_planes()
        return them (an entry None: nothing excluded).  Returns the records, S int64 [n, 10] (capi.MldRegionDepth, see
        RegionDepths.records(); None where boxes is).  No synchronisation: torch's current stream is made to wait for the
        call; a host read synchronises as usual.  attach_region_depths() first."""
        import torch
        rd = self._attached("region_depth_boxes", "region_depths")
        if not isinstance(clouds, dict):
            clouds = self.projected_clouds(clouds, cam=True, pixel_map=True)
        if clouds.get("cam") is None or clouds.get("pixel_map") is None:
            raise ValueError("clouds: projected_clouds(cam=True, pixel_map=True) of this frame")
        dev = clouds["pixel_map"][0].device
        record = [torch.empty((_entries(b, 4), RegionDepths.WORDS), dtype=torch.int64, device=dev) if b is not None else None
                  for b in boxes]
        self.est._after_torch(*[b for b in boxes if b is not None][:1], clouds["pixel_map"][0])
        rd.collect(clouds["pixel_map"], clouds["index"], clouds["cam"], boxes, record, masks)
        self.est.orderTorchAfter()
        return record

    def attach_nearest_depths(self, radius: int, count: int) -> NearestDepths:
        """The nearest-return depths of the S sequences that nearest_depths() runs, for up to max_tracks tracks per
        sequence: the `count` (1 .. NearestDepths.MAX_COUNT) closest returns within `radius` (1 .. NearestDepths.MAX_RADIUS)
        pixels.  It takes the estimator's parameters as they are now."""
        return self._attach("nearest_depth_lists", radius, count)

    def nearest_depths(self, f, clouds, list_capacity: int = 0):
        """A depth for the tracks of table `f` (prepare_step() / prepare()) from their nearest returns on this frame's
        clouds - for the tracks whose search rectangle holds too few: NearestDepths.collect_tracks on the table's u_new,
        v_new and on `clouds`, the dict projected_clouds(cam=True, pixel_map=True) returned for the same clouds with a
        capacity that did not truncate.  Returns a dict with record (S int64 [n, 8]: capi.MldNearestDepth, see
        NearestDepths.records()) and nb (S int32 [n, list_capacity]: a row holds the first min(n_nb, list_capacity)
        visible indices of its list, the rest is not written; None with list_capacity 0).  No synchronisation: torch's
        current stream is made to wait for the call; a host read synchronises as usual.  attach_nearest_depths() first."""
        import torch
        nd = self._attached("nearest_depth_lists", "nearest_depths")
        u_new, v_new, dev, ns = self._feature_tables(f, clouds)
        cap = int(list_capacity)
        out = {"record": [torch.empty((n, NearestDepths.WORDS), dtype=torch.int64, device=dev) for n in ns],
               "nb": [torch.empty((n, cap), dtype=torch.int32, device=dev) for n in ns] if cap else None}
        nd.collect_tracks(u_new, v_new, clouds["pixel_map"], clouds["index"], clouds["cam"], out["record"], cap, out["nb"])
        self.est.orderTorchAfter()
        return out

    def attach_row_growth(self, growth=None, row_capacity: int = 4096, max_points: int = 1 << 19) -> RowGrowth:
        """The region growing along lidar rows of the S sequences that row_growth() runs, for up to max_tracks tracks per
        sequence, clouds of up to max_points visible points and row_capacity (1 .. RowGrowth.MAX_ROWS) rows each.  growth:
        a capi.MldRowGrowthParams (None: capi.row_growth_params_default()).  It takes the estimator's parameters as they
        are now."""
        return self._attach("row_growth_lists", max_points, row_capacity, growth)

    def row_growth(self, f, clouds, list_capacity: int = 0, merge=None):
        """A depth for the tracks of table `f` (prepare_step() / prepare()) from the reference's region growing on this
        frame's clouds: RowGrowth.segment on `clouds`, the dict projected_clouds(cam=True, pixel_map=True) returned for
        the same clouds with a capacity that did not truncate, then RowGrowth.collect_tracks on the table's u_new, v_new.
        merge: None, or the pair (depth, types) of S float32 / int32 tensors [n] the step wrote for these tracks
        (f["current"]): the entries the stage decides (type 20, 4, 3) are overwritten in place, the others not touched.
        Returns a dict with record (S int64 [n, 9]: capi.MldRowGrowth, see RowGrowth.records()), grown (S int32 [n,
        list_capacity]: a row holds the first min(n_grown, list_capacity) visible indices of its list, the rest is not
        written; None with list_capacity 0), row_start (S int32 [row_capacity + 1]) and cloud (int32 [S, 4]:
        capi.MldRowGrowthCloud, see RowGrowth.cloud_records()).  No synchronisation: torch's current stream is made to
        wait for the calls; a host read synchronises as usual.  attach_row_growth() first."""
        import torch
        rg = self._attached("row_growth_lists", "row_growth")
        u_new, v_new, dev, ns = self._feature_tables(f, clouds)
        cap = int(list_capacity)
        depth, types = merge if merge is not None else (None, None)
        out = {"record": [torch.empty((n, RowGrowth.WORDS), dtype=torch.int64, device=dev) for n in ns],
               "grown": [torch.empty((n, cap), dtype=torch.int32, device=dev) for n in ns] if cap else None,
               "row_start": [torch.empty(rg.row_capacity + 1, dtype=torch.int32, device=dev) for _ in ns],
               "cloud": torch.empty((self.S, 4), dtype=torch.int32, device=dev)}
        rg.segment(clouds["uv"], clouds["n_visible"], out["row_start"], out["cloud"])
        rg.collect_tracks(u_new, v_new, clouds["pixel_map"], clouds["index"], clouds["cam"], clouds["uv"], out["row_start"],
                          out["cloud"], out["record"], cap, out["grown"], depth, types)
        self.est.orderTorchAfter()
        return out

    def attach_sweep_merge(self, max_sweeps: int, max_points: int) -> SweepMerge:
        """The merge of up to max_sweeps lidar sweeps of up to max_points points each per sequence that merge_sweeps()
        runs ahead of the projection (max_sweeps * max_points <= 8 388 607; 133 KB of scratch per sequence per million
        points of the merged cloud)."""
        return self._attach("sweep_merger", max_sweeps, max_points)

    def merge_sweeps(self, sweeps, transforms, min_range: float = 0.0, max_range: float = float("inf"), sweep: bool = False,
                     orig: bool = False):
        """The current sweep of every sequence with its older sweeps behind it, all in the current lidar frame, ready for
        the projection (prepare_step() / prepare(), projected_clouds(), mld_set_clouds*_device): SweepMerge.merge on
        `sweeps` (S lists of n_sweeps float32 CUDA tensors [n, 4] or [n, 8], sweep 0 the current one) and `transforms`
        (None, or S lists of n_sweeps entries, each None or the row-major 3x4 matrix into the current lidar frame), with a
        capacity that never truncates.  Returns a dict with merged (S float32 [n_kept, 4], views of the tensors the call
        wrote), n (the S host counts n_kept, which the projection takes from the host), record (the S records on the
        host, capi.MldSweepMergeRecord) and, where asked for, sweep (S uint8 [n_kept]: the sweep a record came from)
        and orig (S int32 [n_kept]: its index within its sweep).  One call on the GPU, then ONE device-to-host copy of
        112 * S bytes and one synchronisation per batch: the projection takes its counts from the host.  torch's current
        stream is made to wait for the call.  attach_sweep_merge() first."""
        import torch
        sm = self._attached("sweep_merger", "merge_sweeps")
        if len(sweeps) != self.S:
            raise ValueError(f"sweeps: expected {self.S} entries, one per sequence")
        flat = [c for row in sweeps for c in row if c is not None]
        dev = flat[0].device if flat else torch.device("cuda", self.est._device)
        items = [sum(int(c.shape[0]) for c in row if c is not None) for row in sweeps]
        merged = [torch.empty((n, 4), dtype=torch.float32, device=dev) for n in items]
        record = torch.empty((self.S, SweepMerge.WORDS), dtype=torch.int64, device=dev)
        sw = [torch.empty(n, dtype=torch.uint8, device=dev) for n in items] if sweep else None
        og = [torch.empty(n, dtype=torch.int32, device=dev) for n in items] if orig else None
        self.est._after_torch(*flat[:1])
        sm.merge(sweeps, transforms, None, merged, record, sw, og, min_range, max_range)
        self.est.orderTorchAfter()
        host = SweepMerge.records(record)  # (the copy waits for the call)
        ns = [int(k) for k in host["n_kept"]]
        return {"merged": [m[:k] for m, k in zip(merged, ns)], "n": ns, "record": host,
                "sweep": [t[:k] for t, k in zip(sw, ns)] if sweep else None,
                "orig": [t[:k] for t, k in zip(og, ns)] if orig else None}

    def attach_labels(self) -> SemanticLabels:
        """The label assignment of the S sequences that labels() queues behind a step."""
        return self._attach("semantic_labels")

    def labels(self, f, images, roi, label_out, votes_out=None):
        """The labels of the tracks of table `f` (prepare_step() / prepare()), queued on the estimator's stream - behind
        the step() / run() of `f` when called after it: SemanticLabels.assign on the table's u_new / v_new.
        attach_labels() first."""
        labels = self._attached("semantic_labels", "labels")
        u_new, v_new = f["features"]
        labels.assign(images, roi, u_new, v_new, label_out, votes_out)

    def attach_store(self, max_history: int) -> TrackletStore:
        """The GPU-resident tracklet maps of the S sequences that step() works on."""
        return self._attach("store", max_history)

    def _tables(self, clouds, coeffs, masks, t_cur, t_last, nt, **lists):
        """The table of a frame for step() / run(): a pointer table for clouds, masks and every list of `lists` under
        its name (S tensors each, none of them None), the point counts "n", the track counts "nt" (lengths of `nt`), the
        optional type tables, and what keeps the tensors alive: "keep" = clouds, masks, the lists in their order, t_cur,
        t_last."""
        S = self.S
        vp = lambda ts: (C.c_void_p * S)(*[int(t.data_ptr()) for t in ts])  # noqa: E731
        f = {"clouds": vp(clouds), "n": (C.c_int64 * S)(*[int(c.shape[0]) for c in clouds]),
             "coeffs": np.ascontiguousarray(coeffs, dtype=np.float32).reshape(S, 4), "masks": vp(masks),
             "nt": (C.c_int64 * S)(*[int(t.shape[0]) for t in nt]),
             "t_cur": vp(t_cur) if t_cur is not None else None, "t_last": vp(t_last) if t_last is not None else None}
        f.update((name, vp(ts)) for name, ts in lists.items())
        f["keep"] = (list(clouds), list(masks), *[list(ts) for ts in lists.values()], t_cur, t_last)
        f["features"] = (list(lists["u_new"]), list(lists["v_new"]))
        f["current"] = (list(lists["d_cur"]), list(t_cur) if t_cur is not None else None)
        return f

    def prepare_step(self, clouds, coeffs, masks, ids, u_new, v_new, u_old, v_old, d_cur, d_last, t_cur=None, t_last=None):
        """Pointer tables of one frame of every sequence for step(): as prepare(), with the S int32 CUDA tensors of
        track ids in place of the new-track masks."""
        return self._tables(clouds, coeffs, masks, t_cur, t_last, ids, ids=ids, u_new=u_new, v_new=v_new, u_old=u_old,
                            v_old=v_old, d_cur=d_cur, d_last=d_last)

    def step(self, f, nxt: Optional["TrackletBatch"] = None, handover: str = "projection", restart=None, leaving=None):
        """run() with the tracklet maps on the GPU (mld_tracklets_step_device): projection of the current bank, then
        new-track decision -> depths -> histories as one asynchronous chain.  `f` from prepare_step(); attach_store()
        first.  The histories are read with store.export(...).  restart: None, or S flags - a lane with a flag starts a
        new recording on this frame: its store is emptied first, every id of it is new and its d_last is -1.  With lanes
        that differ (restart, or lane_has_last) the call is mld_tracklets_step_lanes_device, else today's.
        leaving: None, or the buffers of store.set_leaving_sink() as a dict (store.leaving_buffers() makes one) - they
        receive what this step removes from the store: a restarting lane's tracks whole, of the other lanes the tracks
        that end and the entries that fall off (store.export_leaving)."""
        store = self._attached("store", "step")
        est, lib = self.est, self.est._lib
        uniform, last, again = self._lane_flags(restart)
        if leaving is not None:
            store.set_leaving_sink(**{k: leaving[k] for k in TrackletStore.LEAVING_KEYS + ("record",)})
        self._project(f, last)
        self._release(nxt, handover)
        tail = (f["ids"], f["u_new"], f["v_new"], f["u_old"], f["v_old"], f["nt"], f["d_cur"], f["d_last"], f["t_cur"], f["t_last"])
        if last is None:
            rc = lib.mld_tracklets_step_device(est._ctx, store._tr, self.bank, 1 if uniform else 0, *tail)
        else:
            rc = lib.mld_tracklets_step_lanes_device(est._ctx, store._tr, self.bank, last, again, *tail)
        store._check(rc)
        self._stepped(f)

    def prepare(self, clouds, coeffs, masks, u_new, v_new, u_old, v_old, is_new, d_cur, d_last, t_cur=None, t_last=None):
        """Pointer tables of one frame of every sequence (reusable: a steady-state caller prepares one per bank).
        clouds / masks: S torch CUDA tensors ([N,4] float32 / int32 inlier bitmask), coeffs [S,4] float32 (host);
        u_new ... is_new: S CUDA tensors each (float32 x4, uint8); outputs: S CUDA float32 tensors (d_cur, d_last) and
        optional int32 (t_cur, t_last)."""
        return self._tables(clouds, coeffs, masks, t_cur, t_last, u_new, u_new=u_new, v_new=v_new, u_old=u_old, v_old=v_old,
                            is_new=is_new, d_cur=d_cur, d_last=d_last)

    def run(self, f, nxt: Optional["TrackletBatch"] = None, handover: str = "projection", restart=None):
        """One frame of every sequence from prepared tables: projection of the current bank, then the tracklet call.
        `nxt`: another TrackletBatch (other sequences) that takes the next step - it is released as soon as this
        projection has finished, so that its projection runs beside these feature kernels (include/mld.h "Two contexts").
        restart: None, or S flags - a lane with a flag starts a new recording on this frame (the caller's mask marks
        all its tracks new): its previous frame is not used and its d_last is -1."""
        S, est, lib = self.S, self.est, self.est._lib
        uniform, last, _ = self._lane_flags(restart)
        self._project(f, last)
        self._release(nxt, handover)
        tail = (f["u_new"], f["v_new"], f["u_old"], f["v_old"], f["is_new"], f["nt"], f["d_cur"], f["d_last"], f["t_cur"], f["t_last"])
        if last is None:
            est._check(lib.mld_tracklets_depths_device(est._ctx, S, self.bank, 1 if uniform else 0, *tail))
        else:
            est._check(lib.mld_tracklets_depths_lanes_device(est._ctx, S, self.bank, last, *tail))
        self._stepped(f)

    def frame(self, clouds, *args, **kw):
        self.est._after_torch(clouds[0])
        self.run(self.prepare(clouds, *args, **kw))

    def close(self):
        for attr in self._ATTACHABLE:
            if getattr(self, attr, None) is not None:
                getattr(self, attr).close()
                setattr(self, attr, None)
        self.est.close()
