"""The Python batch wrappers of mono_lidar_depth_amd/tracklets.py against a recording stand-in for the library: which C
function each public method calls and with which arguments, which inputs it refuses before any call, and the bookkeeping
of TrackletBatch around the nine attachable objects.  The wrappers never touch the device themselves, so CPU tensors and
a fake library are enough; the expected values are written out from the input tensors."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mono_lidar_depth_amd import (CoverageMaps, DepthEstimatorError, DepthReports, FeatureTraces, PlaneInliers,
                                  ProjectedClouds, RansacPlanes, SemanticLabels, SemanticPlanes, TrackletBatch,
                                  TrackletStore, capi)

S, W, H = 3, 6, 4
CAPS = [40, 0, 2]  # against clouds of 33, no and 5 points: above n, zero, truncating
U8, I16, I32, I64, F32, F64 = torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float64
T12 = [1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3]
ANY = object()


def plain(a):
    """An argument as the test compares it: tables as lists, void pointers as integers, byref() as its object."""
    if isinstance(a, C.Array):
        return list(a)
    if isinstance(a, C.c_void_p):
        return a.value
    if type(a).__name__ == "CArgObject":
        return a._obj
    return a


class FakeLib:
    """Records (name, arguments) of every call; 1 for *_create, b"" for *_last_error, 0 otherwise."""

    def __init__(self, handle=1, status=0):
        self.calls, self.handle, self.status, self.peek, self.seen = [], handle, status, {}, {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, tuple(plain(a) for a in args)))
            if name in self.peek:  # (memory that is only valid during the call)
                self.seen[name] = self.peek[name](args)
            if name.endswith("_create"):
                args[-1]._obj.value = self.status
                return self.handle
            return b"" if name.endswith("_last_error") else 0
        return fn

    def since(self, mark=0):
        return [c for c in self.calls[mark:] if not c[0].endswith("_destroy")]


class FakeEstimator:
    def __init__(self, lib):
        self._lib, self._ctx, self._device = lib, 77, 0
        self._T = np.eye(4)
        self._T[:3, 3] = (0.1, 0.2, 0.3)
        self._camera = SimpleNamespace(as_struct=lambda: capi.MldCamera(100.0, 3.0, 2.0, W, H))
        self.params = capi.MldParams()

    def getParameters(self):
        return self.params

    def _after_torch(self, *tensors):
        pass

    def orderTorchAfter(self):
        pass

    def _check(self, rc):
        assert rc == 0

    def orderAfter(self, other):
        self._lib.calls.append(("orderAfter", (other,)))

    def orderAfterClassify(self, other):
        self._lib.calls.append(("orderAfterClassify", (other,)))

    def close(self):
        self._lib.calls.append(("est.close", ()))


class Floats:
    """Matches a pointer to these values."""

    def __init__(self, values):
        self.values = [float(v) for v in np.ravel(values)]

    def matches(self, p):
        return p is not None and not isinstance(p, (int, list)) and [p[i] for i in range(len(self.values))] == self.values


class Camera:
    def matches(self, cam):
        return isinstance(cam, capi.MldCamera) and (cam.focal_length, cam.principal_point_x, cam.principal_point_y,
                                                    cam.width, cam.height) == (100.0, 3.0, 2.0, W, H)


class Same:
    """Matches byref() of this very object."""

    def __init__(self, obj):
        self.obj = obj

    def matches(self, got):
        return got is self.obj


def assert_call(call, name, want):
    assert call[0] == name
    got = call[1]
    assert len(got) == len(want), f"{name}: {len(got)} arguments"
    for i, (g, w) in enumerate(zip(got, want)):
        if w is ANY:
            continue
        if hasattr(w, "matches"):
            assert w.matches(g), f"{name}: argument {i}"
        else:
            assert type(g) is type(w) and g == w, f"{name}: argument {i}: {g!r} != {w!r}"


def z(shape, dt):
    return torch.zeros(shape, dtype=dt)


def per(shapes, dt):
    return [None if s is None else z(s, dt) for s in shapes]


def P(ts):
    """The pointer table of a list of tensors as plain() shows it."""
    return None if ts is None else [None if t is None else (t.data_ptr() or None) for t in ts]


def apart(n, dt):
    """n entries that are not contiguous."""
    return z(2 * n, dt)[::2]


def clouds(width=4):
    return per([(33, width), None, (5, width)], F32)


def images():
    return [z((H, 8), U8)[:, :W] for _ in range(S)]


COEFFS = np.arange(12, dtype=np.float32).reshape(3, 4)

KINDS = {
    "tracks": lambda est, **kw: TrackletStore(est, S, 10, 4),
    "labels": lambda est, **kw: SemanticLabels(est, S),
    "splanes": lambda est, **kw: SemanticPlanes(est, S, 100),
    "rplanes": lambda est, **kw: RansacPlanes(est, S, 100, **kw),
    "pclouds": lambda est, **kw: ProjectedClouds(est, S, 100),
    "reports": lambda est, **kw: DepthReports(est, S, 50),
    "inliers": lambda est, **kw: PlaneInliers(est, S, 100, **kw),
    "traces": lambda est, **kw: FeatureTraces(est, S, 50, **kw),
    "coverage": lambda est, **kw: CoverageMaps(est, S, **kw),
}
HANDLES = {"tracks": "_tr", "labels": "_lb", "splanes": "_sp", "rplanes": "_rp", "pclouds": "_pc", "reports": "_dr",
           "inliers": "_pi", "traces": "_ft", "coverage": "_cm"}
NAMES = {"tracks": "tracks", "labels": "labels", "splanes": "semantic_planes", "rplanes": "ransac_planes",
         "pclouds": "projected_clouds", "reports": "depth_reports", "inliers": "plane_inliers", "traces": "feature_traces",
         "coverage": "coverage_maps"}


def created(kind, **kw):
    lib = FakeLib()
    est = FakeEstimator(lib)
    obj = KINDS[kind](est, **kw)
    return lib, est, obj


def leaving():
    return dict(ids=per([4, None, 2], I32), offsets=per([5, None, 3], I64), fp=per([(6, 3), None, (2, 3)], F32),
                spill_ids=per([3, None, None], I32), spill_fp=per([(3, 3), None, None], F32), record=z((3, 4), I64))


def trace_tail():
    return dict(pixel_map=per([(H, W), 1, (H, W)], I32), index=per([33, None, 5], I32), cam=per([(33, 3), None, (5, 3)], F64),
                trace=per([(7, 23), None, (3, 23)], I64), coeffs=COEFFS, masks=per([2, None, 1], I32), list_capacity=2,
                nb=per([(7, 2), None, (3, 2)], I32), seg=None, road=per([None, None, (3, 2)], I32), road_inl=None)


def report_tail():
    return dict(types=per([7, None, 3], I32), report=z((3, 24), I64), capacity=CAPS, points=per([(7, 3), None, (2, 3)], F64),
                feature=per([7, None, None], I32))


# an accepted call of every public method that reaches the C ABI: "kind.method" -> keyword arguments
GOOD = {
    "tracks.begin": lambda: dict(ids=per([7, 1, 3], I32), is_new_out=per([7, 1, 3], U8)),
    "tracks.commit": lambda: {k: per([7, 1, 3], F32) for k in ("u_new", "v_new", "u_old", "v_old", "d_cur", "d_last")},
    "tracks.export": lambda: dict(fp_out=per([(7, 4, 3), (1, 4, 3), (3, 4, 3)], F32), len_out=per([7, 1, 3], I32)),
    "tracks.export_packed": lambda: dict(fp_out=per([(28, 3), (4, 3), (2, 3)], F32), offsets_out=per([8, 2, 4], I64)),
    "tracks.export_leaving": lambda: dict(leaving(), flush=[1, 0, 1]),
    "tracks.set_leaving_sink": leaving,
    "tracks.import_packed": lambda: dict(ids=per([2, None, 1], I32), offsets=per([3, None, 2], I64),
                                         fp=per([(5, 3), None, None], F32), select=[1, 0, 1]),
    "tracks.reset": lambda: dict(select=[0, 1, 0]),
    "labels.assign": lambda: dict(images=images(), roi=(5, 3), u=per([7, 1, 3], F32), v=per([7, 1, 3], F32),
                                  label_out=per([7, 1, 3], I16), votes_out=per([(7, 2), None, (3, 2)], I32)),
    "splanes.estimate": lambda: dict(clouds=per([(33, 4), (2, 4), (5, 4)], F32), images=images(), labels=(6, 7, 8, 9),
                                     inlier_threshold=0.25, result_out=z((3, 8), I32), masks_out=per([2, 1, 1], I32)),
    "rplanes.estimate": lambda: dict(clouds=clouds(8), seeds=[1, 2 ** 32 + 5, -1], result_out=z((3, 8), I32),
                                     masks_out=per([2, None, 1], I32)),
    "pclouds.export": lambda: dict(clouds=clouds(), capacity=CAPS, n_visible=z(3, I64), uv=per([(33, 2), None, (2, 2)], F64),
                                   index=per([33, None, 2], I32), depth=None, cam=per([(33, 3), None, (5, 3)], F64),
                                   pixel_map=per([(H, W), None, (H, W)], I32)),
    "reports.collect": lambda: dict(uv=per([(7, 2), None, (3, 2)], F64), depth=per([7, None, 3], F64), **report_tail()),
    "reports.collect_tracks": lambda: dict(u=per([7, None, 3], F32), v=per([7, None, 3], F32), depth=per([7, None, 3], F32),
                                           **report_tail()),
    "inliers.export": lambda: dict(clouds=clouds(), masks=per([2, None, 1], I32), capacity=CAPS, counts=z((3, 2), I64),
                                   index=per([33, None, 2], I32), lidar=None, cam=per([(33, 3), None, (2, 3)], F64)),
    "traces.collect": lambda: dict(uv=per([(7, 2), None, (3, 2)], F64), **trace_tail()),
    "traces.collect_tracks": lambda: dict(u=per([7, None, 3], F32), v=per([7, None, 3], F32), **trace_tail()),
    "coverage.collect": lambda: dict(pixel_map=per([(H, W)] * 3, I32), index=per([33, None, 5], I32),
                                     cam=per([(33, 3), None, (5, 3)], F64), record=z((3, 8), I64), coeffs=COEFFS,
                                     masks=per([2, None, 1], I32), nb=per([(H, W), None, (H, W)], U8), road=None, road_inl=None,
                                     road_far=None, reach=per([(H, W)] * 3, U8), bucket=(4, 2),
                                     bucket_out=per([(6, 3), None, (2, 3)], I32)),
}


def leaving_want(a):
    return [P(a[k]) for k in TrackletStore.LEAVING_KEYS] + [[4, 0, 2], [6, 0, 2], [3, 0, 0], a["record"].data_ptr()]


def trace_want(a):
    return [P(a["pixel_map"]), P(a["index"]), [33, 0, 5], P(a["cam"]), [33, 0, 5], Floats(COEFFS), P(a["masks"]), 2,
            P(a["trace"]), P(a["nb"]), None, P(a["road"]), None]


def report_want(a):
    return [P(a["types"]), [7, 0, 3], CAPS, a["report"].data_ptr(), P(a["points"]), P(a["feature"])]


# the one C call each of them makes: (function, arguments after the handle)
WANT = {
    "tracks.begin": lambda a: ("mld_tracks_begin_device", [P(a["ids"]), [7, 1, 3], P(a["is_new_out"])]),
    "tracks.commit": lambda a: ("mld_tracks_commit_device", [P(a[k]) for k in ("u_new", "v_new", "u_old", "v_old", "d_cur", "d_last")]),
    "tracks.export": lambda a: ("mld_tracks_export_device", [P(a["fp_out"]), P(a["len_out"])]),
    "tracks.export_packed": lambda a: ("mld_tracks_export_packed_device", [P(a["fp_out"]), [28, 4, 2], P(a["offsets_out"])]),
    "tracks.export_leaving": lambda a: ("mld_tracks_export_leaving_device", [[1, 0, 1]] + leaving_want(a)),
    "tracks.set_leaving_sink": lambda a: ("mld_tracks_set_leaving_sink", leaving_want(a)),
    "tracks.import_packed": lambda a: ("mld_tracks_import_packed_device",
                                       [[1, 0, 1], P(a["ids"]), [2, 0, 1], P(a["offsets"]), P(a["fp"]), [5, 0, 0]]),
    "tracks.reset": lambda a: ("mld_tracks_reset_device", [[0, 1, 0]]),
    "labels.assign": lambda a: ("mld_labels_assign_device", [P(a["images"]), H, W, 8, 5, 3, P(a["u"]), P(a["v"]), [7, 1, 3],
                                                             P(a["label_out"]), P(a["votes_out"])]),
    "splanes.estimate": lambda a: ("mld_semantic_planes_estimate_device",
                                   [P(a["clouds"]), [33, 2, 5], 16, P(a["images"]), H, W, 8, ANY, 4, 0.25,
                                    a["result_out"].data_ptr(), P(a["masks_out"])]),
    "rplanes.estimate": lambda a: ("mld_ransac_planes_estimate_device",
                                   [P(a["clouds"]), [33, 0, 5], 32, [1, 5, 0xFFFFFFFF], a["result_out"].data_ptr(), P(a["masks_out"])]),
    "pclouds.export": lambda a: ("mld_projected_clouds_export_device",
                                 [P(a["clouds"]), [33, 0, 5], 16, CAPS, a["n_visible"].data_ptr(), P(a["uv"]), P(a["index"]), None,
                                  P(a["cam"]), P(a["pixel_map"])]),
    "reports.collect": lambda a: ("mld_depth_reports_collect_device", [P(a["uv"]), P(a["depth"])] + report_want(a)),
    "reports.collect_tracks": lambda a: ("mld_depth_reports_collect_tracks_device",
                                         [P(a["u"]), P(a["v"]), P(a["depth"])] + report_want(a)),
    "inliers.export": lambda a: ("mld_plane_inliers_export_device",
                                 [P(a["clouds"]), [33, 0, 5], 16, P(a["masks"]), CAPS, a["counts"].data_ptr(), P(a["index"]), None,
                                  P(a["cam"])]),
    "traces.collect": lambda a: ("mld_feature_traces_collect_device", [P(a["uv"]), [7, 0, 3]] + trace_want(a)),
    "traces.collect_tracks": lambda a: ("mld_feature_traces_collect_tracks_device", [P(a["u"]), P(a["v"]), [7, 0, 3]] + trace_want(a)),
    "coverage.collect": lambda a: ("mld_coverage_maps_collect_device",
                                   [P(a["pixel_map"]), P(a["index"]), [33, 0, 5], P(a["cam"]), [33, 0, 5], Floats(COEFFS),
                                    P(a["masks"]), P(a["nb"]), None, None, None, P(a["reach"]), a["record"].data_ptr(), 4, 2,
                                    [6, 0, 2], P(a["bucket_out"])]),
}


def one_call(key, args, **kw):
    """The calls an object of `key`'s kind records for method(**args) after its creation."""
    kind, method = key.split(".")
    lib, est, obj = created(kind, **kw)
    mark = len(lib.calls)
    getattr(obj, method)(**args)
    return lib, lib.since(mark)


@pytest.mark.parametrize("key", sorted(GOOD))
def test_an_accepted_call_is_one_c_call_with_these_arguments(key):
    args = GOOD[key]()
    lib, calls = one_call(key, args)
    name, want = WANT[key](args)
    assert len(calls) == 1
    assert_call(calls[0], name, [1] + want)


def test_absent_optional_tables_are_null():
    a = dict(GOOD["tracks.begin"](), is_new_out=None)
    assert_call(one_call("tracks.begin", a)[1][0], "mld_tracks_begin_device", [1, P(a["ids"]), [7, 1, 3], None])
    a = dict(GOOD["tracks.export_packed"](), fp_out=None)
    assert_call(one_call("tracks.export_packed", a)[1][0], "mld_tracks_export_packed_device", [1, None, None, P(a["offsets_out"])])
    a = dict(GOOD["tracks.export_leaving"](), flush=None)
    assert one_call("tracks.export_leaving", a)[1][0][1][1] is None
    a = dict(GOOD["tracks.import_packed"](), select=None, ids=per([2, None, 0], I32))
    assert_call(one_call("tracks.import_packed", a)[1][0], "mld_tracks_import_packed_device",
                [1, None, [a["ids"][0].data_ptr(), None, None], [2, 0, 0], [a["offsets"][0].data_ptr(), None, None],
                 P(a["fp"]), [5, 0, 0]])
    assert_call(one_call("tracks.reset", {})[1][0], "mld_tracks_reset_device", [1, None])
    a = dict(GOOD["labels.assign"](), votes_out=None)
    assert one_call("labels.assign", a)[1][0][1][-1] is None
    a = dict(GOOD["pclouds.export"](), capacity=None, uv=per([(33, 2), None, (5, 2)], F64), index=per([33, None, 5], I32),
             depth=per([33, None, 5], F64), cam=None, pixel_map=None)
    got = one_call("pclouds.export", a)[1][0][1]
    assert got[4] == [33, 0, 5] and got[8:] == (P(a["depth"]), None, None)
    a = dict(GOOD["inliers.export"](), capacity=None, index=per([33, None, 5], I32), lidar=per([(33, 3), None, None], F32), cam=None)
    got = one_call("inliers.export", a)[1][0][1]
    assert got[5] == [33, 0, 5] and got[8:] == (P(a["lidar"]), None)
    a = dict(GOOD["traces.collect"](), coeffs=None, masks=None, list_capacity=0, nb=None, road=None)
    assert one_call("traces.collect", a)[1][0][1][8:] == (None, None, 0, P(a["trace"]), None, None, None, None)
    a = dict(GOOD["coverage.collect"](), coeffs=None, masks=None, nb=None, reach=None, bucket=None, bucket_out=None)
    assert one_call("coverage.collect", a)[1][0][1][6:] == (None, None) + (None,) * 5 + (a["record"].data_ptr(), 0, 0, None, None)


def test_a_deselected_sequence_is_handed_over_as_null_whatever_its_entries():
    a = GOOD["tracks.import_packed"]()
    a.update(ids=per([2, 9, 1], I32), offsets=per([3, 1, 2], I64), fp=per([(5, 3), (1, 3), None], F32))
    got = one_call("tracks.import_packed", a)[1][0][1]
    assert got[2] == [a["ids"][0].data_ptr(), None, a["ids"][2].data_ptr()] and got[3] == [2, 0, 1]
    assert got[4] == [a["offsets"][0].data_ptr(), None, a["offsets"][2].data_ptr()]
    assert got[5] == [a["fp"][0].data_ptr(), None, None] and got[6] == [5, 0, 0]


def test_the_leaving_sink_is_taken_away_with_nine_nulls():
    lib, calls = one_call("tracks.set_leaving_sink", {})
    assert_call(calls[0], "mld_tracks_set_leaving_sink", [1] + [None] * 9)


def test_counts_reads_into_an_array_of_its_own():
    lib, est, store = created("tracks")
    out = store.counts()
    assert out.shape == (S, 6) and out.dtype == np.int64 and not out.any()
    assert_call(lib.calls[-1], "mld_tracks_counts", [1, ANY])


def test_the_ground_labels_reach_the_call_as_int32():
    lib, est, sp = created("splanes")
    lib.peek["mld_semantic_planes_estimate_device"] = lambda args: list((C.c_int32 * args[9]).from_address(args[8]))
    sp.estimate(**GOOD["splanes.estimate"]())
    assert lib.seen["mld_semantic_planes_estimate_device"] == [6, 7, 8, 9]


def test_the_label_calls_pass_the_larger_of_row_stride_and_columns():
    a = GOOD["labels.assign"]()
    a["images"] = [z(W, U8).expand(1, W) for _ in range(S)]  # (one row: its stride is not looked at)
    assert one_call("labels.assign", a)[1][0][1][2:5] == (1, W, W)
    a = GOOD["splanes.estimate"]()
    a["images"] = [z(W, U8).expand(1, W) for _ in range(S)]
    assert one_call("splanes.estimate", a)[1][0][1][5:8] == (1, W, W)


def test_clouds_of_eight_floats_and_no_cloud_at_all():
    a = dict(GOOD["pclouds.export"](), clouds=clouds(8))
    assert one_call("pclouds.export", a)[1][0][1][3] == 32
    a = dict(GOOD["rplanes.estimate"](), clouds=[None] * 3, masks_out=[None] * 3)
    assert one_call("rplanes.estimate", a)[1][0][1][1:4] == ([None] * 3, [0, 0, 0], 16)
    a = dict(GOOD["inliers.export"](), clouds=[None] * 3, masks=[None] * 3, index=[None] * 3)
    assert one_call("inliers.export", a)[1][0][1][1:4] == ([None] * 3, [0, 0, 0], 16)


def test_reports_without_points_pass_neither_capacities_nor_the_feature_table():
    for key in ("reports.collect", "reports.collect_tracks"):
        a = dict(GOOD[key](), points=None, capacity=[-1, 0, 2])  # (capacities are not looked at without points)
        got = one_call(key, a)[1][0][1]
        assert got[-5] == [7, 0, 3] and got[-4] is None and got[-3] == a["report"].data_ptr() and got[-2:] == (None, None)
        a = dict(GOOD[key](), types=None, capacity=None, points=per([(7, 3), None, (3, 3)], F64), feature=None)
        got = one_call(key, a)[1][0][1]
        assert got[-6] is None and got[-4] == [7, 0, 3] and got[-2:] == (P(a["points"]), None)


def test_traces_check_nothing_of_a_sequence_without_features():
    a = GOOD["traces.collect"]()
    a["trace"][1], a["nb"][1], a["index"][1] = apart(3, I32), apart(3, F64), z(4, F64)
    got = one_call("traces.collect", a)[1][0][1]
    assert got[3:6] == (P(a["pixel_map"]), P(a["index"]), [33, 4, 5]) and got[11:13] == (P(a["trace"]), P(a["nb"]))
    a = dict(GOOD["traces.collect"](), list_capacity=0)  # (no capacity: the lists are passed on unchecked)
    a["nb"][0] = z(1, F64)
    assert one_call("traces.collect", a)[1][0][1][12] == P(a["nb"])


CREATE = {
    "tracks": lambda est, P_: [S, 10, 4],
    "labels": lambda est, P_: [S],
    "splanes": lambda est, P_: [S, 100, Camera(), Floats(T12)],
    "rplanes": lambda est, P_: [S, 100, Same(P_)],
    "pclouds": lambda est, P_: [S, 100, Camera(), Floats(T12)],
    "reports": lambda est, P_: [S, 50, Camera()],
    "inliers": lambda est, P_: [S, 100, Same(P_), Floats(T12)],
    "traces": lambda est, P_: [S, 50, Same(P_), Camera(), Floats(T12)],
    "coverage": lambda est, P_: [S, Same(P_), Camera(), Floats(T12)],
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_creation(kind):
    lib, est, obj = created(kind)
    assert len(lib.calls) == 1
    assert_call(lib.calls[0], f"mld_{NAMES[kind]}_create", [77] + CREATE[kind](est, est.params) + [ANY])
    assert isinstance(lib.calls[0][1][-1], C.c_int)
    assert getattr(obj, HANDLES[kind]) == 1 and obj._lib is lib and obj._est is est and obj.S == S and obj._keep == {}
    if kind in ("pclouds", "traces", "coverage"):
        assert (obj.width, obj.height) == (W, H)
    obj.close()
    assert lib.calls[1:] == [(f"mld_{NAMES[kind]}_destroy", (1,))] and getattr(obj, HANDLES[kind]) is None
    obj.close()
    assert len(lib.calls) == 2


@pytest.mark.parametrize("kind", ["rplanes", "inliers", "traces", "coverage"])
def test_creation_with_parameters_of_the_callers(kind):
    mine = capi.MldParams()
    lib, est, obj = created(kind, parameters=mine)
    assert_call(lib.calls[0], f"mld_{NAMES[kind]}_create", [77] + CREATE[kind](est, mine) + [ANY])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_failed_creation_raises_with_the_status(kind):
    lib = FakeLib(handle=0, status=capi.MLD_ERR_CAPACITY)
    with pytest.raises(DepthEstimatorError) as e:
        KINDS[kind](FakeEstimator(lib))
    assert e.value.code == capi.MLD_ERR_CAPACITY
    assert [c[0] for c in lib.calls] == [f"mld_{NAMES[kind]}_create", f"mld_{NAMES[kind]}_last_error"]
    assert lib.calls[1][1] == (None,)


def test_mask_words_and_the_constants():
    for cls in (SemanticPlanes, RansacPlanes, PlaneInliers):
        assert [cls.mask_words(n) for n in (0, 1, 32, 33, 64)] == [0, 1, 1, 2, 2]
    assert TrackletStore.COUNT_NAMES == ("live", "new", "old", "features_ok", "features_failed", "duplicates")
    assert TrackletStore.LEAVING_KEYS == ("ids", "offsets", "fp", "spill_ids", "spill_fp")
    assert (DepthReports.WORDS, FeatureTraces.WORDS, CoverageMaps.WORDS) == (24, 23, 8)
    assert FeatureTraces.MAX_LIST == 1024 and SemanticLabels.NO_LABEL == -2
    assert CoverageMaps.MAPS == ("nb", "road", "road_inl", "road_far", "reach")
    assert FeatureTraces.DTYPE.itemsize == 184 and CoverageMaps.DTYPE.itemsize == 64
    lib, est, cm = created("coverage")
    assert cm.buckets(4, 2) == 4 and cm.buckets(5, 3) == 4 and cm.buckets(1, 1) == 24


def entry(name, s, value):
    """Replaces entry s of the list `name`."""
    def change(a):
        a[name] = list(a[name])
        a[name][s] = value
    return change


def short(name):
    def change(a):
        a[name] = list(a[name])[:2]
    return change


def put(**kw):
    return lambda a: a.update(kw)


def lengths(key, names):
    return [(key, f"{n} of two entries", short(n)) for n in names]


def cloud_rows(key, width=4):
    return [(key, "clouds of two widths", entry("clouds", 2, z((5, 12 - width), F32))),
            (key, "clouds of three floats", put(clouds=per([(33, 3), (2, 3), (5, 3)], F32))),
            (key, "a cloud that is not contiguous", entry("clouds", 0, z((33, 2 * width), F32)[:, :width])),
            (key, "a cloud of doubles", entry("clouds", 0, z((33, width), F64))),
            (key, "a cloud of one dimension", entry("clouds", 2, z(20, F32)))]


REFUSALS = (
    lengths("tracks.begin", ["ids", "is_new_out"]) +
    lengths("tracks.commit", ["u_new", "v_new", "u_old", "v_old", "d_cur", "d_last"]) +
    lengths("tracks.export", ["fp_out", "len_out"]) +
    lengths("tracks.export_packed", ["fp_out", "offsets_out"]) +
    lengths("tracks.export_leaving", list(TrackletStore.LEAVING_KEYS) + ["flush"]) +
    lengths("tracks.set_leaving_sink", list(TrackletStore.LEAVING_KEYS)) +
    lengths("tracks.import_packed", ["ids", "offsets", "fp"]) +
    lengths("tracks.reset", ["select"]) +
    lengths("labels.assign", ["images", "u", "v", "label_out", "votes_out"]) +
    lengths("splanes.estimate", ["clouds", "images", "masks_out"]) +
    lengths("rplanes.estimate", ["clouds", "seeds", "masks_out"]) +
    lengths("pclouds.export", ["clouds", "capacity", "uv", "index", "cam", "pixel_map"]) +
    lengths("reports.collect", ["uv", "depth", "types", "capacity", "points", "feature"]) +
    lengths("reports.collect_tracks", ["u", "v", "depth", "types", "capacity", "points", "feature"]) +
    lengths("inliers.export", ["clouds", "masks", "capacity", "index", "cam"]) +
    lengths("traces.collect", ["uv", "pixel_map", "index", "cam", "trace", "masks", "nb", "road"]) +
    lengths("traces.collect_tracks", ["u", "v", "pixel_map"]) +
    lengths("coverage.collect", ["pixel_map", "index", "cam", "masks", "nb", "reach", "bucket_out"]) +
    cloud_rows("splanes.estimate") + cloud_rows("rplanes.estimate", 8) + cloud_rows("pclouds.export") + cloud_rows("inliers.export") +
    [
        ("pclouds.export", "depth of two entries", put(depth=per([33, None], F64))),
        ("inliers.export", "lidar of two entries", put(lidar=per([(33, 3), None], F32))),
        ("traces.collect", "seg of two entries", put(seg=per([(7, 2), None], I32))),
        ("traces.collect", "road_inl of two entries", put(road_inl=per([(7, 2), None], I32))),
        ("coverage.collect", "road of two entries", put(road=per([(H, W), None], U8))),
        ("coverage.collect", "road_inl of two entries", put(road_inl=per([(H, W), None], U8))),
        ("coverage.collect", "road_far of two entries", put(road_far=per([(H, W), None], U8))),
        # the tracklet store
        ("tracks.export_packed", "fp_out that is not contiguous", entry("fp_out", 1, z((4, 6), F32)[:, :3])),
        ("tracks.export_leaving", "ids that are not contiguous", entry("ids", 0, apart(4, I32))),
        ("tracks.export_leaving", "fp that is not contiguous", entry("fp", 2, z((2, 6), F32)[:, :3])),
        ("tracks.export_leaving", "a record of int32", put(record=z((3, 4), I32))),
        ("tracks.export_leaving", "a record of two sequences", put(record=z((2, 4), I64))),
        ("tracks.export_leaving", "a record that is not contiguous", put(record=z((3, 8), I64)[:, ::2])),
        ("tracks.export_leaving", "offsets of as many entries as ids", entry("offsets", 0, z(4, I64))),
        ("tracks.export_leaving", "offsets missing beside ids", entry("offsets", 2, None)),
        ("tracks.export_leaving", "spill_fp shorter than spill_ids", entry("spill_fp", 0, z((2, 3), F32))),
        ("tracks.export_leaving", "spill_fp missing beside spill_ids", entry("spill_fp", 0, None)),
        ("tracks.set_leaving_sink", "offsets of as many entries as ids", entry("offsets", 0, z(4, I64))),
        ("tracks.set_leaving_sink", "spill_fp shorter than spill_ids", entry("spill_fp", 0, z((2, 3), F32))),
        ("tracks.set_leaving_sink", "a record of two sequences", put(record=z((2, 4), I64))),
        ("tracks.import_packed", "select of four entries", put(select=[1, 0, 1, 1])),
        ("tracks.import_packed", "offsets missing", entry("offsets", 0, None)),
        ("tracks.import_packed", "offsets of as many entries as ids", entry("offsets", 0, z(2, I64))),
        ("tracks.import_packed", "offsets of int32", entry("offsets", 2, z(2, I32))),
        ("tracks.import_packed", "offsets that are not contiguous", entry("offsets", 0, apart(3, I64))),
        ("tracks.import_packed", "fp of doubles", entry("fp", 0, z((5, 3), F64))),
        ("tracks.import_packed", "fp that is not contiguous", entry("fp", 0, z((5, 6), F32)[:, :3])),
        # label images
        ("labels.assign", "an image of another shape", entry("images", 1, z((H, 8), U8)[:, :5])),
        ("labels.assign", "an image of another row stride", entry("images", 2, z((H, 16), U8)[:, :W])),
        ("labels.assign", "an image whose columns lie apart", entry("images", 0, z((H, 16), U8)[:, ::2][:, :W])),
        ("labels.assign", "v of another length", entry("v", 0, z(6, F32))),
        ("labels.assign", "label_out of another length", entry("label_out", 2, z(4, I16))),
        ("labels.assign", "votes_out of another shape", entry("votes_out", 0, z((7, 3), I32))),
        ("splanes.estimate", "an image of another shape", entry("images", 1, z((H, 8), U8)[:, :5])),
        ("splanes.estimate", "an image of another row stride", entry("images", 2, z((H, 16), U8)[:, :W])),
        # the plane estimators
        ("splanes.estimate", "a mask of one word for 33 points", entry("masks_out", 0, z(1, I32))),
        ("splanes.estimate", "a result of 7 columns", put(result_out=z((3, 7), I32))),
        ("splanes.estimate", "a result of int64", put(result_out=z((3, 8), I64))),
        ("splanes.estimate", "a result that is not contiguous", put(result_out=z((3, 16), I32)[:, ::2])),
        ("rplanes.estimate", "a mask of one word for 33 points", entry("masks_out", 0, z(1, I32))),
        ("rplanes.estimate", "a mask missing beside its cloud", entry("masks_out", 2, None)),
        ("rplanes.estimate", "a result of 7 columns", put(result_out=z((3, 7), I32))),
        ("rplanes.estimate", "a result of int64", put(result_out=z((3, 8), I64))),
        ("rplanes.estimate", "a result that is not contiguous", put(result_out=z((3, 16), I32)[:, ::2])),
        # projected clouds
        ("pclouds.export", "a negative capacity", put(capacity=[40, 0, -1])),
        ("pclouds.export", "n_visible of four", put(n_visible=z(4, I64))),
        ("pclouds.export", "n_visible of int32", put(n_visible=z(3, I32))),
        ("pclouds.export", "n_visible that is not contiguous", put(n_visible=apart(3, I64))),
        ("pclouds.export", "uv missing", entry("uv", 2, None)),
        ("pclouds.export", "uv of 65 entries for 33 points", entry("uv", 0, z(65, F64))),
        ("pclouds.export", "uv of floats", entry("uv", 0, z((33, 2), F32))),
        ("pclouds.export", "uv that is not contiguous", entry("uv", 2, apart(4, F64))),
        ("pclouds.export", "index missing", entry("index", 0, None)),
        ("pclouds.export", "index of one entry for two", entry("index", 2, z(1, I32))),
        ("pclouds.export", "index of int64", entry("index", 2, z(2, I64))),
        ("pclouds.export", "depth of 32 entries for 33 points", put(depth=per([32, None, 2], F64))),
        ("pclouds.export", "cam of the capacity, not of the cloud", entry("cam", 2, z((2, 3), F64))),
        ("pclouds.export", "a pixel map of 23 cells", entry("pixel_map", 0, z(23, I32))),
        ("pclouds.export", "a pixel map of bytes", entry("pixel_map", 2, z((H, W), U8))),
        # depth reports
        ("reports.collect", "a report of 23 words", put(report=z((3, 23), I64))),
        ("reports.collect", "a report of int32", put(report=z((3, 24), I32))),
        ("reports.collect", "a report that is not contiguous", put(report=z((3, 48), I64)[:, ::2])),
        ("reports.collect", "types of another length", entry("types", 0, z(8, I32))),
        ("reports.collect", "types of int64", entry("types", 2, z(3, I64))),
        ("reports.collect", "types that are not contiguous", entry("types", 2, apart(3, I32))),
        ("reports.collect", "a negative capacity", put(capacity=[-1, 0, 2])),
        ("reports.collect", "points missing", entry("points", 0, None)),
        ("reports.collect", "points of 5 entries for two", entry("points", 2, z(5, F64))),
        ("reports.collect", "points of floats", entry("points", 2, z((2, 3), F32))),
        ("reports.collect", "feature of 6 entries for 7", entry("feature", 0, z(6, I32))),
        ("reports.collect", "feature of int64", entry("feature", 0, z(7, I64))),
        ("reports.collect", "uv missing beside depth", entry("uv", 0, None)),
        ("reports.collect", "uv of floats", entry("uv", 0, z((7, 2), F32))),
        ("reports.collect", "uv that is not contiguous", entry("uv", 2, z((3, 4), F64)[:, :2])),
        ("reports.collect", "uv of another length than depth", entry("uv", 2, z((4, 2), F64))),
        ("reports.collect", "uv without depth", entry("uv", 1, z((1, 2), F64))),
        ("reports.collect", "depth of floats", entry("depth", 0, z(7, F32))),
        ("reports.collect_tracks", "u missing beside depth", entry("u", 0, None)),
        ("reports.collect_tracks", "v of doubles", entry("v", 0, z(7, F64))),
        ("reports.collect_tracks", "u of another length than depth", entry("u", 2, z(4, F32))),
        ("reports.collect_tracks", "depth that is not contiguous", entry("depth", 2, apart(3, F32))),
        ("reports.collect_tracks", "a negative capacity", put(capacity=[40, 0, -2])),
        ("reports.collect_tracks", "a report of 23 words", put(report=z((3, 23), I64))),
        # plane inliers
        ("inliers.export", "a negative capacity", put(capacity=[40, -1, 2])),
        ("inliers.export", "counts of three columns", put(counts=z((3, 3), I64))),
        ("inliers.export", "counts of int32", put(counts=z((3, 2), I32))),
        ("inliers.export", "counts that are not contiguous", put(counts=z((3, 4), I64)[:, ::2])),
        ("inliers.export", "a mask missing beside its cloud", entry("masks", 2, None)),
        ("inliers.export", "a mask of one word for 33 points", entry("masks", 0, z(1, I32))),
        ("inliers.export", "index missing", entry("index", 0, None)),
        ("inliers.export", "index of one entry for two", entry("index", 2, z(1, I32))),
        ("inliers.export", "lidar of doubles", put(lidar=per([(33, 3), None, (2, 3)], F64))),
        ("inliers.export", "lidar of 5 entries for two points", put(lidar=per([(33, 3), None, 5], F32))),
        ("inliers.export", "cam of 98 entries for 33 points", entry("cam", 0, z(98, F64))),
        # feature traces
        ("traces.collect", "a list capacity below 0", put(list_capacity=-1)),
        ("traces.collect", "a list capacity above 1024", put(list_capacity=1025)),
        ("traces.collect", "coeffs without masks", put(masks=None)),
        ("traces.collect", "masks without coeffs", put(coeffs=None)),
        ("traces.collect", "a pixel map missing", entry("pixel_map", 0, None)),
        ("traces.collect", "a pixel map of 23 cells", entry("pixel_map", 2, z(23, I32))),
        ("traces.collect", "index of int64", entry("index", 0, z(33, I64))),
        ("traces.collect", "cam of floats", entry("cam", 2, z((5, 3), F32))),
        ("traces.collect", "cam that is not contiguous", entry("cam", 2, z((5, 6), F64)[:, :3])),
        ("traces.collect", "a trace missing", entry("trace", 2, None)),
        ("traces.collect", "a trace of 22 words a feature", entry("trace", 0, z((7, 22), I64))),
        ("traces.collect", "a trace of int32", entry("trace", 0, z((7, 23), I32))),
        ("traces.collect", "a list of one entry a feature for a capacity of two", entry("nb", 0, z((7, 1), I32))),
        ("traces.collect", "a list of int64", entry("road", 2, z((3, 2), I64))),
        ("traces.collect", "uv of floats", entry("uv", 0, z((7, 2), F32))),
        ("traces.collect", "uv of an odd number of entries", entry("uv", 0, z(15, F64))),
        ("traces.collect", "uv that is not contiguous", entry("uv", 2, z((3, 4), F64)[:, :2])),
        ("traces.collect_tracks", "u without v", entry("v", 0, None)),
        ("traces.collect_tracks", "u and v of two lengths", entry("v", 2, z(4, F32))),
        ("traces.collect_tracks", "u of doubles", entry("u", 0, z(7, F64))),
        ("traces.collect_tracks", "v that is not contiguous", entry("v", 2, apart(3, F32))),
        ("traces.collect_tracks", "a list capacity above 1024", put(list_capacity=1025)),
        ("traces.collect_tracks", "coeffs without masks", put(masks=None)),
        # coverage maps
        ("coverage.collect", "coeffs without masks", put(masks=None)),
        ("coverage.collect", "masks without coeffs", put(coeffs=None)),
        ("coverage.collect", "bucket without bucket_out", put(bucket_out=None)),
        ("coverage.collect", "bucket_out without bucket", put(bucket=None)),
        ("coverage.collect", "a record of 7 words a sequence", put(record=z((3, 7), I64))),
        ("coverage.collect", "a record of int32", put(record=z((3, 8), I32))),
        ("coverage.collect", "a record that is not contiguous", put(record=z((3, 16), I64)[:, ::2])),
        ("coverage.collect", "a pixel map missing", entry("pixel_map", 1, None)),
        ("coverage.collect", "a pixel map of 23 cells", entry("pixel_map", 1, z(23, I32))),
        ("coverage.collect", "a pixel map of int64", entry("pixel_map", 0, z((H, W), I64))),
        ("coverage.collect", "index of int64", entry("index", 0, z(33, I64))),
        ("coverage.collect", "cam of floats", entry("cam", 2, z((5, 3), F32))),
        ("coverage.collect", "a map of 23 cells", entry("nb", 0, z(23, U8))),
        ("coverage.collect", "a map of int32", entry("reach", 1, z((H, W), I32))),
        ("coverage.collect", "a map that is not contiguous", entry("reach", 2, z((H, 8), U8)[:, :W])),
        ("coverage.collect", "bucket_out of int64", entry("bucket_out", 0, z((6, 3), I64))),
        ("coverage.collect", "bucket_out that is not contiguous", entry("bucket_out", 2, z((2, 6), I32)[:, :3])),
    ])


@pytest.mark.parametrize("key,what,change", REFUSALS, ids=[f"{k}: {w}" for k, w, _ in REFUSALS])
def test_a_refused_input_raises_before_any_c_call(key, what, change):
    kind, method = key.split(".")
    lib, est, obj = created(kind)
    args = GOOD[key]()
    change(args)
    with pytest.raises(ValueError):
        getattr(obj, method)(**args)
    assert lib.since(1) == []


def test_semantic_planes_refuse_a_sequence_without_a_cloud():
    for s in range(S):
        lib, est, sp = created("splanes")
        args = GOOD["splanes.estimate"]()
        args["clouds"][s] = None
        with pytest.raises((ValueError, AttributeError)):
            sp.estimate(**args)
        assert lib.since(1) == []


def test_leaving_buffers_want_one_count_per_sequence():
    lib, est, store = created("tracks")
    with pytest.raises(ValueError):
        store.leaving_buffers([1, 2], device=torch.device("cpu"))
    buf = store.leaving_buffers([2, 0, 1], device=torch.device("cpu"))
    assert [tuple(t.shape) for t in buf["fp"]] == [(8, 3), (0, 3), (4, 3)] and tuple(buf["record"].shape) == (S, 4)
    assert [t.numel() for t in buf["offsets"]] == [3, 1, 2] and set(buf) == set(TrackletStore.LEAVING_KEYS) | {"record"}


def test_the_tensors_of_a_call_stay_referenced_for_two_calls():
    import gc
    import weakref
    lib, est, pc = created("pclouds")
    refs = []
    for _ in range(3):
        a = GOOD["pclouds.export"]()
        refs.append(weakref.ref(a["uv"][0]))
        pc.export(**a)
        del a
    gc.collect()
    assert refs[0]() is None and refs[1]() is not None and refs[2]() is not None
    lib, est, store = created("tracks")
    a = GOOD["tracks.begin"]()
    ref = weakref.ref(a["ids"][0])
    store.begin(**a)
    del a
    gc.collect()
    assert ref() is not None
    store.close()
    gc.collect()
    assert ref() is None


# ---- TrackletBatch ----

ATTACH = [  # (attach method, its arguments, attribute, class, consumer, a consumer call, creation arguments behind ctx)
    ("attach_store", (4,), "store", TrackletStore, "step", lambda tb: tb.step({}), lambda P_: [S, 10, 4]),
    ("attach_labels", (), "semantic_labels", SemanticLabels, "labels", lambda tb: tb.labels({}, [], (1, 1), []), lambda P_: [S]),
    ("attach_planes", (), "planes", SemanticPlanes, "semantic_planes", lambda tb: tb.semantic_planes([], []),
     lambda P_: [S, 1 << 19, Camera(), Floats(T12)]),
    ("attach_ransac_planes", (), "rplanes", RansacPlanes, "ransac_planes", lambda tb: tb.ransac_planes([], []),
     lambda P_: [S, 1 << 19, Same(P_)]),
    ("attach_projected_clouds", (), "pclouds", ProjectedClouds, "projected_clouds", lambda tb: tb.projected_clouds([]),
     lambda P_: [S, 1 << 19, Camera(), Floats(T12)]),
    ("attach_reports", (), "depth_reports", DepthReports, "reports", lambda tb: tb.reports({}), lambda P_: [S, 10, Camera()]),
    ("attach_plane_inliers", (), "inliers", PlaneInliers, "plane_inliers", lambda tb: tb.plane_inliers([], []),
     lambda P_: [S, 1 << 19, Same(P_), Floats(T12)]),
    ("attach_traces", (), "feature_traces", FeatureTraces, "traces", lambda tb: tb.traces({}, {}),
     lambda P_: [S, 10, Same(P_), Camera(), Floats(T12)]),
    ("attach_coverage", (), "coverage_maps", CoverageMaps, "coverage", lambda tb: tb.coverage({}),
     lambda P_: [S, Same(P_), Camera(), Floats(T12)]),
]


def batch(lib=None):
    """A TrackletBatch on the fake estimator: the fields its methods need, without a context."""
    lib = lib or FakeLib()
    tb = TrackletBatch.__new__(TrackletBatch)
    tb.S, tb.est, tb.max_tracks = S, FakeEstimator(lib), 10
    tb.bank, tb.lane_has_last = 0, [False] * S
    tb._keep, tb._keep_previous = None, ([], [])
    tb._slot_set = [[False] * S, [False] * S]
    for row in ATTACH:
        setattr(tb, row[2], None)
    return lib, tb


@pytest.mark.parametrize("row", ATTACH, ids=[r[0] for r in ATTACH])
def test_attach_creates_once_and_the_consumer_names_it(row):
    attach, args, attr, cls, consumer, call, create = row
    lib, tb = batch()
    with pytest.raises(DepthEstimatorError) as e:
        call(tb)
    assert e.value.code == capi.MLD_ERR_NOT_INITIALIZED and f"TrackletBatch.{consumer} without {attach}" in str(e.value)
    assert lib.calls == []
    obj = getattr(tb, attach)(*args)
    assert type(obj) is cls and getattr(tb, attr) is obj and obj._est is tb.est
    assert len(lib.calls) == 1
    assert_call(lib.calls[0], f"mld_{cls._NAME}_create", [77] + create(tb.est.params) + [ANY])
    assert getattr(tb, attach)(*args) is obj and len(lib.calls) == 1


def test_attach_takes_the_size_of_the_clouds():
    for attach in ("attach_planes", "attach_ransac_planes", "attach_projected_clouds", "attach_plane_inliers"):
        lib, tb = batch()
        assert getattr(tb, attach)(max_points=123).max_points == 123 and lib.calls[0][1][2] == 123
    lib, tb = batch()
    assert tb.attach_store(max_history=5).max_history == 5


def test_close_destroys_every_attached_object_once_and_before_the_estimator():
    lib, tb = batch()
    for attach, args, *_ in ATTACH:
        getattr(tb, attach)(*args)
    mark = len(lib.calls)
    tb.close()
    names = [c[0] for c in lib.calls[mark:]]
    assert sorted(names[:-1]) == sorted(f"mld_{r[3]._NAME}_destroy" for r in ATTACH) and names[-1] == "est.close"
    assert all(getattr(tb, r[2]) is None for r in ATTACH)
    lib, tb = batch()
    tb.attach_labels()
    tb.close()
    assert [c[0] for c in lib.calls[1:]] == ["mld_labels_destroy", "est.close"]


def frame_lists(n=(7, 1, 3)):
    return dict(clouds=per([(33, 4), (2, 4), (5, 4)], F32), coeffs=COEFFS, masks=per([2, 1, 1], I32),
                u_new=per(n, F32), v_new=per(n, F32), u_old=per(n, F32), v_old=per(n, F32), d_cur=per(n, F32),
                d_last=per(n, F32), t_cur=per(n, I32), t_last=None)


TABLES = ("clouds", "masks", "u_new", "v_new", "u_old", "v_old", "d_cur", "d_last", "t_cur")


@pytest.mark.parametrize("which,extra", [("prepare", "is_new"), ("prepare_step", "ids")])
def test_prepare_builds_the_tables_of_a_frame(which, extra):
    lib, tb = batch()
    a = frame_lists()
    a[extra] = per([7, 1, 3], U8 if extra == "is_new" else I32)
    f = getattr(tb, which)(**a)
    assert set(f) == set(TABLES) | {extra, "n", "nt", "coeffs", "t_last", "keep", "features", "current"}
    for k in TABLES + (extra,):
        assert isinstance(f[k], C.c_void_p * S) and list(f[k]) == P(a[k]), k
    assert f["t_last"] is None and list(f["n"]) == [33, 2, 5] and list(f["nt"]) == [7, 1, 3]
    assert isinstance(f["n"], C.c_int64 * S) and isinstance(f["nt"], C.c_int64 * S)
    assert f["coeffs"].dtype == np.float32 and f["coeffs"].shape == (S, 4) and np.array_equal(f["coeffs"], COEFFS)
    assert f["coeffs"].flags.c_contiguous
    order = ("clouds", "masks", "ids", "u_new", "v_new", "u_old", "v_old", "is_new", "d_cur", "d_last", "t_cur", "t_last")
    want = [a[k] for k in order if k in a]
    assert len(f["keep"]) == 11 and all(g is None if w is None else list(g) == w for g, w in zip(f["keep"], want))
    assert f["features"] == (a["u_new"], a["v_new"]) and f["current"] == (a["d_cur"], a["t_cur"])
    assert lib.calls == []
    f = getattr(tb, which)(**dict(a, t_cur=None, t_last=per([7, 1, 3], I32)))
    assert f["t_cur"] is None and f["current"] == (a["d_cur"], None) and list(f["t_last"]) == P(f["keep"][-1])
    for k in TABLES[:-1] + (extra,):  # an entry None is not passed down as NULL
        with pytest.raises((AttributeError, ValueError, TypeError)):
            getattr(tb, which)(**dict(a, **{k: [a[k][0], None, a[k][2]]}))


def tail_of(f, first):
    return [list(f[k]) if f[k] is not None else None
            for k in first + ("nt", "d_cur", "d_last", "t_cur", "t_last")]


def projection(f, bank):
    return ("mld_set_clouds_planes_range_device", [77, bank * S, S, list(f["clouds"]), list(f["n"]), 16, Floats(COEFFS), list(f["masks"])])


def test_step_projects_hands_over_and_steps():
    lib, tb = batch()
    other = batch(lib)[1]
    tb.attach_store(4)
    f = tb.prepare_step(ids=per([7, 1, 3], I32), **frame_lists())
    tail = tail_of(f, ("ids", "u_new", "v_new", "u_old", "v_old"))
    mark = len(lib.calls)
    tb.step(f)
    assert [c[0] for c in lib.calls[mark:]] == ["mld_set_clouds_planes_range_device", "mld_tracklets_step_device"]
    assert_call(lib.calls[mark], *projection(f, 0))
    assert_call(lib.calls[mark + 1], "mld_tracklets_step_device", [77, 1, 0, 0] + tail)
    assert tb.bank == 1 and tb.lane_has_last == [True] * S and tb._keep == (None, f)
    mark = len(lib.calls)
    tb.step(f, nxt=other)
    assert [c[0] for c in lib.calls[mark:]] == ["mld_set_clouds_planes_range_device", "orderAfter", "mld_tracklets_step_device"]
    assert_call(lib.calls[mark], *projection(f, 1))
    assert lib.calls[mark + 1][1] == (tb.est,)
    assert_call(lib.calls[mark + 2], "mld_tracklets_step_device", [77, 1, 1, 1] + tail)
    assert tb.bank == 0 and tb._keep == (f, f)
    mark = len(lib.calls)
    tb.step(f, nxt=other, handover="classify", restart=[0, 1, 0])
    assert [c[0] for c in lib.calls[mark:]] == ["mld_set_clouds_planes_range_device", "orderAfterClassify",
                                                "mld_tracklets_step_lanes_device"]
    assert_call(lib.calls[mark + 2], "mld_tracklets_step_lanes_device", [77, 1, 0, [1, 0, 1], [0, 1, 0]] + tail)
    mark = len(lib.calls)
    tb.step(f, nxt=tb)  # (itself: nothing to hand over)
    assert [c[0] for c in lib.calls[mark:]] == ["mld_set_clouds_planes_range_device", "mld_tracklets_step_device"]
    buf = tb.store.leaving_buffers([7, 1, 3], device=torch.device("cpu"))
    mark = len(lib.calls)
    tb.step(f, leaving=buf)
    assert [c[0] for c in lib.calls[mark:]] == ["mld_tracks_set_leaving_sink", "mld_set_clouds_planes_range_device",
                                                "mld_tracklets_step_device"]
    assert lib.calls[mark][1][1] == P(buf["ids"]) and lib.calls[mark][1][-1] == buf["record"].data_ptr()


def test_run_projects_hands_over_and_calculates():
    lib, tb = batch()
    other = batch(lib)[1]
    f = tb.prepare(is_new=per([7, 1, 3], U8), **frame_lists())
    tail = tail_of(f, ("u_new", "v_new", "u_old", "v_old", "is_new"))
    tb.run(f)
    assert [c[0] for c in lib.calls] == ["mld_set_clouds_planes_range_device", "mld_tracklets_depths_device"]
    assert_call(lib.calls[0], *projection(f, 0))
    assert_call(lib.calls[1], "mld_tracklets_depths_device", [77, S, 0, 0] + tail)
    mark = len(lib.calls)
    tb.run(f, other, "classify")
    assert [c[0] for c in lib.calls[mark:]] == ["mld_set_clouds_planes_range_device", "orderAfterClassify",
                                                "mld_tracklets_depths_device"]
    assert lib.calls[mark + 1][1] == (tb.est,)
    assert_call(lib.calls[mark + 2], "mld_tracklets_depths_device", [77, S, 1, 1] + tail)
    mark = len(lib.calls)
    tb.run(f, other, restart=[1, 0, 0])
    assert [c[0] for c in lib.calls[mark:]] == ["mld_set_clouds_planes_range_device", "orderAfter",
                                                "mld_tracklets_depths_lanes_device"]
    assert_call(lib.calls[mark + 2], "mld_tracklets_depths_lanes_device", [77, S, 0, [0, 1, 1]] + tail)
    assert tb.bank == 1 and tb._keep == (f, f)


@pytest.mark.parametrize("which", ["semantic_planes", "ransac_planes"])
def test_the_planes_of_a_frame_come_back_in_their_own_columns(which):
    lib, tb = batch()
    fn = f"mld_{which}_estimate_device"
    at = 11 if which == "semantic_planes" else 5
    rec = np.arange(8 * S, dtype=np.int32).reshape(S, 8) + 100

    def fill(args):
        (C.c_int32 * (8 * S)).from_address(args[at])[:] = rec.reshape(-1).tolist()
    lib.peek[fn] = fill
    cl = per([(33, 4), (2, 4), (5, 4)], F32)
    if which == "semantic_planes":
        tb.attach_planes()
        coeffs, masks, status, counts = tb.semantic_planes(cl, images())
    else:
        tb.attach_ransac_planes()
        coeffs, masks, status, counts = tb.ransac_planes(cl, [1, 2, 3])
    names = [c[0] for c in lib.calls[1:]]
    assert names == [fn, "mld_synchronize"] and lib.calls[2][1] == (77,)
    call = lib.calls[1][1]
    assert call[1] == P(cl) and call[-1] == P(masks) and [m.numel() for m in masks] == [2, 1, 1]
    assert all(m.dtype == I32 for m in masks)
    if which == "semantic_planes":
        assert call[9:11] == (4, tb.est.params.ransac_plane_refinement_treshold)
        assert np.array_equal(counts, rec[:, 4:6])
    else:
        assert call[4] == [1, 2, 3]
        assert np.array_equal(counts, rec[:, [7, 4, 5]])
    assert coeffs.dtype == np.float32 and np.array_equal(coeffs.view(np.int32), rec[:, :4])
    assert np.array_equal(status, rec[:, 6]) and counts.flags.c_contiguous and counts.dtype == np.int32


def test_the_batch_calls_clamp_the_capacities_to_the_clouds():
    lib, tb = batch()
    tb.attach_projected_clouds()
    tb.attach_plane_inliers()
    tb.attach_reports()
    mark = len(lib.calls)
    out = tb.projected_clouds(clouds(), depth=True, cam=True, pixel_map=True, capacity=CAPS)
    got = lib.calls[mark][1]
    assert got[2] == [33, 0, 5] and got[4] == [33, 0, 2] and got[5] == out["n_visible"].data_ptr()
    assert [tuple(t.shape) for t in out["uv"]] == [(33, 2), (0, 2), (2, 2)] and [t.numel() for t in out["depth"]] == [33, 0, 2]
    assert [tuple(t.shape) for t in out["cam"]] == [(33, 3), (0, 3), (5, 3)] and tuple(out["pixel_map"][1].shape) == (H, W)
    out = tb.projected_clouds(clouds())
    assert lib.calls[-1][1][4] == [33, 0, 5] and out["depth"] is None and lib.calls[-1][1][8:] == (None, None, None)
    out = tb.plane_inliers(clouds(), per([2, None, 1], I32), lidar=True, capacity=CAPS)
    got = lib.calls[-1][1]
    assert got[5] == [33, 0, 2] and [tuple(t.shape) for t in out["lidar"]] == [(33, 3), (0, 3), (2, 3)] and got[-1] is None
    f = tb.prepare(is_new=per([7, 1, 3], U8), **frame_lists())
    out = tb.reports(f, points=True, capacity=[40, 0, 2])
    got = lib.calls[-1]
    assert got[0] == "mld_depth_reports_collect_tracks_device" and got[1][5:7] == ([7, 1, 3], [7, 0, 2])
    assert got[1][1:5] == (list(f["u_new"]), list(f["v_new"]), list(f["d_cur"]), list(f["t_cur"]))
    assert [tuple(t.shape) for t in out["points"]] == [(7, 3), (0, 3), (2, 3)] and got[1][-1] == P(out["feature"])
    out = tb.reports(f, capacity=[40, 0, 2])
    assert lib.calls[-1][1][6] is None and out["points"] is None and lib.calls[-1][1][-2:] == (None, None)


def test_labels_traces_and_coverage_run_on_the_tables_of_a_frame():
    lib, tb = batch()
    tb.attach_labels()
    tb.attach_traces()
    tb.attach_coverage()
    f = tb.prepare(is_new=per([7, 1, 3], U8), **frame_lists())
    lab = per([7, 1, 3], I16)
    tb.labels(f, images(), (5, 3), lab)
    got = lib.calls[-1]
    assert got[0] == "mld_labels_assign_device" and got[1][7:9] == (list(f["u_new"]), list(f["v_new"])) and got[1][-2:] == (P(lab), None)
    pc = dict(pixel_map=per([(H, W)] * 3, I32), index=per([33, 2, 5], I32), cam=per([(33, 3), (2, 3), (5, 3)], F64))
    with pytest.raises(ValueError):
        tb.traces(f, dict(pc, cam=None))
    with pytest.raises(ValueError):
        tb.coverage(dict(pc, pixel_map=None))
    with pytest.raises(ValueError):
        tb.coverage(pc, maps=("nb", "far"))
    out = tb.traces(f, pc, list_capacity=2)
    got = lib.calls[-1]
    assert got[0] == "mld_feature_traces_collect_tracks_device"
    assert_call(got, got[0], [1, list(f["u_new"]), list(f["v_new"]), [7, 1, 3], P(pc["pixel_map"]), P(pc["index"]), [33, 2, 5],
                              P(pc["cam"]), [33, 2, 5], Floats(COEFFS), list(f["masks"]), 2, P(out["trace"])] +
                [P(out[k]) for k in ("nb", "seg", "road", "road_inl")])
    assert [tuple(t.shape) for t in out["trace"]] == [(7, 23), (1, 23), (3, 23)] and tuple(out["road"][2].shape) == (3, 2)
    out = tb.traces(f, pc, planes=False)
    assert lib.calls[-1][1][9:12] == (None, None, 0) and lib.calls[-1][1][13:] == (None,) * 4 and out["nb"] is None
    out = tb.coverage(pc, COEFFS, per([2, 1, 1], I32), maps=("nb", "reach"), bucket=(4, 2), capacity=[9, 0, 3])
    got = lib.calls[-1][1]
    assert got[8:13] == (P(out["nb"]), None, None, None, P(out["reach"])) and got[13:] == (out["record"].data_ptr(), 4, 2, [4, 0, 3], P(out["buckets"]))
    assert [tuple(t.shape) for t in out["buckets"]] == [(4, 3), (0, 3), (3, 3)] and tuple(out["record"].shape) == (S, 8)
    out = tb.coverage(pc)
    assert lib.calls[-1][1][6:8] == (None, None) and lib.calls[-1][1][14:] == (0, 0, None, None) and out["buckets"] is None
    assert all(out[k] is not None for k in CoverageMaps.MAPS)
