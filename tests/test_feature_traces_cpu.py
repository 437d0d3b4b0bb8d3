"""The batched per-feature traces without a GPU: symbols, the record's layout, the refusals of create before the device is
touched, the Python names, where the source sits, and the restatement the GPU tests compare against - on the golden
frames' stored lists and on the small frames whose list lengths the GPU tests rely on."""
import collections
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import CameraPinhole, capi, synth

import feature_trace_restatement as R
from test_golden import CASES, _ragged, load_case

ROOT = Path(__file__).resolve().parent.parent

TRACE_SYMBOLS = ("mld_feature_traces_create", "mld_feature_traces_destroy", "mld_feature_traces_last_error",
                 "mld_feature_traces_collect_device", "mld_feature_traces_collect_tracks_device")
# include/mld.h, mld_feature_trace: (field, offset, bytes)
LAYOUT = [("main_type", 0, 4), ("road_state", 4, 4), ("n_nb", 8, 4), ("n_seg", 12, 4), ("n_road", 16, 4), ("n_road_inl", 20, 4),
          ("corner_pos", 24, 12), ("corner_vis", 36, 12), ("flags", 48, 4), ("pad_", 52, 4), ("main_depth", 56, 8),
          ("hist_lower", 64, 8), ("hist_higher", 72, 8), ("plane_n", 80, 24), ("plane_offset", 104, 8), ("corners", 112, 72)]

SMALL_CAM = CameraPinhole(64, 64, 64.0, 32.0, 32.0)
SMALL_T = np.eye(4)[:3].copy()


def _transform():
    T = np.ascontiguousarray(np.asarray(synth.T_CAM_LIDAR, dtype=np.float64).reshape(-1)[:12])
    return T, T.ctypes.data_as(C.POINTER(C.c_double))


def test_header_capi_and_both_libraries_carry_the_five_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in TRACE_SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_feature_traces mld_feature_traces;" in code
    for word in ("120 * n_seq bytes", "16 * 120 * n_seq bytes", "It cannot occur", "(C0: 14 x 15 = 210)",
                 "nothing behind them is\n *                       touched", "MLD_TRACE_FLAG_BAD_INPUT on the features"):
        assert word in header, word
    for name, value in (("MLD_TRACE_ROAD_NOT_REACHED", 0), ("MLD_TRACE_ROAD_FEW_NEIGHBOURS", 1), ("MLD_TRACE_ROAD_FAR_NEIGHBOUR", 2),
                        ("MLD_TRACE_ROAD_FEW_INLIERS", 3), ("MLD_TRACE_ROAD_FIT", 4), ("MLD_TRACE_FLAG_BAD_INPUT", 1),
                        ("MLD_TRACE_FLAG_NONFINITE_FEATURE", 2)):
        assert re.search(rf"\b{name} = {value}\b", code), name
        assert getattr(capi, name) == value


def test_the_record_has_the_size_and_the_offsets_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mld_feature_trace \{(.*?)\} mld_feature_trace;", header, flags=re.S).group(1)
    # the header's fields in order, with their element counts
    fields = []
    for kind, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * int(m.group(2) or 1)))
    offset, laid = 0, []
    for name, size in fields:
        laid.append((name, offset, size))
        offset += size
    assert laid == LAYOUT and offset == 184  # (every field is naturally aligned where it falls: no padding)
    assert C.sizeof(capi.MldFeatureTrace) == 184 and C.alignment(capi.MldFeatureTrace) == 8
    assert [(n, getattr(capi.MldFeatureTrace, n).offset, getattr(capi.MldFeatureTrace, n).size)
            for n, _ in capi.MldFeatureTrace._fields_] == LAYOUT
    assert R.DTYPE.itemsize == 184 and [(n, R.DTYPE.fields[n][1]) for n in R.DTYPE.names] == [(n, o) for n, o, _ in LAYOUT]
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "traces" / "mld_feature_traces.hip").read_text()
    assert "static_assert(sizeof(mld_feature_trace) == 184" in source


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "FeatureTraces" in m.__all__
    for name in ("collect", "collect_tracks", "records", "close"):
        assert hasattr(m.FeatureTraces, name), name
    assert m.FeatureTraces.WORDS * 8 == 184
    assert hasattr(m.TrackletBatch, "attach_traces") and hasattr(m.TrackletBatch, "traces")


@pytest.mark.parametrize("n_seq,max_features,word", [(0, 100, "n_seq"), (-1, 100, "n_seq"), (65537, 100, "n_seq"),
                                                     (4, 0, "max_features"), (4, -5, "max_features"),
                                                     (4, 16777217, "max_features")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_features, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_feature_traces_create(None, n_seq, max_features, None, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_feature_traces_last_error(None).decode()
    assert "mld_feature_traces_create" in text and word in text and "context" not in text


def _create(ctx, P, cam, Tp):
    lib = capi.load()
    st = C.c_int(0)
    handle = lib.mld_feature_traces_create(ctx, 4, 1000, C.byref(P) if P is not None else None,
                                           C.byref(cam) if cam is not None else None, Tp, C.byref(st))
    assert not handle
    return st.value, lib.mld_feature_traces_last_error(None).decode()


def test_create_judges_its_arguments_before_it_uses_the_context():
    """Null context, then - behind a context that is not null, of which nothing is dereferenced - null params, camera
    and transform, PCA, what mld_create refuses, and the bound on the wide window."""
    P = capi.params_c0()
    cam = synth_camera()
    T, Tp = _transform()
    assert _create(None, P, cam, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_feature_traces_create: null context")
    assert not capi.load().mld_feature_traces_create(None, 65536, 16777216, None, None, None, None)  # (status_out is optional)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert _create(fake, None, cam, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_feature_traces_create: null params")
    assert _create(fake, P, None, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_feature_traces_create: null camera")
    assert _create(fake, P, cam, None) == (capi.MLD_ERR_INVALID_ARG, "mld_feature_traces_create: null T_cam_lidar")
    code, text = _create(fake, P.replace(do_use_PCA=1), cam, Tp)
    assert code == capi.MLD_ERR_UNSUPPORTED_MODE and "mld_feature_traces_create" in text and "do_use_PCA" in text
    for bad, want, word in ((dict(neighbor_search_mode=1), capi.MLD_ERR_UNSUPPORTED_MODE, "neighbor_search_mode"),
                            (dict(do_use_depth_segmentation=1), capi.MLD_ERR_UNSUPPORTED_MODE, "Region growing"),
                            (dict(plane_estimator_use_mestimator=0), capi.MLD_ERR_NO_ROAD_ESTIMATOR, "No road depth estimator"),
                            (dict(plane_estimator_use_mestimator=0, plane_estimator_use_leastsquares=1),
                             capi.MLD_ERR_UNSUPPORTED_MODE, "leastsquares"),
                            (dict(pixelarea_search_witdh=-1), capi.MLD_ERR_INVALID_ARG, "negative search window")):
        code, text = _create(fake, P.replace(**bad), cam, Tp)
        assert code == want and "mld_feature_traces_create" in text and word in text, bad
    code, text = _create(fake, P, capi.MldCamera(0.0, 1.0, 1.0, 64, 64), Tp)
    assert code == capi.MLD_ERR_INVALID_ARG and "bad camera intrinsics" in text
    code, text = _create(fake, P, capi.MldCamera(64.0, 1.0, 1.0, 0, 64), Tp)
    assert code == capi.MLD_ERR_INVALID_ARG and "bad image size" in text
    Tbad = T.copy()
    Tbad[5] = np.inf
    code, text = _create(fake, P, cam, Tbad.ctypes.data_as(C.POINTER(C.c_double)))
    assert code == capi.MLD_ERR_INVALID_ARG and "non-finite" in text


@pytest.mark.parametrize("w,h,cam_wh,refused", [(6, 9, (1242, 375), False),       # C0: 14 x 15 = 210
                                                 (15, 20, (1242, 375), False),     # 32 x 32 = 1024: the bound itself
                                                 (15, 21, (1242, 375), True),      # 32 x 33
                                                 (16, 20, (1242, 375), True),      # 34 x 32
                                                 (200, 200, (1242, 375), True),
                                                 (200, 200, (32, 32), False),      # the image bounds the window: 32 x 32
                                                 (200, 200, (33, 32), True)])
def test_create_refuses_a_wide_window_of_more_than_1024_cells(w, h, cam_wh, refused):
    """min(W, floor(2 halfX2) + 2) * min(H, floor(2 halfY2) + 2) <= 1024, halfX2 = w * 0.5 * 2.0, halfY2 = h * 0.5 * 1.5.
    A window within the bound gets as far as the context, which is a fake one here: that call is not made."""
    nx = min(cam_wh[0], int(np.floor(2 * (w * 0.5 * 2.0))) + 2)
    ny = min(cam_wh[1], int(np.floor(2 * (h * 0.5 * 1.5))) + 2)
    assert (nx * ny > 1024) == refused
    if not refused:
        return
    P = capi.params_c0().replace(pixelarea_search_witdh=w, pixelarea_search_height=h)
    _, Tp = _transform()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    code, text = _create(fake, P, capi.MldCamera(700.0, 600.0, 180.0, *cam_wh), Tp)
    assert code == capi.MLD_ERR_CAPACITY and "mld_feature_traces_create" in text and "1024 cells" in text


def synth_camera():
    return capi.MldCamera(synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_W, synth.KITTI_H)


@pytest.mark.parametrize("tracks", [False, True])
def test_collect_on_no_object_is_refused(tracks):
    lib = capi.load()
    assert not lib.mld_feature_traces_create(None, 0, 1, None, None, None, None)  # (leaves another text behind)
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    tail = (zero, tab, tab, zero, tab, zero, None, None, 0, tab, None, None, None, None)
    if tracks:
        rc = lib.mld_feature_traces_collect_tracks_device(None, tab, tab, *tail)
    else:
        rc = lib.mld_feature_traces_collect_device(None, tab, *tail)
    assert rc == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_feature_traces_last_error(None).decode()
    fn = "mld_feature_traces_collect_tracks_device" if tracks else "mld_feature_traces_collect_device"
    assert text == fn + ": null object (ft)"
    lib.mld_feature_traces_destroy(None)


def test_the_traces_are_a_translation_unit_of_their_own():
    """In traces/, on the shared batch header and the public header only, linked into both libraries; the depth path's
    sources do not know of it; one kernel with a stable name."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "traces" / "mld_feature_traces.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h",
                                                           "../batch/mld_depth_path.h", "../../../include/mld.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    assert "asm" not in re.sub(r"//.*", "", text + (csrc / "batch" / "mld_depth_path.h").read_text())
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_feature_trace"]
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(TRACES)" in ln for ln in link_lines)
    assert re.search(r"^TRACES\s*:=\s*traces/mld_feature_traces\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(INLIERS\) \$\(TRACES\)", mk, flags=re.M)
    assert "mld_feature_traces" in (csrc / "batch" / "mld_batch_object.h").read_text()
    for path in csrc.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert "mld_feature_traces" not in path.read_text(), path.name


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_golden_lists(name):
    """The per-feature lists stored with the golden frames, the stored result types, and what a record says about them."""
    g = load_case(name)
    cam = CameraPinhole(g["cam"].width, g["cam"].height, g["cam"].focal_length, g["cam"].principal_point_x,
                        g["cam"].principal_point_y)
    fr = R.Restatement(g["P"], g["cloud"], g["plane"], cam, g["T"])
    assert np.array_equal(fr.index, g["point_index"]) and np.array_equal(fr.pixel_map, g["pixel_map"])
    rec, lists, (types, depths) = fr.trace(g["uv"])
    assert np.array_equal(types, g["type"]) and np.array_equal(depths, g["depth"], equal_nan=True)
    for i in range(len(g["uv"])):
        for mine, theirs in (("nb", "nb_idx"), ("seg", "seg_pos"), ("road", "road_idx"), ("road_inl", "road_pos")):
            assert lists[i][mine].tolist() == _ragged(g, theirs, i), (i, mine)
        r = rec[i]
        assert (r["n_nb"], r["n_seg"], r["n_road"], r["n_road_inl"]) == tuple(len(lists[i][k]) for k in R.LISTS)
        if g["corners"][i][0] >= 0:
            assert r["corner_pos"].tolist() == g["corners"][i].tolist()
        # what the record implies about the product's answer
        if r["road_state"] == R.FIT:
            assert types[i] in (16, 4, 5, 6, 7)
        else:
            assert types[i] == r["main_type"]
            assert depths[i] == r["main_depth"] or (r["road_state"] != R.NOT_REACHED and depths[i] == -1.0)
        assert (r["main_depth"] != -1.0) == (r["main_type"] == 1) or r["main_depth"] == -1.0
        assert np.isnan(r["corners"]).all() == (r["corner_pos"][0] < 0)
        assert np.isnan(r["plane_n"]).all() == (r["corner_pos"][0] < 0 or r["main_type"] == 8)
    if g["plane"] is None:
        assert (rec["road_state"] == R.NOT_REACHED).all() and (rec["n_road"] == 0).all()


def test_the_far_test_is_the_oracles():
    """FAR_NEIGHBOUR against FEW_INLIERS rests on the NumPy restatement of the f32 distance: where the oracle's trace
    keeps inliers no neighbour may be far, and with a threshold nothing passes every reached feature is FAR_NEIGHBOUR."""
    g = load_case("c0")
    cam = CameraPinhole(g["cam"].width, g["cam"].height, g["cam"].focal_length, g["cam"].principal_point_x,
                        g["cam"].principal_point_y)
    rec, lists, _ = R.Restatement(g["P"], g["cloud"], g["plane"], cam, g["T"]).trace(g["uv"])
    kept = rec["n_road_inl"] > 0
    assert kept.any() and np.isin(rec["road_state"][kept], (R.FEW_INLIERS, R.FIT)).all()
    tight = g["P"].replace(ransac_plane_point_distance_treshold=-1.0)
    rec2, _, _ = R.Restatement(tight, g["cloud"], g["plane"], cam, g["T"]).trace(g["uv"])
    reached = rec2["road_state"] != R.NOT_REACHED
    assert reached.any() and (rec2["road_state"][reached] == R.FAR_NEIGHBOUR).all() and (rec2["n_road_inl"] == 0).all()


def test_the_small_frames_reach_what_the_gpu_tests_rely_on():
    """Asserted on the ORACLE's trace: the sparse cloud gives neighbour counts 0, 1, 2 and 3; the dense one with an 8 x 8
    search area narrow lists of 63, 64, 65 and more entries (a ballot and its successor), wide lists beyond 128, and
    features whose segmented list has 65 or more entries with corners found; both meet every special feature."""
    P = capi.params_c0()
    uv = R.small_features(257)
    assert (~np.isfinite(uv).all(axis=1)).sum() == 4 and ((uv < 0) | (uv > 64)).any()
    cloud = R.sparse_cloud()
    rec, _, _ = R.Restatement(P, cloud, R.small_plane(cloud), SMALL_CAM, SMALL_T).trace(uv)
    assert {0, 1, 2, 3} <= set(rec["n_nb"].tolist())
    assert len(set(rec["main_type"].tolist())) >= 4 and len(set(rec["road_state"].tolist())) >= 3
    assert (rec["flags"] == R.NONFINITE).sum() == 4
    P8 = P.replace(pixelarea_search_witdh=8, pixelarea_search_height=8)
    cloud = R.dense_cloud()
    rec, _, _ = R.Restatement(P8, cloud, R.small_plane(cloud), SMALL_CAM, SMALL_T).trace(R.dense_features())
    counts = collections.Counter(rec["n_nb"].tolist())
    assert counts[63] and counts[64] and counts[65] and max(counts) > 65
    assert rec["n_road"].max() > 128
    assert ((rec["n_seg"] >= 65) & (rec["corner_pos"][:, 0] >= 0)).sum() >= 1
    assert {R.NOT_REACHED, R.FAR_NEIGHBOUR, R.FIT} <= set(rec["road_state"].tolist())
