"""The batched coverage maps without a GPU: symbols, the record's layout, the refusals of create before the device is touched,
the Python names, where the source sits, and the restatement the GPU tests compare against - checked against the oracle's
trace of EVERY pixel of a 64 x 64 frame and of a golden frame."""
import collections
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import CameraPinhole, capi, synth

import coverage_restatement as V
import feature_trace_restatement as R
from helpers import make_oracle
from test_golden import load_case

ROOT = Path(__file__).resolve().parent.parent

COVERAGE_SYMBOLS = ("mld_coverage_maps_create", "mld_coverage_maps_destroy", "mld_coverage_maps_last_error",
                    "mld_coverage_maps_collect_device")
# include/mld.h, mld_coverage_record: (field, offset, bytes)
LAYOUT = [("n_reach", 0, 8), ("n_reach_road", 8, 8), ("n_occupied", 16, 8), ("n_inlier", 24, 8), ("n_far", 32, 8),
          ("max_nb", 40, 4), ("flags", 44, 4), ("n_buckets", 48, 4), ("pad_", 52, 12)]

SMALL_CAM = CameraPinhole(64, 64, 64.0, 32.0, 32.0)
SMALL_T = np.eye(4)[:3].copy()


def _transform():
    T = np.ascontiguousarray(np.asarray(synth.T_CAM_LIDAR, dtype=np.float64).reshape(-1)[:12])
    return T, T.ctypes.data_as(C.POINTER(C.c_double))


def kitti():
    return capi.MldCamera(synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_W, synth.KITTI_H)


def test_header_capi_and_both_libraries_carry_the_four_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in COVERAGE_SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_coverage_maps mld_coverage_maps;" in code
    for word in ("112 * n_seq bytes", "24 * WW * H * n_seq bytes", "2 * W * H * n_seq bytes", "16 * 112 * n_seq bytes",
                 "(C0: 14 x 15)", "more than 64 columns or more than 64 rows", "four launches", "no atomics"):
        assert word in header, word
    for name, value in (("MLD_COVERAGE_REACH_MAIN", 1), ("MLD_COVERAGE_REACH_ROAD", 2), ("MLD_COVERAGE_FLAG_BAD_INPUT", 1),
                        ("MLD_COVERAGE_FLAG_HAS_PLANE", 2)):
        assert re.search(rf"\b{name} = {value}\b", code), name
        assert getattr(capi, name) == value


def test_the_record_has_the_size_and_the_offsets_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mld_coverage_record \{(.*?)\} mld_coverage_record;", header, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * int(m.group(2) or 1)))
    offset, laid = 0, []
    for name, size in fields:
        laid.append((name, offset, size))
        offset += size
    assert laid == LAYOUT and offset == 64  # (every field is naturally aligned where it falls: no padding)
    assert C.sizeof(capi.MldCoverageRecord) == 64 and C.alignment(capi.MldCoverageRecord) == 8
    assert [(n, getattr(capi.MldCoverageRecord, n).offset, getattr(capi.MldCoverageRecord, n).size)
            for n, _ in capi.MldCoverageRecord._fields_] == LAYOUT
    assert V.DTYPE.itemsize == 64 and [(n, V.DTYPE.fields[n][1]) for n in V.DTYPE.names] == [(n, o) for n, o, _ in LAYOUT]
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "coverage" / "mld_coverage_maps.hip").read_text()
    assert "static_assert(sizeof(mld_coverage_record) == 64" in source


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "CoverageMaps" in m.__all__
    for name in ("collect", "records", "buckets", "close"):
        assert hasattr(m.CoverageMaps, name), name
    assert m.CoverageMaps.WORDS * 8 == 64 and m.CoverageMaps.MAPS == V.MAPS
    assert hasattr(m.TrackletBatch, "attach_coverage") and hasattr(m.TrackletBatch, "coverage")


@pytest.mark.parametrize("n_seq", [0, -1, 65537])
def test_create_refuses_a_bad_size_before_it_looks_at_the_context(n_seq):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_coverage_maps_create(None, n_seq, None, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_coverage_maps_last_error(None).decode()
    assert "mld_coverage_maps_create" in text and "n_seq" in text and "context" not in text


def _create(ctx, P, cam, Tp):
    lib = capi.load()
    st = C.c_int(0)
    handle = lib.mld_coverage_maps_create(ctx, 4, C.byref(P) if P is not None else None,
                                          C.byref(cam) if cam is not None else None, Tp, C.byref(st))
    assert not handle
    return st.value, lib.mld_coverage_maps_last_error(None).decode()


def test_create_judges_its_arguments_before_it_uses_the_context():
    """Null context, then - behind a context that is not null, of which nothing is dereferenced - null params, camera
    and transform, what mld_create refuses, and the image sizes."""
    P = capi.params_c0()
    cam = kitti()
    T, Tp = _transform()
    assert _create(None, P, cam, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_coverage_maps_create: null context")
    assert not capi.load().mld_coverage_maps_create(None, 65536, None, None, None, None)  # (status_out is optional)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert _create(fake, None, cam, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_coverage_maps_create: null params")
    assert _create(fake, P, None, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_coverage_maps_create: null camera")
    assert _create(fake, P, cam, None) == (capi.MLD_ERR_INVALID_ARG, "mld_coverage_maps_create: null T_cam_lidar")
    for bad, want, word in ((dict(neighbor_search_mode=1), capi.MLD_ERR_UNSUPPORTED_MODE, "neighbor_search_mode"),
                            (dict(do_use_depth_segmentation=1), capi.MLD_ERR_UNSUPPORTED_MODE, "Region growing"),
                            (dict(plane_estimator_use_mestimator=0), capi.MLD_ERR_NO_ROAD_ESTIMATOR, "No road depth estimator"),
                            (dict(plane_estimator_use_mestimator=0, plane_estimator_use_leastsquares=1),
                             capi.MLD_ERR_UNSUPPORTED_MODE, "leastsquares"),
                            (dict(pixelarea_search_witdh=-1), capi.MLD_ERR_INVALID_ARG, "negative search window")):
        code, text = _create(fake, P.replace(**bad), cam, Tp)
        assert code == want and "mld_coverage_maps_create" in text and word in text, bad
    code, text = _create(fake, P, capi.MldCamera(64.0, 1.0, 1.0, 0, 64), Tp)
    assert code == capi.MLD_ERR_INVALID_ARG and "bad image size" in text
    code, text = _create(fake, P, capi.MldCamera(64.0, 1.0, 1.0, 65536, 4), Tp)
    assert code == capi.MLD_ERR_CAPACITY and "65535" in text
    Tbad = T.copy()
    Tbad[5] = np.inf
    code, text = _create(fake, P, cam, Tbad.ctypes.data_as(C.POINTER(C.c_double)))
    assert code == capi.MLD_ERR_INVALID_ARG and "non-finite" in text


@pytest.mark.parametrize("w,h,cam_wh,refused", [(6, 9, (1242, 375), False),      # C0: 14 x 15
                                                 (31, 41, (1242, 375), False),    # 64 x 63: the bound itself (61.5 + 2)
                                                 (31, 42, (1242, 375), True),     # 64 x 65
                                                 (32, 41, (1242, 375), True),     # 66 x 63
                                                 (200, 200, (1242, 375), True),
                                                 (200, 200, (64, 64), False),     # the image bounds the window
                                                 (200, 200, (65, 64), True),
                                                 (200, 200, (64, 65), True)])
def test_create_refuses_a_wide_window_of_more_than_64_columns_or_rows(w, h, cam_wh, refused):
    """min(W, floor(2 halfX2) + 2) <= 64 and min(H, floor(2 halfY2) + 2) <= 64, halfX2 = w * 0.5 * 2.0, halfY2 = h * 0.5 *
    1.5.  A window within the bound gets as far as the context, which is a fake one here: that call is not made."""
    nx = min(cam_wh[0], int(np.floor(2 * (w * 0.5 * 2.0))) + 2)
    ny = min(cam_wh[1], int(np.floor(2 * (h * 0.5 * 1.5))) + 2)
    assert (nx > 64 or ny > 64) == refused
    if not refused:
        return
    P = capi.params_c0().replace(pixelarea_search_witdh=w, pixelarea_search_height=h)
    _, Tp = _transform()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    code, text = _create(fake, P, capi.MldCamera(700.0, 600.0, 180.0, *cam_wh), Tp)
    assert code == capi.MLD_ERR_CAPACITY and "mld_coverage_maps_create" in text and "64 columns" in text


def test_collect_on_no_object_is_refused():
    lib = capi.load()
    assert not lib.mld_coverage_maps_create(None, 0, None, None, None, None)  # (leaves another text behind)
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    rc = lib.mld_coverage_maps_collect_device(None, tab, tab, zero, tab, zero, None, None, None, None, None, None, None, None,
                                              0, 0, None, None)
    assert rc == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_coverage_maps_last_error(None).decode() == "mld_coverage_maps_collect_device: null object (cm)"
    lib.mld_coverage_maps_destroy(None)


def test_the_coverage_maps_are_a_translation_unit_of_their_own():
    """In coverage/, on the shared batch headers and the public header only, linked into both libraries; the depth path's
    sources and the other batch objects do not know of it; three kernels with stable names, no atomics."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "coverage" / "mld_coverage_maps.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h",
                                                           "../batch/mld_depth_path.h", "../../../include/mld.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    code = re.sub(r"//.*", "", text + (csrc / "batch" / "mld_depth_path.h").read_text())  # (the unit and the header its code moved to)
    assert "asm" not in code and "atomic" not in code.lower() and "__threadfence" not in code
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_coverage_classify", "k_coverage_count", "k_coverage_finish"]
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 3  # (+ the descriptor upload: four launches)
    assert "hipMalloc" not in text.split("mld_coverage_maps_collect_device(")[-1]  # (nothing is allocated per call)
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(COVERAGE)" in ln for ln in link_lines)
    assert re.search(r"^COVERAGE\s*:=\s*coverage/mld_coverage_maps\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(TRACES\) \$\(COVERAGE\)", mk, flags=re.M)
    assert "__global__" not in (csrc / "batch" / "mld_batch_device.h").read_text()
    for path in csrc.rglob("*"):
        if path.is_file() and path.name != "Makefile" and path.parent.name != "coverage":
            assert "mld_coverage" not in path.read_text(), path.name


def test_the_window_bounds_are_the_f64_rule_and_not_x_plus_minus_a_constant():
    """C0: the wide half height is 6.75 - 14 rows away from the borders, not 13 or 15 - and the borders clamp."""
    (hx1, hy1), (hx2, hy2) = V.half_sizes(capi.params_c0())
    assert (hx1, hy1, hx2, hy2) == (3.0, 4.5, 6.0, 6.75)
    lo, hi = V.bounds(375, hy2)
    assert (lo[100], hi[100]) == (93, 106) and (lo[0], hi[0]) == (0, 6) and (lo[374], hi[374]) == (367, 374) and (lo[6], hi[6]) == (0, 12)
    lo, hi = V.bounds(1242, hx2)
    assert (lo[100], hi[100]) == (94, 106) and (lo[1241], hi[1241]) == (1235, 1241)
    lo, hi = V.bounds(1, 100.0)
    assert (lo[0], hi[0]) == (0, 0)


def mixed_cloud(seed=3):
    """Dense on the left half of the 64 x 64 image, sparse in the next quarter, empty in the last: pixels with both reach
    bits, with bit 0 only and with neither, and buckets without a pixel."""
    rng = np.random.default_rng(4500 + seed)
    dens = np.where(np.arange(64) < 32, 0.9, np.where(np.arange(64) < 48, 0.05, 0.0))
    ys, xs = np.nonzero(rng.random((64, 64)) < dens[None, :])
    z = np.where(ys < 32, rng.uniform(10.21, 10.45, xs.size), rng.uniform(8.0, 13.0, xs.size))
    return R.pixel_cloud(np.stack([xs, ys], axis=1), z)


def _frames():
    cl = mixed_cloud()
    yield "small", capi.params_c0(), cl, R.small_plane(cl), SMALL_CAM, SMALL_T, (8, 8)
    g = load_case("c0")
    cam = CameraPinhole(g["cam"].width, g["cam"].height, g["cam"].focal_length, g["cam"].principal_point_x, g["cam"].principal_point_y)
    yield "golden_c0", g["P"], g["cloud"], g["plane"], cam, g["T"], (16, 16)


@pytest.mark.parametrize("which", ["small", "golden_c0"])
def test_the_restatement_agrees_with_the_oracles_trace_of_every_pixel(which):
    name, P, cloud, plane, cam, T, bucket = next(f for f in _frames() if f[0] == which)
    ref = make_oracle(P, cam, T)
    ref.set_cloud(cloud)
    ref.set_ground_plane(*plane)
    Tinv, _ = ref.calibration()
    W, H = cam.as_struct().width, cam.as_struct().height
    pm = ref.pixel_map().reshape(H, W)
    bits = np.zeros(cloud.shape[0], dtype=bool)
    bits[np.asarray(plane[1], dtype=np.int64)] = True
    maps, rec, buckets = V.coverage(P, pm, ref.point_index(), np.ascontiguousarray(ref.cloud_camera_cs().T), cloud.shape[0], Tinv,
                                    plane[0], bits, bucket=bucket)
    assert max(maps[k].max() for k in ("nb", "road", "road_inl", "road_far")) < 255  # (nothing saturates here)
    types = collections.Counter()
    whole = 0
    for y in range(H):
        for x in range(W):
            t = ref.trace_feature(float(x), float(y))
            types[t["type"]] += 1
            reach = int(maps["reach"][y, x])
            assert len(t["nb_idx"]) == maps["nb"][y, x], (x, y)
            assert (t["type"] == 2) == (not reach & 1), (x, y)
            if t["type"] == 16:
                assert reach & 2, (x, y)
            if t["reached_road"]:  # the oracle scanned the wide window; it walked all of it unless a neighbour was far
                assert len(t["road_idx"]) == maps["road"][y, x], (x, y)
                if maps["road_far"][y, x] == 0:
                    whole += 1
                    assert len(t["road_pos"]) == maps["road_inl"][y, x], (x, y)
                    assert (len(t["road_pos"]) >= 3) == bool(reach & 2), (x, y)
                else:
                    assert len(t["road_pos"]) == 0 and not reach & 2, (x, y)
    # what the frame must reach
    seen = collections.Counter(maps["reach"].reshape(-1).tolist())
    assert seen[0] and seen[1] and seen[3] and not seen[2]
    assert types[16] >= 20 and types[2] == seen[0] and whole >= 100
    assert rec["n_far"] > 0 and rec["n_inlier"] > 0 and rec["flags"] == V.HAS_PLANE
    assert rec["n_reach"] == seen[1] + seen[3] and rec["n_reach_road"] == seen[3]
    empty = buckets[:, 0] < 0
    assert empty.any() and not empty.all() and (buckets[empty] == (-1, -1, 0)).all()
    bx, by, n = buckets[~empty].T
    assert (maps["nb"][by, bx] == n).all() and (maps["reach"][by, bx] & 1).all() and n.max() == rec["max_nb"]
    # without a plane: no inlier, no far cell, no road bit; the narrow map does not change
    bare, rec0, _ = V.coverage(P, pm, ref.point_index(), np.ascontiguousarray(ref.cloud_camera_cs().T), cloud.shape[0], Tinv)
    assert np.array_equal(bare["nb"], maps["nb"]) and np.array_equal(bare["road"], maps["road"])
    assert not bare["road_inl"].any() and not bare["road_far"].any() and not (bare["reach"] & 2).any()
    assert rec0["flags"] == 0 and rec0["n_inlier"] == 0 and rec0["n_far"] == 0 and rec0["n_buckets"] == 0
