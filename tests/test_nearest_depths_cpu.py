"""The batched nearest-return depths without a GPU: symbols, the record's layout, the Python names, where the source sits,
the refusals of create before the device is touched, and the restatement the GPU tests compare against:
  main_path     on the WINDOW's own list it must be OracleDepthEstimator.calculate_depth (types identical, depths bit for
                bit), so that afterwards only the list differs
  nearest_list  against a brute force that sorts ALL cells of the image by (d2, y, x)"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi, synth

import nearest_depth_restatement as N
from helpers import make_oracle
from test_golden import CASES, load_case

ROOT = Path(__file__).resolve().parent.parent

SYMBOLS = ("mld_nearest_depths_create", "mld_nearest_depths_destroy", "mld_nearest_depths_last_error",
           "mld_nearest_depths_collect_device", "mld_nearest_depths_collect_tracks_device")
# include/mld.h, mld_nearest_depth: (field, offset, bytes)
LAYOUT = [("type", 0, 4), ("n_in_radius", 4, 4), ("n_nb", 8, 4), ("n_seg", 12, 4), ("d2_first", 16, 4), ("d2_last", 20, 4),
          ("nearest_orig", 24, 4), ("flags", 28, 4), ("depth", 32, 8), ("nearest_z", 40, 8), ("corner_vis", 48, 12), ("pad_", 60, 4)]
RADII = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
COUNTS = (1, 2, 3, 63, 64, 65, 255, 256)


def test_header_capi_and_both_libraries_carry_the_five_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_nearest_depths mld_nearest_depths;" in code
    for name, value in (("MLD_NEAREST_MAX_RADIUS", 64), ("MLD_NEAREST_MAX_COUNT", 256)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
        assert getattr(capi, name) == value
    for name, value in (("MLD_NEAREST_FLAG_BAD_INPUT", 1), ("MLD_NEAREST_FLAG_NONFINITE_FEATURE", 2)):
        assert re.search(rf"\b{name} = {value}\b", code), name
        assert getattr(capi, name) == value
    # the two differences from the reference's finder are said where a user reads them
    for text in (header, (ROOT / "INTEGRATION.md").read_text()):
        assert "neighbor_search_mode" in text and "one return per pixel" in text.lower() and "exact" in text.lower()


def test_the_record_has_the_size_and_the_offsets_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mld_nearest_depth \{(.*?)\} mld_nearest_depth;", header, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * int(m.group(2) or 1)))
    offset, laid = 0, []
    for name, size in fields:
        laid.append((name, offset, size))
        offset += size
    assert laid == LAYOUT and offset == 64  # (every field is naturally aligned where it falls: no padding)
    assert C.sizeof(capi.MldNearestDepth) == 64 and C.alignment(capi.MldNearestDepth) == 8
    assert [(n, getattr(capi.MldNearestDepth, n).offset, getattr(capi.MldNearestDepth, n).size)
            for n, _ in capi.MldNearestDepth._fields_] == LAYOUT
    assert N.DTYPE.itemsize == 64 and [(n, N.DTYPE.fields[n][1]) for n in N.DTYPE.names] == [(n, o) for n, o, _ in LAYOUT]
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "nearest" / "mld_nearest_depths.hip").read_text()
    assert "static_assert(sizeof(mld_nearest_depth) == 64" in source


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "NearestDepths" in m.__all__
    for name in ("collect", "collect_tracks", "records", "close"):
        assert hasattr(m.NearestDepths, name), name
    assert m.NearestDepths.WORDS == 8 and m.NearestDepths.DTYPE.itemsize == 64
    assert (m.NearestDepths.MAX_RADIUS, m.NearestDepths.MAX_COUNT) == (64, 256)
    assert hasattr(m.TrackletBatch, "attach_nearest_depths") and hasattr(m.TrackletBatch, "nearest_depths")
    rows = [(attr, row) for attr, row in m.TrackletBatch._ATTACHABLE.items() if row[0] is m.NearestDepths]
    assert len(rows) == 1 and rows[0][1][1] == "attach_nearest_depths"


def test_the_nearest_depths_are_a_translation_unit_of_their_own():
    """In nearest/, on the shared batch headers and the public header only, linked into both libraries; the depth path's
    sources do not know of it; one kernel with a stable name; no inline assembly."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "nearest" / "mld_nearest_depths.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h",
                                                           "../batch/mld_depth_path.h", "../../../include/mld.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    assert "asm" not in re.sub(r"//.*", "", text)
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_nearest_depths"]
    assert "main_path(" in text and re.search(r"\bMainPath main_path\(", (csrc / "batch" / "mld_depth_path.h").read_text())
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(NEAREST)" in ln for ln in link_lines)
    assert re.search(r"^NEAREST\s*:=\s*nearest/mld_nearest_depths\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(NEAREST\)", mk, flags=re.M)
    for path in csrc.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert "mld_nearest_depths" not in path.read_text(), path.name


def synth_camera():
    return capi.MldCamera(synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_W, synth.KITTI_H)


@pytest.mark.parametrize("n_seq,max_features,radius,count,word", [
    (0, 100, 10, 10, "n_seq"), (65537, 100, 10, 10, "n_seq"), (4, 0, 10, 10, "max_features"), (4, 16777217, 10, 10, "max_features"),
    (4, 100, 0, 10, "radius"), (4, 100, -1, 10, "radius"), (4, 100, 65, 10, "radius"),
    (4, 100, 10, 0, "count"), (4, 100, 10, -3, "count"), (4, 100, 10, 257, "count")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_features, radius, count, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_nearest_depths_create(None, n_seq, max_features, radius, count, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_nearest_depths_last_error(None).decode()
    assert "mld_nearest_depths_create" in text and word in text and "context" not in text


def _create(ctx, P, cam, radius=10, count=10):
    lib = capi.load()
    st = C.c_int(0)
    handle = lib.mld_nearest_depths_create(ctx, 4, 1000, radius, count, C.byref(P) if P is not None else None,
                                           C.byref(cam) if cam is not None else None, C.byref(st))
    assert not handle
    return st.value, lib.mld_nearest_depths_last_error(None).decode()


def test_create_judges_its_arguments_before_it_uses_the_context():
    """Null context, then - behind a context that is not null, of which nothing is dereferenced - null params and camera,
    PCA, all depths zero, and what mld_create refuses of a parameter set and a camera, with its texts."""
    P = capi.params_c0()
    cam = synth_camera()
    assert _create(None, P, cam) == (capi.MLD_ERR_INVALID_ARG, "mld_nearest_depths_create: null context")
    assert not capi.load().mld_nearest_depths_create(None, 65536, 16777216, 64, 256, None, None, None)  # (status_out is optional)
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert _create(fake, None, cam) == (capi.MLD_ERR_INVALID_ARG, "mld_nearest_depths_create: null params")
    assert _create(fake, P, None) == (capi.MLD_ERR_INVALID_ARG, "mld_nearest_depths_create: null camera")
    for bad, want, word in ((dict(do_use_PCA=1), capi.MLD_ERR_UNSUPPORTED_MODE, "do_use_PCA"),
                            (dict(set_all_depths_to_zero=1), capi.MLD_ERR_UNSUPPORTED_MODE, "set_all_depths_to_zero"),
                            (dict(neighbor_search_mode=1), capi.MLD_ERR_UNSUPPORTED_MODE,
                             "neighbor_search_mode has the invalid value: 1"),
                            (dict(do_use_depth_segmentation=1), capi.MLD_ERR_UNSUPPORTED_MODE,
                             "DepthEstimator: Region growing not supported!"),
                            (dict(plane_estimator_use_mestimator=0), capi.MLD_ERR_NO_ROAD_ESTIMATOR, "No road depth estimator selected."),
                            (dict(plane_estimator_use_mestimator=0, plane_estimator_use_leastsquares=1),
                             capi.MLD_ERR_UNSUPPORTED_MODE, "leastsquares"),
                            (dict(pixelarea_search_witdh=-1), capi.MLD_ERR_INVALID_ARG, "negative search window")):
        code, text = _create(fake, P.replace(**bad), cam)
        assert code == want and text.startswith("mld_nearest_depths_create: ") and word in text, bad
    code, text = _create(fake, P, capi.MldCamera(0.0, 1.0, 1.0, 64, 64))
    assert code == capi.MLD_ERR_INVALID_ARG and "bad camera intrinsics" in text
    code, text = _create(fake, P, capi.MldCamera(64.0, 1.0, 1.0, 0, 64))
    assert code == capi.MLD_ERR_INVALID_ARG and "bad image size" in text
    code, text = _create(fake, P, capi.MldCamera(64.0, 1.0, 1.0, 65536, 4))
    assert code == capi.MLD_ERR_CAPACITY and "65535" in text
    # the sizes come first: a bad radius is named although the parameters are bad as well
    code, text = _create(fake, P.replace(do_use_PCA=1), cam, radius=65)
    assert code == capi.MLD_ERR_INVALID_ARG and "radius" in text


@pytest.mark.parametrize("tracks", [False, True])
def test_collect_on_no_object_is_refused(tracks):
    lib = capi.load()
    assert not lib.mld_nearest_depths_create(None, 0, 1, 1, 1, None, None, None)  # (leaves another text behind)
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    tail = (zero, tab, tab, zero, tab, zero, 0, tab, None)
    if tracks:
        rc = lib.mld_nearest_depths_collect_tracks_device(None, tab, tab, *tail)
    else:
        rc = lib.mld_nearest_depths_collect_device(None, tab, *tail)
    assert rc == capi.MLD_ERR_INVALID_ARG
    fn = "mld_nearest_depths_collect_tracks_device" if tracks else "mld_nearest_depths_collect_device"
    assert lib.mld_nearest_depths_last_error(None).decode() == fn + ": null object (nd)"
    lib.mld_nearest_depths_destroy(None)


# ---- main_path is the oracle's main path --------------------------------------------------------------------------------

def _main_path_against_the_oracle(P, cam, T, cloud, uv):
    """main_path on the window's own list (trace_feature's nb_idx) against calculate_depth, road off: the number of features
    and the types seen."""
    ref = make_oracle(P, cam, T)
    ref.set_cloud(cloud)
    ref.set_ground_plane(None, None)
    depth, types = ref.calculate_depth(uv)
    cam_pts = np.ascontiguousarray(ref.cloud_camera_cs().T)
    index = ref.point_index()
    wrong = []
    for i, (u, v) in enumerate(np.asarray(uv, dtype=np.float64)):
        nb = ref.trace_feature(float(u), float(v))["nb_idx"]
        mp = N.main_path(ref, P, u, v, cam_pts[index[nb]])
        if mp["type"] != types[i] or np.float64(mp["depth"]).view(np.int64) != depth[i].view(np.int64):
            wrong.append((i, mp["type"], int(types[i]), mp["depth"], float(depth[i])))
    assert not wrong, wrong[:5]
    return set(types.tolist())


@pytest.mark.parametrize("name", CASES)
def test_main_path_is_the_oracle_on_the_golden_cases_with_the_road_off(name):
    from mono_lidar_depth_amd import CameraPinhole
    g = load_case(name)
    c = g["cam"]
    cam = CameraPinhole(c.width, c.height, c.focal_length, c.principal_point_x, c.principal_point_y)
    _main_path_against_the_oracle(g["P"], cam, g["T"], g["cloud"], g["uv"])


@pytest.mark.parametrize("scanner,variant", [("HDL64", dict()), ("VLP16", dict()),
                                             ("HDL64", dict(treshold_depth_mode=1, treshold_depth_local_mode=1)),
                                             ("HDL64", dict(do_use_histogram_segmentation=0, do_use_triangle_size_maximation=0))])
def test_main_path_is_the_oracle_on_synthetic_frames(scanner, variant):
    """At least 400 features on an HDL-64 and a VLP-16 frame, half of them near returns so that the path runs to its end."""
    P = capi.params_c0().replace(**variant)
    cloud = synth.make_cloud(getattr(synth, scanner), seed=3, frame=0)
    uv = np.concatenate([synth.make_features(220, seed=3), synth.make_features_near_points(cloud, 220, seed=4)])
    assert uv.shape[0] >= 400
    seen = _main_path_against_the_oracle(P, None, None, cloud, uv)
    if not variant:
        assert 2 in seen and (scanner == "VLP16" or 1 in seen)


def test_the_threshold_codes_map_to_the_result_types():
    """threshold_global / threshold_local return 1 below the minimum and 2 above the maximum: types 5 / 4 and 7 / 6."""
    from oracle import oracle
    P = capi.params_c0().replace(treshold_depth_mode=0, treshold_depth_local_mode=0)
    assert oracle.threshold_global(P, float(P.treshold_depth_min) - 1.0)[0] == 1 and N.GLOBAL_TYPE[1] == 5
    assert oracle.threshold_global(P, float(P.treshold_depth_max) + 1.0)[0] == 2 and N.GLOBAL_TYPE[2] == 4
    pts = np.array([[0.0, 0.0, 10.0], [1.0, 0.0, 10.5], [0.0, 1.0, 11.0]])
    assert oracle.threshold_local(P, pts, -1e6)[0] == 1 and N.LOCAL_TYPE[1] == 7
    assert oracle.threshold_local(P, pts, 1e6)[0] == 2 and N.LOCAL_TYPE[2] == 6
    assert [capi.RESULT_TYPE_NAMES[t] for t in (4, 5, 6, 7)] == ["TresholdDepthGlobalGreaterMax", "TresholdDepthGlobalSmallerMin",
                                                                  "TresholdDepthLocalGreaterMax", "TresholdDepthLocalSmallerMin"]


# ---- nearest_list is the rule -------------------------------------------------------------------------------------------

def brute_force(pm, index, index_len, n_points, u, v, R, k):
    """Every cell of the image sorted by (d2, y, x), one at a time."""
    H, W = pm.shape
    cx, cy = N.centre_cell(u, v, W, H, R)
    cells = sorted(((x - cx) ** 2 + (y - cy) ** 2, y, x) for y in range(H) for x in range(W))
    vis, d2s, bad = [], [], False
    for d2, y, x in cells:
        if d2 > R * R:
            break
        m = int(pm[y, x])
        if m == -1:
            continue
        if not (0 <= m < index_len and 0 <= int(index[m]) < n_points):
            bad = True
            continue
        vis.append(m)
        d2s.append(d2)
    return vis[:k], d2s[:k], len(vis), (N.BAD_INPUT if bad else 0)


def random_map(seed, W=40, H=30, density=0.3, spoil=0):
    rng = np.random.default_rng(7700 + seed)
    ys, xs = np.nonzero(rng.random((H, W)) < density)
    n_vis = xs.size
    pm = np.full((H, W), -1, dtype=np.int32)
    pm[ys, xs] = rng.permutation(n_vis)
    n_points = n_vis + 5
    index = rng.permutation(n_points)[:n_vis].astype(np.int32)
    for _ in range(spoil):  # map values and index values outside their arrays
        y, x = rng.integers(0, H), rng.integers(0, W)
        pm[y, x] = rng.choice([-2, n_vis, n_vis + 100, -(2 ** 31)])
        if n_vis:
            index[rng.integers(0, n_vis)] = rng.choice([-1, n_points, 2 ** 31 - 1])
    return pm, index, n_vis, n_points


@pytest.mark.parametrize("R", RADII)
def test_nearest_list_equals_the_brute_force(R):
    W, H = 40, 30
    centres = [(0.0, 0.0), (W - 1.0, H - 1.0), (-3.0, 2.0), (W - 1.0 + R, 5.0), (float(W + R), 5.0), (-0.5, 7.25), (1e300, 3.0),
               (-1e300, -1e300), (19.5, 14.5), (20.0, -float(R)), (7.9, H + R - 0.5)]
    for seed, (density, spoil) in enumerate(((0.3, 0), (1.0, 0), (0.03, 0), (0.4, 12))):
        pm, index, index_len, n_points = random_map(seed, W, H, density, spoil)
        rng = np.random.default_rng(seed)
        feats = centres + [(rng.uniform(-2, W + 2), rng.uniform(-2, H + 2)) for _ in range(3)]
        for k in COUNTS:
            for u, v in feats:
                vis, d2, n_in, flags = N.nearest_list(pm, index, index_len, n_points, u, v, R, k)
                want = brute_force(pm, index, index_len, n_points, u, v, R, k)
                assert (vis.tolist(), d2.tolist(), n_in, flags) == want, (seed, R, k, u, v)
    for bad in (np.nan, np.inf, -np.inf):
        assert N.nearest_list(pm, index, index_len, n_points, bad, 3.0, R, 4)[2:] == (0, N.NONFINITE)
        assert N.nearest_list(pm, index, index_len, n_points, 3.0, bad, R, 4)[0].size == 0


def test_the_corner_trap_and_the_tie_order():
    """(3, 3) from the centre, d2 18, lies in the first square and is farther than (4, 0), d2 16, of the next one; the twelve
    cells with d2 25 come in (y, x) order and a list may end inside them."""
    pm = np.full((11, 11), -1, dtype=np.int32)
    pm[8, 8], pm[5, 9] = 0, 1
    index = np.arange(2, dtype=np.int32)
    assert N.nearest_list(pm, index, 2, 2, 5.0, 5.0, 5, 1)[0].tolist() == [1]
    assert N.nearest_list(pm, index, 2, 2, 5.0, 5.0, 5, 2)[0].tolist() == [1, 0]
    ring = [(dx, dy) for dy in range(-5, 6) for dx in range(-5, 6) if dx * dx + dy * dy == 25]
    assert len(ring) == 12
    pm[:] = -1
    for i, (dx, dy) in enumerate(reversed(ring)):
        pm[5 + dy, 5 + dx] = i
    index = np.arange(12, dtype=np.int32)
    assert N.nearest_list(pm, index, 12, 12, 5.0, 5.0, 5, 12)[0].tolist() == list(range(11, -1, -1))
    assert N.nearest_list(pm, index, 12, 12, 5.0, 5.0, 5, 5)[0].tolist() == [11, 10, 9, 8, 7]
    assert N.nearest_list(pm, index, 12, 12, 5.0, 5.0, 4, 12)[2] == 0
