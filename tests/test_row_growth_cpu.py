"""The batched row growth without a GPU: symbols, the layouts, the Python names, where the source sits, the refusals of
create before the device is touched, and the restatement the GPU tests compare against:
  the reference's own test case (test_monolidar_fusion.cpp:173-275, LidarSegmenter.test1) with the indices its loops give
  tail          on the WINDOW's own list it must be OracleDepthEstimator.calculate_depth with the count test and the
                histogram off (types identical, depths bit for bit)
  window_list   against the oracle's neighbour list
  the quirks    one hand-made scene per quirk on which the literal rule and the repaired rule differ
The scenes and the generator of the randomised sweep are shared with test_row_growth_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import CameraPinhole, capi, synth

import row_growth_restatement as RG
from helpers import make_oracle

ROOT = Path(__file__).resolve().parent.parent

SYMBOLS = ("mld_row_growth_params_default", "mld_row_growth_params_yaml", "mld_row_growth_create", "mld_row_growth_destroy",
           "mld_row_growth_last_error", "mld_row_growth_segment_device", "mld_row_growth_collect_device",
           "mld_row_growth_collect_tracks_device")
# include/mld.h, mld_row_growth: (field, offset, bytes)
LAYOUT = [("type", 0, 4), ("state", 4, 4), ("grown_type", 8, 4), ("flags", 12, 4), ("n_nb", 16, 4), ("seed_vis", 20, 4),
          ("second_vis", 24, 4), ("seed_row", 28, 4), ("second_row", 32, 4), ("n_first", 36, 4), ("n_grown", 40, 4),
          ("corner_vis", 44, 12), ("depth", 56, 8), ("seed_z", 64, 8)]
PARAM_NAMES = ["depth_segmentation_max_treshold_gradient", "depth_segmentation_max_neighbor_distance",
               "depth_segmentation_max_neighbor_distance_gradient", "depth_segmentation_max_neighbor_to_seedpoint_distance",
               "depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient",
               "depth_segmentation_max_seedpoint_to_seedpoint_distance",
               "depth_segmentation_max_neighbor_to_seedpoint_distance_gradient", "depth_segmentation_max_pointcount"]
IDENTITY = np.eye(4)[:3].copy()


# ---- scenes: hand-made visible lists, shared with the GPU tests ------------------------------------------------------------

SCENE_W, SCENE_H, SCENE_F = 256, 48, 64.0
SCENE_CAM = (SCENE_W, SCENE_H, SCENE_F, 128.0, 24.0)  # CameraPinhole(width, height, focal length, principal point)
GENEROUS = RG.growth(0, 5, 0, 5, 0, 2, 0, -1)         # the values of the reference's own test


def scene_params(**kw):
    """C0 with a search window of 3 x 3 cells and one neighbour enough, the road off."""
    return capi.params_c0().replace(pixelarea_search_witdh=2, pixelarea_search_height=2, radiusSearch_count_min=1,
                                    do_use_ransac_plane=0, **kw)


def line(u0, du, n, v, x0=0.0, dx=0.5, y=0.0, z=10.0):
    """A row of n returns: u falls by du per column from u0, x by dx from x0; (u, v, x, y, z) per return."""
    return [(u0 - du * c, v, x0 - dx * c, y, z) for c in range(n)]


def three_rows(n=30, du=4.0, dx=0.5, z=10.0, dy=2.0):
    """Rows at v = 10, 20, 30 (y = -dy, 0, dy), n columns each from u = 200 down: the standard layout.  The outer rows are
    0.2 off in x: among the third corners that tie, the first in list order then spans a triangle that is planar enough."""
    return [line(200.0, du, n, 10.0, x0=-0.2, dx=dx, y=-dy, z=z), line(200.0, du, n, 20.0, dx=dx, y=0.0, z=z),
            line(200.0, du, n, 30.0, x0=-0.2, dx=dx, y=dy, z=z)]


class Scene:
    """rows: lists of (u, v, x, y, z) in scan order.  The visible list is their concatenation, the original indices run
    the other way through a cloud with three more points, the pixel map keeps the first return with z > 0 of a cell."""

    def __init__(self, rows, W=SCENE_W, H=SCENE_H, row_capacity=64, repaired=RG.LITERAL, expect_rows=True):
        pts = np.array([p for row in rows for p in row], dtype=np.float64).reshape(-1, 5)
        n = pts.shape[0]
        self.W, self.H, self.n_vis, self.n_points = W, H, n, n + 3
        self.vis_uv = np.ascontiguousarray(pts[:, :2])
        self.index = (n + 2 - np.arange(n)).astype(np.int32)
        self.cam = np.full((self.n_points, 3), 777.0)
        self.cam[self.index] = pts[:, 2:]
        self.pm = np.full((H, W), -1, dtype=np.int32)
        for i in range(n):
            x, y = int(pts[i, 0]), int(pts[i, 1])
            if 0 <= x < W and 0 <= y < H and pts[i, 4] > 0 and self.pm[y, x] == -1:
                self.pm[y, x] = i
        self.row_capacity = row_capacity
        starts = RG.segment_rows(self.vis_uv[:, 0], repaired)
        if expect_rows:  # the rows the scene was built of are the rows the segmentation finds
            assert starts == list(np.cumsum([0] + [len(r) for r in rows])[:-1]), starts
        self.repaired = repaired

    def sequence(self):
        if self.repaired:
            starts = RG.segment_rows(self.vis_uv[:, 0], self.repaired)
            row_start = np.full(self.row_capacity + 1, -7, dtype=np.int32)
            row_start[:len(starts)] = starts
            row_start[len(starts)] = self.n_vis
            return RG.Sequence(self.pm, self.index, self.n_vis, self.cam, self.vis_uv, row_start, len(starts), self.n_vis,
                               self.row_capacity)
        rec, row_start = RG.cloud_record(self.vis_uv[:, 0], self.row_capacity)
        return RG.Sequence(self.pm, self.index, self.n_vis, self.cam, self.vis_uv, row_start, rec["n_rows"], rec["n_vis"],
                           self.row_capacity)


def scene_frame(P, cam=SCENE_CAM):
    """The oracle frame the tail takes its viewing ray from."""
    return make_oracle(P, CameraPinhole(*cam), IDENTITY)


def at(row, c, du=4.0, u0=200.0):
    """A feature whose 3 x 3 window holds column c of the row at v (and nothing else at du >= 2)."""
    return (u0 - du * c + 0.5, row + 0.5)


def quirk_cases():
    """name -> (rows, params, growth, feature, the repaired names).  On every one the literal record or list differs from
    the repaired one; test_row_growth_gpu.py runs the literal side of each on the GPU."""
    P = scene_params()
    cases = {}
    # the float fold: three returns in one window (du = 1), scan order is ascending x = descending column
    # (the floats around 10 are 9.5e-7 apart)
    for name, zs in (("float_fold_up", (11.0, 10.0000006, 10.0000008)),     # (float)10.0000006 rounds up past 10.0000008
                     ("float_fold_down", (11.0, 10.0000003, 10.0000001))):  # (float)10.0000003 rounds down to 10.0
        rows = [line(200.0, 1.0, 120, 10.0, dx=0.05, y=-0.5), line(200.0, 1.0, 120, 20.0, dx=0.05),
                line(200.0, 1.0, 120, 30.0, dx=0.05, y=0.5)]
        for k, z in enumerate(zs):  # columns 41, 40, 39 are read in this order
            u, v, x, y, _ = rows[1][41 - k]
            rows[1][41 - k] = (u, v, x, y, z)
        cases[name] = (rows, P, GENEROUS, (160.5, 20.5), {"float_fold"})
    # a jump of exactly 50 between the end of the top row and the start of the seed's row opens no row
    rows = [line(200.0, 4.0, 26, 10.0, y=-0.5), line(150.0, 4.0, 30, 20.0, x0=-6.25), line(200.0, 4.0, 30, 30.0, y=0.5)]
    cases["strict_50"] = (rows, P, GENEROUS, (150.0 - 4.0 * 8 + 0.5, 20.5), {"strict_50"})
    # the feature half way between the rows above and below: a tie, the bottom row comes first
    cases["tie_bottom"] = (three_rows(), P, GENEROUS, (200.0 - 4.0 * 12 + 0.5, 20.0), {"tie_bottom"})
    # the crossing column c against c - 1: |p_c - f|^2 = 90.5 is compared with |p_c - p_{c-1}|^2 = 16, not with 102.5
    cases["pc_pc1"] = (three_rows(), P, GENEROUS, at(20.0, 12), {"pc_pc1"})
    # maxDistanceSeed is the NEIGHBOUR limit 2 and maxDistanceNeighbor the neighbour-to-seed limit 5
    cases["swapped_roles"] = (three_rows(), P, GENEROUS, at(20.0, 12), {"swapped_roles"})
    # `last` stays the last point accepted above the seed: the first point below is 2.5 from it
    cases["last_kept"] = (three_rows(), P, RG.growth(0, 5, 0, 1, 0, 2, 0, -1), at(20.0, 12), {"last_kept"})
    # the merge stops when the columns below the seed run out
    cases["merge_either"] = (three_rows(), P, RG.growth(0, 5, 0, 5, 0, 2, 0, 256), at(20.0, 2), {"merge_either"})
    cases["half_count_odd"] = (three_rows(), P, RG.growth(0, 5, 0, 5, 0, 2, 0, 5), at(20.0, 12), {"half_count"})
    cases["half_count_zero"] = (three_rows(), P, RG.growth(0, 5, 0, 5, 0, 2, 0, 0), at(20.0, 12), {"half_count"})
    # above the threshold the delta is z - start: 0.2 + 19.8 * 0.02 = 0.596 reaches the neighbour at 0.5, 0.2 + 10 * 0.02 does not
    cases["max_dist_above"] = (three_rows(z=20.0, dy=0.5), P, capi.row_growth_params_yaml().replace(depth_segmentation_max_pointcount=-1),
                               at(20.0, 12), {"max_dist_start"})
    return cases


def run_case(rows, P, G, feature, repaired=RG.LITERAL):
    scene = Scene(rows, repaired=repaired & {"strict_50"}, expect_rows=False)
    seq = scene.sequence()
    if repaired - {"strict_50"}:  # the record through the repaired rule: the same composition, rule by rule
        nb = RG.window_list(seq, P, *feature)
        zs = [seq.point3(m)[2] for m in nb]
        seed = nb[RG.seed_fold(zs, repaired)]
        g = RG.neighbor_points(seq, G, feature, seed, repaired)
        return dict(seed_vis=seed, state=g["state"], second_vis=g["second_vis"], n_first=g["n_first"], grown=g["grown"],
                    seed_row=g["seed_row"])
    rec, lists = RG.records(scene_frame(P), P, G, seq, [feature])
    r = rec[0]
    return dict(seed_vis=int(r["seed_vis"]), state=int(r["state"]), second_vis=int(r["second_vis"]), n_first=int(r["n_first"]),
                grown=lists[0].tolist(), seed_row=int(r["seed_row"]), rec=r)


# ---- the randomised sweep: synthetic scan-ordered clouds -----------------------------------------------------------------

SWEEP_W, SWEEP_H, SWEEP_F = 96, 40, 96.0
SWEEP_CAM = (SWEEP_W, SWEEP_H, SWEEP_F, 48.0, 20.0)
SWEEP_SEEDS = 40
SWEEP_GROWTH = {"default": capi.row_growth_params_default, "yaml": capi.row_growth_params_yaml, "generous": lambda: GENEROUS}


def sweep_params():
    return capi.params_c0().replace(do_use_ransac_plane=0)


def sweep_scene(seed, n_features=16):
    """(Scene, features): beams of jittered v whose u falls from the right border to the left, the depth in steps; a tenth
    of the clouds has one beam only.  The features lie near returns."""
    rng = np.random.default_rng(9100 + seed)
    n_beams = 1 if seed % 10 == 9 else int(rng.integers(4, 9))
    vs = np.sort(rng.uniform(3.0, SWEEP_H - 3.0, n_beams))

    def profile():  # the depth over u: a few levels with steps between them
        edges = np.sort(rng.uniform(0.0, SWEEP_W, int(rng.integers(1, 5))))
        levels = rng.uniform(4.0, 14.0, edges.size + 1)
        return lambda u: levels[np.searchsorted(edges, u)]

    shared = profile()
    rows = []
    for b in range(n_beams):
        depth = profile() if rng.random() < 0.15 else shared  # a beam on another object
        du_max = rng.uniform(1.2, 4.5)
        u = rng.uniform(88.0, 95.0)
        end = rng.uniform(1.0, 30.0)
        row = []
        while u > end:
            zz = depth(u) + rng.normal(0.0, 0.01)
            v = vs[b] + rng.normal(0.0, 0.15)
            row.append((u, v, (u - 48.0) / SWEEP_F * zz, (v - 20.0) / SWEEP_F * zz, zz))
            u -= rng.uniform(0.7, du_max)
        rows.append(row)
    scene = Scene(rows, W=SWEEP_W, H=SWEEP_H, row_capacity=16)
    pick = rng.integers(0, scene.n_vis, n_features)
    uv = scene.vis_uv[pick] + rng.uniform(-1.5, 1.5, (n_features, 2))
    uv[::4] = np.floor(uv[::4])
    return scene, np.ascontiguousarray(uv)


def sweep_records(name):
    """Per seed (scene, features, records, lists) of the restatement for the parameter set `name`."""
    P, G = sweep_params(), SWEEP_GROWTH[name]()
    frame = scene_frame(P, SWEEP_CAM)
    out = []
    for seed in range(SWEEP_SEEDS):
        scene, uv = sweep_scene(seed)
        rec, lists = RG.records(frame, P, G, scene.sequence(), uv)
        out.append((scene, uv, rec, lists))
    return out


# ---- the reference's own test case ----------------------------------------------------------------------------------------

def reference_grid():
    """test_monolidar_fusion.cpp:187-227: 20 x 20 points at z = 20, x from 10 down to -9 inside y from -10 up to 9, camera
    f = 600 with the principal point (1000, 1000), identity transform."""
    pts = np.array([(x, y, 20.0) for y in np.arange(-10.0, 10.0) for x in np.arange(10.0, -10.0, -1.0)])
    uv = np.stack([600.0 * pts[:, 0] / 20.0 + 1000.0, 600.0 * pts[:, 1] / 20.0 + 1000.0], axis=1)
    return pts, uv


def grid_sequence():
    pts, uv = reference_grid()
    rec, row_start = RG.cloud_record(uv[:, 0], 64)
    return RG.Sequence(np.full((1, 1), -1, np.int32), np.arange(400, dtype=np.int32), 400, pts, uv, row_start, rec["n_rows"],
                       rec["n_vis"], 64)


def test_the_reference_grid_has_twenty_rows():
    _, uv = reference_grid()
    assert RG.segment_rows(uv[:, 0]) == list(range(0, 400, 20))
    rec, row_start = RG.cloud_record(uv[:, 0], 64)
    assert (rec["n_rows"], rec["n_vis"], rec["longest_row"], rec["flags"]) == (20, 400, 20, 0)
    assert row_start[:21].tolist() == list(range(0, 401, 20)) and (row_start[21:] == -7).all()


@pytest.mark.parametrize("G,state,grown", [
    (RG.growth(0, 5, 0, 5, 0, 2, 0, -1), 1, [211, 212, 209, 208, 231, 232, 229, 228]),  # asserted there: result 1, size 8
    (RG.growth(0, 5, 0, 5, 0, 2, 0, 4), 1, [211, 209, 231, 229]),
    (capi.row_growth_params_yaml(), -3, [])])
def test_the_references_own_test_case(G, state, grown):
    """The feature (1000, 1000) is the return 210, which the reference's getNearestPoint finds among all 400."""
    seq = grid_sequence()
    g = RG.neighbor_points(seq, G, (1000.0, 1000.0), 210)
    assert (g["state"], g["grown"]) == (state, grown) and not seq.bad
    assert g["seed_row"] == 10 and g["second_row"] == 11 and g["second_vis"] == 230  # a tie: the bottom row


# ---- the C-ABI, the layouts, the names --------------------------------------------------------------------------------------

def test_header_capi_and_both_libraries_carry_the_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in SYMBOLS:
            assert name in declared and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name, value in (("MLD_ROW_GROWTH_MAX_COUNT", 256), ("MLD_ROW_GROWTH_MAX_LIST", 1024), ("MLD_ROW_GROWTH_MAX_ROWS", 65536)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code) and getattr(capi, name) == value, name
    for name, value in (("BAD_INPUT", 1), ("NONFINITE_FEATURE", 2), ("ROWS_TRUNCATED", 4), ("LIST_CAPPED", 8)):
        assert re.search(rf"\bMLD_ROW_GROWTH_FLAG_{name} = {value}\b", code) and getattr(capi, "MLD_ROW_GROWTH_FLAG_" + name) == value
    assert "mld_row_growth below" in header  # the pointer at do_use_depth_segmentation
    assert [capi.RESULT_TYPE_NAMES[t] for t in (17, 18, 19, 20)] == [
        "RegionGrowingNearestSeedNotAvailable", "RegionGrowingSeedsOutOfRange", "RegionGrowingInsufficientPoints",
        "SuccessRegionGrowing"]
    assert "mld_row_growth_segment_device" in (ROOT / "INTEGRATION.md").read_text()


def _struct_fields(code, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", code, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * int(m.group(2) or 1)))
    offset, laid = 0, []
    for field, size in fields:
        laid.append((field, offset, size))
        offset += size
    return laid, offset


def test_the_structs_have_the_sizes_and_the_offsets_of_the_header():
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    laid, size = _struct_fields(code, "mld_row_growth")
    assert laid == LAYOUT and size == 72 and size % 8 == 0
    assert C.sizeof(capi.MldRowGrowth) == 72 and C.alignment(capi.MldRowGrowth) == 8
    assert [(n, getattr(capi.MldRowGrowth, n).offset, getattr(capi.MldRowGrowth, n).size)
            for n, _ in capi.MldRowGrowth._fields_] == LAYOUT
    assert RG.DTYPE.itemsize == 72 and [(n, RG.DTYPE.fields[n][1]) for n in RG.DTYPE.names] == [(n, o) for n, o, _ in LAYOUT]
    laid, size = _struct_fields(code, "mld_row_growth_params")
    assert [n for n, _, _ in laid] == PARAM_NAMES + ["pad_"] and size == 64 == C.sizeof(capi.MldRowGrowthParams)
    assert [n for n, _ in capi.MldRowGrowthParams._fields_] == PARAM_NAMES + ["pad_"]
    laid, size = _struct_fields(code, "mld_row_growth_cloud")
    assert [n for n, _, _ in laid] == ["n_rows", "n_vis", "longest_row", "flags"] == [n for n, _ in capi.MldRowGrowthCloud._fields_]
    assert size == 16 == C.sizeof(capi.MldRowGrowthCloud)
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "rows" / "mld_row_growth.hip").read_text()
    assert "static_assert(sizeof(mld_row_growth) == 72" in source


def test_the_two_parameter_sets_are_the_references():
    d, y = capi.row_growth_params_default(), capi.row_growth_params_yaml()
    assert [getattr(d, n) for n in PARAM_NAMES] == [0.0, 0.3, 0.0, 0.5, 0.0, 0.5, 0.0, 5]      # DepthEstimatorParameters.h:52-60
    assert [getattr(y, n) for n in PARAM_NAMES] == [10.0, 0.2, 0.02, 0.5, 0.05, 0.5, 0.05, 4]  # parameters.yaml:77-91
    g = RG.growth(1, 2, 3, 4, 5, 6, 7, 8)
    assert (g.depth_segmentation_max_seedpoint_to_seedpoint_distance, g.depth_segmentation_max_neighbor_to_seedpoint_distance,
            g.depth_segmentation_max_neighbor_distance) == (2, 4, 6)


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "RowGrowth" in m.__all__
    for name in ("segment", "collect", "collect_tracks", "records", "cloud_records", "close"):
        assert hasattr(m.RowGrowth, name), name
    assert m.RowGrowth.WORDS == 9 and m.RowGrowth.DTYPE.itemsize == 72 and m.RowGrowth.CLOUD_DTYPE.itemsize == 16
    assert (m.RowGrowth.MAX_COUNT, m.RowGrowth.MAX_LIST, m.RowGrowth.MAX_ROWS) == (256, 1024, 65536)
    assert hasattr(m.TrackletBatch, "attach_row_growth") and hasattr(m.TrackletBatch, "row_growth")
    rows = [(attr, row) for attr, row in m.TrackletBatch._ATTACHABLE.items() if row[0] is m.RowGrowth]
    assert len(rows) == 1 and rows[0][1][1] == "attach_row_growth"


def test_the_row_growth_is_a_translation_unit_of_its_own():
    """In rows/, on the shared batch headers and the public header only, linked into both libraries; the depth path's
    sources do not know of it; four kernels with stable names; no inline assembly, no atomics."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "rows" / "mld_row_growth.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h",
                                                           "../batch/mld_depth_path.h", "../../../include/mld.h"]
    code = re.sub(r"//.*", "", text)
    assert "mld_device.h" not in text and "mld_diag.h" not in text and "asm" not in code and "atomic" not in code
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_rg_pass", "k_rg_scan", "k_rg_write", "k_row_growth"]
    for shared in ("gather_window(", "max_spanning_triangle(", "list_minmax_z(", "finish_main(", "feature_grid(", "read_feature<",
                   "store_record(", "scan_chunk_counts(", "group_ranks<"):
        assert shared in code, shared
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(ROWS)" in ln for ln in link_lines)
    assert re.search(r"^ROWS\s*:=\s*rows/mld_row_growth\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(ROWS\)", mk, flags=re.M)
    for path in csrc.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert "mld_row_growth" not in path.read_text(), path.name


# ---- the refusals that need no GPU ------------------------------------------------------------------------------------------

def _create(ctx, P, G, cam, T=IDENTITY, sizes=(4, 1000, 5000, 64)):
    lib = capi.load()
    st = C.c_int(0)
    Tp = np.ascontiguousarray(T, dtype=np.float64).reshape(-1).ctypes.data_as(C.POINTER(C.c_double)) if T is not None else None
    handle = lib.mld_row_growth_create(ctx, *sizes, C.byref(P) if P is not None else None, C.byref(G) if G is not None else None,
                                       C.byref(cam) if cam is not None else None, Tp, C.byref(st))
    assert not handle
    return st.value, lib.mld_row_growth_last_error(None).decode()


@pytest.mark.parametrize("sizes,word", [
    ((0, 100, 100, 8), "n_seq"), ((65537, 100, 100, 8), "n_seq"), ((4, 0, 100, 8), "max_features"),
    ((4, 16777217, 100, 8), "max_features"), ((4, 100, 0, 8), "max_points"), ((4, 100, 8388608, 8), "max_points"),
    ((4, 100, 100, 0), "row_capacity"), ((4, 100, 100, 65537), "row_capacity")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(sizes, word):
    code, text = _create(None, None, None, None, None, sizes)
    assert code == capi.MLD_ERR_INVALID_ARG and "mld_row_growth_create" in text and word in text and "context" not in text


def test_create_judges_its_arguments_before_it_uses_the_context():
    P, G = capi.params_c0(), capi.row_growth_params_yaml()
    cam = capi.MldCamera(synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_W, synth.KITTI_H)
    assert _create(None, P, G, cam) == (capi.MLD_ERR_INVALID_ARG, "mld_row_growth_create: null context")
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert _create(fake, None, G, cam)[1] == "mld_row_growth_create: null params"
    assert _create(fake, P, None, cam)[1] == "mld_row_growth_create: null growth"
    assert _create(fake, P, G, None)[1] == "mld_row_growth_create: null camera"
    assert _create(fake, P, G, cam, None)[1] == "mld_row_growth_create: null T_cam_lidar"
    for count in (-2, 257):
        code, text = _create(fake, P, G.replace(depth_segmentation_max_pointcount=count), cam)
        assert code == capi.MLD_ERR_INVALID_ARG and "depth_segmentation_max_pointcount" in text
    for bad, want, word in ((dict(do_use_PCA=1), capi.MLD_ERR_UNSUPPORTED_MODE, "do_use_PCA"),
                            (dict(set_all_depths_to_zero=1), capi.MLD_ERR_UNSUPPORTED_MODE, "set_all_depths_to_zero"),
                            (dict(neighbor_search_mode=1), capi.MLD_ERR_UNSUPPORTED_MODE, "neighbor_search_mode has the invalid value: 1"),
                            (dict(plane_estimator_use_mestimator=0), capi.MLD_ERR_NO_ROAD_ESTIMATOR, "No road depth estimator selected."),
                            (dict(pixelarea_search_witdh=-1), capi.MLD_ERR_INVALID_ARG, "negative search window"),
                            (dict(pixelarea_search_witdh=40, pixelarea_search_height=40), capi.MLD_ERR_CAPACITY, "1024 cells")):
        for seg in (0, 1):  # do_use_depth_segmentation may hold either value: it is this object's subject
            code, text = _create(fake, P.replace(do_use_depth_segmentation=seg, **bad), G, cam)
            assert code == want and text.startswith("mld_row_growth_create: ") and word in text, bad
    code, text = _create(fake, P, G, capi.MldCamera(0.0, 1.0, 1.0, 64, 64))
    assert code == capi.MLD_ERR_INVALID_ARG and "bad camera intrinsics" in text
    T = IDENTITY.copy()
    T[1, 2] = np.nan
    code, text = _create(fake, P, G, cam, T)
    assert code == capi.MLD_ERR_INVALID_ARG and "non-finite" in text
    # mld_create keeps refusing the mode with the same text
    st = C.c_int(0)
    Tp = np.ascontiguousarray(IDENTITY).reshape(-1).ctypes.data_as(C.POINTER(C.c_double))
    assert not capi.load().mld_create(C.byref(P.replace(do_use_depth_segmentation=1)), C.byref(cam), Tp, 0, 1, 1000, 1000, C.byref(st))
    assert st.value == capi.MLD_ERR_UNSUPPORTED_MODE
    assert "DepthEstimator: Region growing not supported!" in capi.load().mld_create_error().decode()


@pytest.mark.parametrize("call", ["segment", "collect", "tracks"])
def test_calls_on_no_object_are_refused(call):
    lib = capi.load()
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    tail = (zero, tab, tab, zero, tab, zero, tab, tab, None, 0, tab, None, None, None)
    if call == "segment":
        rc, fn = lib.mld_row_growth_segment_device(None, tab, zero, None, tab, None), "mld_row_growth_segment_device"
    elif call == "collect":
        rc, fn = lib.mld_row_growth_collect_device(None, tab, *tail), "mld_row_growth_collect_device"
    else:
        rc, fn = lib.mld_row_growth_collect_tracks_device(None, tab, tab, *tail), "mld_row_growth_collect_tracks_device"
    assert rc == capi.MLD_ERR_INVALID_ARG and lib.mld_row_growth_last_error(None).decode() == fn + ": null object (rg)"
    lib.mld_row_growth_destroy(None)


def test_the_wrapper_refuses_before_any_call():
    """RowGrowth on a recording stand-in for the library: the argument checks of the shared helpers."""
    import torch
    from mono_lidar_depth_amd import RowGrowth
    from test_batch_wrappers_cpu import FakeEstimator, FakeLib, H, W
    lib = FakeLib()
    rg = RowGrowth(FakeEstimator(lib), 2, 100, 500, 8)
    name, args = lib.calls[0]
    assert name == "mld_row_growth_create" and args[1:5] == (2, 100, 500, 8) and args[6] is rg.growth
    mark = len(lib.calls)
    uv = [torch.zeros((5, 2), dtype=torch.float64), None]
    nvis, cloud = torch.zeros(2, dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32)
    rows = [torch.zeros(9, dtype=torch.int32) for _ in range(2)]
    with pytest.raises(ValueError, match="row_start"):
        rg.segment(uv, nvis, [rows[0], torch.zeros(8, dtype=torch.int32)], cloud)
    with pytest.raises(ValueError, match="cloud"):
        rg.segment(uv, nvis, rows, torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="one per sequence"):
        rg.segment(uv[:1], nvis, rows, cloud)
    feats = [torch.zeros((3, 2), dtype=torch.float64), None]
    pm = [torch.zeros((H, W), dtype=torch.int32), None]
    index, cam = [torch.zeros(5, dtype=torch.int32), None], [torch.zeros((7, 3), dtype=torch.float64), None]
    rec = [torch.zeros((3, 9), dtype=torch.int64), None]
    with pytest.raises(ValueError, match="list_capacity"):
        rg.collect(feats, pm, index, cam, uv, rows, cloud, rec, list_capacity=1025)
    with pytest.raises(ValueError, match="vis_uv"):
        rg.collect(feats, pm, index, cam, [torch.zeros((4, 2), dtype=torch.float64), None], rows, cloud, rec)
    with pytest.raises(ValueError, match="record"):
        rg.collect(feats, pm, index, cam, uv, rows, cloud, [torch.zeros((3, 8), dtype=torch.int64), None])
    with pytest.raises(ValueError, match="depth"):
        rg.collect(feats, pm, index, cam, uv, rows, cloud, rec, depth=[torch.zeros(3, dtype=torch.float32), None])
    assert lib.calls[mark:] == []
    rg.segment(uv, nvis, rows, cloud)
    rg.collect(feats, pm, index, cam, uv, rows, cloud, rec, depth=[torch.zeros(3, dtype=torch.float64), None])
    assert [c[0] for c in lib.calls[mark:]] == ["mld_row_growth_segment_device", "mld_row_growth_collect_device"]
    assert lib.calls[mark][1][2] == [5, 0] and lib.calls[mark + 1][1][2] == [3, 0] and lib.calls[mark + 1][1][11] == 0


def test_the_batch_segments_and_collects_on_the_tables_of_a_frame():
    """TrackletBatch.row_growth on the recording stand-in: the guard, one create, then the segment call on the exported
    clouds and the tracks form of the collect call with the step's outputs as merge arrays."""
    from mono_lidar_depth_amd import DepthEstimatorError, RowGrowth
    from test_batch_wrappers_cpu import H, S, U8, P as ptrs, W, batch, clouds, frame_lists, per
    lib, tb = batch()
    f = tb.prepare(is_new=per([7, 1, 3], U8), **frame_lists())
    tb.attach_projected_clouds()
    cl = tb.projected_clouds(clouds(), cam=True, pixel_map=True)
    with pytest.raises(DepthEstimatorError, match="TrackletBatch.row_growth without attach_row_growth"):
        tb.row_growth(f, cl)
    growth = capi.row_growth_params_yaml()
    rg = tb.attach_row_growth(growth, row_capacity=8, max_points=50)
    assert type(rg) is RowGrowth and tb.attach_row_growth() is rg and rg.growth is growth
    assert lib.calls[-1][0] == "mld_row_growth_create" and lib.calls[-1][1][1:5] == (S, 10, 50, 8)
    with pytest.raises(ValueError, match="projected_clouds"):
        tb.row_growth(f, dict(cl, pixel_map=None))
    mark = len(lib.calls)
    out = tb.row_growth(f, cl, list_capacity=3, merge=f["current"])
    seg, col = lib.calls[mark:]
    assert seg[0] == "mld_row_growth_segment_device" and col[0] == "mld_row_growth_collect_tracks_device"
    assert seg[1][1] == ptrs(cl["uv"]) and seg[1][2] == [33, 0, 5] and seg[1][3] == cl["n_visible"].data_ptr()
    assert seg[1][4] == ptrs(out["row_start"]) and seg[1][5] == out["cloud"].data_ptr()
    got = col[1]
    (u_new, v_new), (d_cur, t_cur) = f["features"], f["current"]
    assert got[1:4] == (ptrs(u_new), ptrs(v_new), [7, 1, 3]) and got[6] == [33, 0, 5] and got[8] == [33, 0, 5]
    assert got[9:13] == (ptrs(cl["uv"]), ptrs(out["row_start"]), out["cloud"].data_ptr(), 3)
    assert got[13:] == (ptrs(out["record"]), ptrs(out["grown"]), ptrs(d_cur), ptrs(t_cur))
    assert [tuple(t.shape) for t in out["record"]] == [(7, 9), (1, 9), (3, 9)] and [tuple(t.shape) for t in out["grown"]] == [(7, 3), (1, 3), (3, 3)]
    assert all(t.numel() == 9 for t in out["row_start"]) and tuple(out["cloud"].shape) == (S, 4) and (H, W) == tuple(cl["pixel_map"][0].shape)
    out = tb.row_growth(f, cl)
    assert out["grown"] is None and lib.calls[-1][1][12:] == (0, ptrs(out["record"]), None, None, None)


# ---- the tail and the window are the oracle's -------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [dict(), dict(do_use_triangle_size_maximation=0, treshold_depth_local_mode=1)])
def test_tail_and_window_are_the_oracle_on_a_synthetic_frame(variant):
    """On the window's own list the tail is calculate_depth with the count test and the histogram off, road off; and
    window_list reads the oracle's neighbours from the oracle's pixel map."""
    P = capi.params_c0().replace(do_use_ransac_plane=0, **variant)
    cloud = synth.make_cloud(synth.HDL64, seed=3, frame=0)
    uv = np.concatenate([synth.make_features(100, seed=3), synth.make_features_near_points(cloud, 200, seed=4)])
    ref = make_oracle(P.replace(do_use_histogram_segmentation=0, radiusSearch_count_min=0))
    ref.set_cloud(cloud)
    ref.set_ground_plane(None, None)
    depth, types = ref.calculate_depth(uv)
    cam_pts = np.ascontiguousarray(ref.cloud_camera_cs().T)
    index = ref.point_index()
    seq = RG.Sequence(ref.pixel_map(), index, index.size, cam_pts, ref.visible_image_points().T.reshape(-1, 2), [0, index.size], 1,
                      index.size, 1)
    wrong = []
    for i, (u, v) in enumerate(uv):
        nb = ref.trace_feature(float(u), float(v))["nb_idx"]
        assert RG.window_list(seq, P, float(u), float(v)) == nb.tolist() and not seq.bad
        t, d, _ = RG.tail(ref, P, u, v, cam_pts[index[nb]])
        if t != types[i] or np.float64(d).view(np.int64) != depth[i].view(np.int64):
            wrong.append((i, t, int(types[i]), d, float(depth[i])))
    assert not wrong, wrong[:5]
    assert 1 in set(types.tolist())


# ---- the quirks -------------------------------------------------------------------------------------------------------------

QUIRK_EXPECT = {  # name -> what the literal rule gives: (state, seed column or None, second_vis - row start, n_first, n_grown)
    "float_fold_up": (1, 39, None, None, None), "float_fold_down": (1, 40, None, None, None),
    "strict_50": (1, None, None, None, None), "tie_bottom": (1, 12, 11, 8, 16), "pc_pc1": (1, 12, 11, 8, 16),
    "swapped_roles": (1, 12, 11, 8, 16), "last_kept": (1, 12, 11, 4, 8), "merge_either": (1, 2, 1, 4, 5),
    "half_count_odd": (1, 12, 11, 2, 5), "half_count_zero": (1, 12, 11, 1, 2), "max_dist_above": (1, 12, 11, 2, 4)}


@pytest.mark.parametrize("name", sorted(quirk_cases()))
def test_the_literal_rule_and_the_repaired_rule_differ(name):
    rows, P, G, feature, repaired = quirk_cases()[name]
    lit, rep = run_case(rows, P, G, feature), run_case(rows, P, G, feature, frozenset(repaired))
    keys = ("seed_vis", "seed_row", "state", "second_vis", "n_first", "grown")
    assert [lit[k] for k in keys] != [rep[k] for k in keys], (lit, rep)
    state, col, second, n_first, n_grown = QUIRK_EXPECT[name]
    assert lit["state"] == state and not (lit["rec"]["flags"] & RG.BAD_INPUT)
    seq = Scene(rows, expect_rows=False).sequence()
    start = int(seq.row_start[lit["seed_row"]])
    if col is not None:
        assert lit["seed_vis"] - start == col
    if second is not None:
        assert lit["second_vis"] - int(seq.row_start[lit["rec"]["second_row"]]) == second
    if n_first is not None:
        assert lit["n_first"] == n_first
    if n_grown is not None:
        assert len(lit["grown"]) == n_grown
    if name == "strict_50":  # the top row and the seed's row are one row of 56
        assert seq.n_rows == 2 and lit["seed_row"] == 0 and rep["seed_row"] == 1
    if name == "tie_bottom":
        assert lit["rec"]["second_row"] == 2 and rep["second_vis"] < lit["seed_vis"]
    if name == "float_fold_up":
        assert rep["seed_vis"] - start == 40
    if name == "float_fold_down":
        assert rep["seed_vis"] - start == 39


def test_get_max_dist_below_and_above_the_threshold():
    """Below (and at) the threshold both rules give the start value - the quirk cannot show there; above it the delta is
    taken from the start value, not from the threshold."""
    assert RG.get_max_dist(10.0, 0.5, 0.05, 10.0) == RG.get_max_dist(10.0, 0.5, 0.05, 3.0) == 0.5
    assert RG.get_max_dist(10.0, 0.5, 0.05, 10.0, {"max_dist_start"}) == 0.5
    assert RG.get_max_dist(10.0, 0.5, 0.05, 20.0) == 0.5 + (20.0 - 0.5) * 0.05 == 1.475
    assert RG.get_max_dist(10.0, 0.5, 0.05, 20.0, {"max_dist_start"}) == 0.5 + 10.0 * 0.05 == 1.0


def test_the_strict_fifty_and_the_float_fold_on_bare_lists():
    assert RG.segment_rows([100.0, 50.0, 100.0, 40.0]) == [0] and RG.segment_rows([100.0, 50.0, 100.0, 40.0], {"strict_50"}) == [0, 2]
    assert RG.segment_rows([100.0, 50.0, np.nextafter(100.0, 200.0)]) == [0, 2]
    assert RG.segment_rows([]) == [] and RG.segment_rows([np.nan, 5.0, np.nan, 500.0]) == [0]  # no comparison with a NaN holds
    assert RG.seed_fold([10.0000006, 10.0000008]) == 1 and RG.seed_fold([10.0000006, 10.0000008], {"float_fold"}) == 0
    assert RG.seed_fold([10.0000003, 10.0000001]) == 0 and RG.seed_fold([10.0000003, 10.0000001], {"float_fold"}) == 1
    assert RG.seed_fold([np.nan, np.inf]) == -1 and RG.seed_fold([]) == -1 and RG.seed_fold([np.inf, 1e39, 1e39]) == 2  # (float)1e39 is +inf


# ---- the sweep's generator reaches every state ----------------------------------------------------------------------------

def test_the_sweep_reaches_every_state_in_the_restatement_alone():
    """Over the 40 seeds and the three parameter sets the restatement gives every state and type 20 at least 20 times."""
    states, types = [], []
    for name in SWEEP_GROWTH:
        for _, _, rec, _ in sweep_records(name):
            states += rec["state"].tolist()
            types += rec["type"].tolist()
    for state in (1, -1, -2, -3):
        assert states.count(state) >= 20, (state, states.count(state))
    assert types.count(20) >= 20, types.count(20)
