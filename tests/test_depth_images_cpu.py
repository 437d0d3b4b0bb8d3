"""The batched depth images without a GPU: symbols, the record's layout, the refusals of create in their documented order -
the context last, so all of them are reached without one -, the Python names, where the source sits, and what the frames of
the GPU tests reach, by the oracle at every pixel."""
import collections
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi, synth

import depth_image_frames as F

ROOT = Path(__file__).resolve().parent.parent

SYMBOLS = ("mld_depth_images_create", "mld_depth_images_destroy", "mld_depth_images_last_error", "mld_depth_images_render_device")


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
        for name in SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_depth_images mld_depth_images;" in code
    for word in ("120 * n_seq bytes", "128 * TILES * n_seq bytes", "512 * TILES * n_seq bytes", "16 * 120 * n_seq bytes",
                 "more than 1024 cells", "four launches", "no atomics", "MLD_DEPTH_IMAGE_COOP=1", "do_use_PCA",
                 "plane_estimator_use_triangle_maximation", "set_all_depths_to_zero"):
        assert word in header, word
    for name, value in (("MLD_DEPTH_IMAGE_FLAG_BAD_INPUT", 1), ("MLD_DEPTH_IMAGE_FLAG_HAS_PLANE", 2)):
        assert re.search(rf"\b{name} = {value}\b", code), name
        assert getattr(capi, name) == value


def test_the_record_has_the_size_and_the_offsets_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    n_types = int(re.search(r"MLD_RESULT_TYPE_COUNT = (\d+)", header).group(1))
    body = re.search(r"typedef struct mld_depth_image_record \{(.*?)\} mld_depth_image_record;", header, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\w+)\])?\s*$", item)
            count = {None: 1, "MLD_RESULT_TYPE_COUNT": n_types}.get(m.group(2)) or int(m.group(2))
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * count))
    offset, laid = 0, []
    for name, size in fields:
        laid.append((name, offset, size))
        offset += size
    assert laid == F.LAYOUT and offset == 200  # (every field is naturally aligned where it falls: no padding)
    assert C.sizeof(capi.MldDepthImageRecord) == 200 and C.alignment(capi.MldDepthImageRecord) == 8
    assert [(n, getattr(capi.MldDepthImageRecord, n).offset, getattr(capi.MldDepthImageRecord, n).size)
            for n, _ in capi.MldDepthImageRecord._fields_] == F.LAYOUT
    assert F.DTYPE.itemsize == 200 and [(n, F.DTYPE.fields[n][1]) for n in F.DTYPE.names] == [(n, o) for n, o, _ in F.LAYOUT]
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "images" / "mld_depth_images.hip").read_text()
    assert "static_assert(sizeof(mld_depth_image_record) == 200" in source
    assert "offsetof(mld_depth_image_record, n_cooperative) == 184" in source


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "DepthImages" in m.__all__
    for name in ("render", "records", "grid", "close"):
        assert hasattr(m.DepthImages, name), name
    assert m.DepthImages.WORDS * 8 == 200 and m.DepthImages.DTYPE == F.DTYPE
    assert hasattr(m.TrackletBatch, "attach_depth_images") and hasattr(m.TrackletBatch, "depth_images")
    assert hasattr(capi, "MldDepthImageRecord")


def _create(ctx, P, cam, Tp, n_seq=4):
    lib = capi.load()
    st = C.c_int(0)
    handle = lib.mld_depth_images_create(ctx, n_seq, C.byref(P) if P is not None else None, C.byref(cam) if cam is not None else None,
                                         Tp, C.byref(st))
    assert not handle
    return st.value, lib.mld_depth_images_last_error(None).decode()


def test_create_judges_everything_else_before_it_looks_at_the_context():
    """The documented order with a NULL context throughout: the size; null params, camera and transform; what only this
    object refuses; what mld_create refuses; the window bound; and only then the context."""
    P = capi.params_c0()
    cam = kitti()
    T, Tp = _transform()
    for n_seq in (0, -1, 65537):
        code, text = _create(None, None, None, None, n_seq)
        assert code == capi.MLD_ERR_INVALID_ARG and "n_seq" in text and "context" not in text
    assert _create(None, None, cam, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_depth_images_create: null params")
    assert _create(None, P, None, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_depth_images_create: null camera")
    assert _create(None, P, cam, None) == (capi.MLD_ERR_INVALID_ARG, "mld_depth_images_create: null T_cam_lidar")
    own = (dict(do_use_PCA=1), dict(plane_estimator_use_triangle_maximation=1), dict(set_all_depths_to_zero=1))
    for k, bad in enumerate(own):
        later = {}
        for b in own[k:]:  # (with the later ones set as well, the first is named)
            later.update(b)
        code, text = _create(None, P.replace(**later), cam, Tp)
        assert code == capi.MLD_ERR_UNSUPPORTED_MODE and text.startswith("mld_depth_images_create: " + next(iter(bad))), text
    for bad, want, word in ((dict(neighbor_search_mode=1), capi.MLD_ERR_UNSUPPORTED_MODE, "neighbor_search_mode"),
                            (dict(do_use_depth_segmentation=1), capi.MLD_ERR_UNSUPPORTED_MODE, "Region growing"),
                            (dict(plane_estimator_use_mestimator=0), capi.MLD_ERR_NO_ROAD_ESTIMATOR, "No road depth estimator"),
                            (dict(plane_estimator_use_mestimator=0, plane_estimator_use_leastsquares=1),
                             capi.MLD_ERR_UNSUPPORTED_MODE, "leastsquares"),
                            (dict(pixelarea_search_witdh=-1), capi.MLD_ERR_INVALID_ARG, "negative search window")):
        code, text = _create(None, P.replace(**bad), cam, Tp)
        assert code == want and "mld_depth_images_create" in text and word in text, bad
    code, text = _create(None, P, capi.MldCamera(64.0, 1.0, 1.0, 0, 64), Tp)
    assert code == capi.MLD_ERR_INVALID_ARG and "bad image size" in text
    code, text = _create(None, P, capi.MldCamera(64.0, 1.0, 1.0, 65536, 4), Tp)
    assert code == capi.MLD_ERR_CAPACITY and "65535" in text
    code, text = _create(None, P, capi.MldCamera(0.0, 1.0, 1.0, 64, 64), Tp)
    assert code == capi.MLD_ERR_INVALID_ARG and "intrinsics" in text
    Tbad = T.copy()
    Tbad[5] = np.inf
    code, text = _create(None, P, cam, Tbad.ctypes.data_as(C.POINTER(C.c_double)))
    assert code == capi.MLD_ERR_INVALID_ARG and "non-finite" in text
    # the wide window: min(W, floor(2 halfX2) + 2) * min(H, floor(2 halfY2) + 2) <= 1024; 15 x 42 -> 32 x 65 = 2080 cells
    code, text = _create(None, P.replace(pixelarea_search_witdh=15, pixelarea_search_height=42), cam, Tp)
    assert code == capi.MLD_ERR_CAPACITY and "more than 1024 cells" in text
    code, text = _create(None, P.replace(pixelarea_search_witdh=15, pixelarea_search_height=20), cam, Tp)  # 32 x 32: the bound
    assert (code, text) == (capi.MLD_ERR_INVALID_ARG, "mld_depth_images_create: null context")
    # and last the context
    assert _create(None, P, cam, Tp) == (capi.MLD_ERR_INVALID_ARG, "mld_depth_images_create: null context")
    assert not capi.load().mld_depth_images_create(None, 65536, None, None, None, None)  # (status_out is optional)


def test_render_on_no_object_is_refused():
    lib = capi.load()
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    rc = lib.mld_depth_images_render_device(None, tab, tab, zero, tab, zero, None, None, 0, 0, 1, 1, 1, 1, None, None, None, None)
    assert rc == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_depth_images_last_error(None).decode() == "mld_depth_images_render_device: null object (di)"
    lib.mld_depth_images_destroy(None)


def test_the_depth_images_are_a_translation_unit_of_their_own():
    """In images/, on the shared batch headers and the public header only, linked into both libraries; the depth path's
    sources and the other batch objects do not know of it; three kernels with stable names, no atomics, no inline
    assembly, and the environment is read in the A/B library alone."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "images" / "mld_depth_images.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h",
                                                           "../batch/mld_depth_path.h", "../../../include/mld.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    code = re.sub(r"//.*", "", text + (csrc / "batch" / "mld_depth_path.h").read_text())  # (the unit and the header its code moved to)
    assert "asm" not in code and "atomic" not in code.lower() and "__threadfence" not in code
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_depth_image_lane", "k_depth_image_coop", "k_depth_image_finish"]
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 3  # (+ the descriptor upload: four launches)
    assert "hipMalloc" not in text.split("mld_depth_images_render_device(")[-1]  # (nothing is allocated per call)
    guarded = re.findall(r"#ifdef MLD_AB_SWITCHES\n(.*?)#endif", code, flags=re.S)
    assert len(guarded) == 1 and "getenv" in guarded[0] and code.count("getenv") == 1
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(IMAGES)" in ln for ln in link_lines)
    assert re.search(r"^IMAGES\s*:=\s*images/mld_depth_images\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(COVERAGE\) \$\(IMAGES\)", mk, flags=re.M)
    assert "-ffp-contract=off" in mk
    for path in csrc.rglob("*"):
        if path.is_file() and path.name != "Makefile" and path.parent.name != "images":
            assert "mld_depth_image" not in path.read_text(), path.name


@pytest.mark.parametrize("which", ["mixed", "golden_c0"])
def test_the_frames_of_the_gpu_tests_reach_what_they_must(which):
    """The oracle at every pixel: the 64 x 64 mixed frame has ten result types with at least 15 pixels each, the golden
    frame adds type 4; both have pixels of both routes' interest - type 2 and road depths."""
    fr = F.mixed_frame() if which == "mixed" else F.golden_frame()
    depth, types = fr.expected()
    seen = collections.Counter(types.reshape(-1).tolist())
    if which == "mixed":
        assert set(seen) == {1, 2, 3, 5, 6, 7, 8, 9, 11, 16}
        assert seen[1] == 1976 and seen[16] == 101 and min(seen.values()) >= 15
    else:
        assert (fr.W, fr.H) == (320, 96) and seen[4] > 0 and seen[16] > 1000 and seen[1] > 1000 and seen[2] > 1000
    assert ((depth >= 0) == np.isin(types, (1, 16))).all() and (depth[~np.isin(types, (1, 16))] == -1).all()
