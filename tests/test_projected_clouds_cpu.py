"""The batched export of the projected clouds without a GPU: symbols, refusals before the device is touched, the Python
names, where the source sits."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi, synth

ROOT = Path(__file__).resolve().parent.parent

CLOUD_SYMBOLS = ("mld_projected_clouds_create", "mld_projected_clouds_destroy", "mld_projected_clouds_last_error",
                 "mld_projected_clouds_export_device")


def _camera():
    return capi.MldCamera(synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_W, synth.KITTI_H)


def _transform():
    T = np.ascontiguousarray(np.asarray(synth.T_CAM_LIDAR, dtype=np.float64).reshape(-1)[:12])
    return T, T.ctypes.data_as(C.POINTER(C.c_double))


def test_header_capi_and_library_carry_the_four_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    lib = capi.load()
    for name in CLOUD_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct mld_projected_clouds mld_projected_clouds;" in code
    assert lib.mld_abi_version() == 8
    # the byte formula, the capacity rule and what a truncated sequence's map holds are stated where the caller reads them
    for word in ("8 * ceil(max_points / 64) + 4 * ceil(max_points / 1024) + 60", "16 * 56 * n_seq",
                 "n_visible_out_dev[s] > capacity[s]", "may hold values >= capacity[s]", "Every cell is"):
        assert word in header, word


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "ProjectedClouds" in m.__all__
    for name in ("export", "close"):
        assert hasattr(m.ProjectedClouds, name), name
    assert hasattr(m.TrackletBatch, "attach_projected_clouds") and hasattr(m.TrackletBatch, "projected_clouds")


@pytest.mark.parametrize("n_seq,max_points,word", [(0, 100, "n_seq"), (-1, 100, "n_seq"), (65537, 100, "n_seq"),
                                                   (4, 0, "max_points"), (4, -5, "max_points"), (4, 8388608, "max_points")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_points, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_projected_clouds_create(None, n_seq, max_points, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_projected_clouds_last_error(None).decode()
    assert "mld_projected_clouds_create" in text and word in text and "context" not in text


def test_create_without_a_context_a_camera_or_a_transform_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    cam = _camera()
    T, Tp = _transform()
    assert not lib.mld_projected_clouds_create(None, 4, 1000, C.byref(cam), Tp, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_projected_clouds_last_error(None).decode()
    assert not lib.mld_projected_clouds_create(None, 65536, 8388607, None, None, None)  # (status_out is optional)
    assert "null context" in lib.mld_projected_clouds_last_error(None).decode()
    # Null camera / transform behind a context that is not null: the arguments are judged before the context is used, so
    # any non-null address will do here; nothing is dereferenced.
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert not lib.mld_projected_clouds_create(fake, 4, 1000, None, Tp, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null camera" in lib.mld_projected_clouds_last_error(None).decode()
    assert not lib.mld_projected_clouds_create(fake, 4, 1000, C.byref(cam), None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null T_cam_lidar" in lib.mld_projected_clouds_last_error(None).decode()
    for w, h in ((0, 375), (1242, 0), (-3, 375)):
        bad = capi.MldCamera(synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, w, h)
        assert not lib.mld_projected_clouds_create(fake, 4, 1000, C.byref(bad), Tp, C.byref(st))
        assert st.value == capi.MLD_ERR_INVALID_ARG
        assert "width and height" in lib.mld_projected_clouds_last_error(None).decode()


def _good_args():
    tab = (C.c_void_p * 1)(None)
    zero = (C.c_int64 * 1)(0)
    return dict(pts=tab, n=zero, stride=16, cap=zero, nvis=None, uv=tab, index=tab, depth=None, cam=None, map=None)


REFUSALS = [dict(), dict(pts=None), dict(n=None), dict(cap=None), dict(uv=None), dict(index=None),
            dict(n=(C.c_int64 * 1)(-1)), dict(cap=(C.c_int64 * 1)(-1)), dict(stride=12), dict(stride=0),
            dict(n=(C.c_int64 * 1)(5)), dict(n=(C.c_int64 * 1)(8388608)),
            dict(n=(C.c_int64 * 1)(5), pts=(C.c_void_p * 1)(0x1002))]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: ",".join(d) or "good")
def test_export_on_no_object_is_refused_whatever_the_arguments(bad):
    """Every refusal of the call, and a call with nothing else wrong, made on a null object: MLD_ERR_INVALID_ARG with a
    text that names the object - decided on the host, no GPU is looked for."""
    lib = capi.load()
    lib.mld_projected_clouds_destroy(None)
    assert not lib.mld_projected_clouds_create(None, 0, 1, None, None, None)  # (leaves another text behind)
    a = dict(_good_args(), **bad)
    rc = lib.mld_projected_clouds_export_device(None, a["pts"], a["n"], a["stride"], a["cap"], a["nvis"], a["uv"], a["index"],
                                                a["depth"], a["cam"], a["map"])
    assert rc == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_projected_clouds_last_error(None).decode()
    assert "mld_projected_clouds_export_device" in text and "null object" in text and "(pc)" in text


def test_the_clouds_are_a_translation_unit_of_their_own():
    """In clouds/, on the public header only, linked into both libraries; the depth path's sources do not know of it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "clouds" / "mld_projected_clouds.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(PCLOUDS)" in ln for ln in link_lines)
    assert all("$(TRACKS) $(LABELS) $(PLANES) $(RPLANES)" in ln for ln in link_lines)
    assert re.search(r"^PCLOUDS\s*:=\s*clouds/mld_projected_clouds\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(PCLOUDS\)", mk, flags=re.M)
    for name in ("mld_api.hip", "mld_kernels.hip", "mld_ransac.hip", "mld_device.h"):
        assert "mld_projected_clouds" not in (csrc / name).read_text(), name
