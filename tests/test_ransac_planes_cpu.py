"""The batched RANSAC plane estimator's C-ABI without a GPU: symbols, the record's layout, refusals before the device is
touched, where the source sits."""
import ctypes as C
import re
from pathlib import Path

import pytest

from mono_lidar_depth_amd import capi

ROOT = Path(__file__).resolve().parent.parent

PLANE_SYMBOLS = ("mld_ransac_planes_create", "mld_ransac_planes_destroy", "mld_ransac_planes_last_error",
                 "mld_ransac_planes_estimate_device")


def test_header_capi_and_library_carry_the_four_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    lib = capi.load()
    for name in PLANE_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct mld_ransac_planes mld_ransac_planes;" in code
    assert lib.mld_abi_version() == 8
    # the byte formula, the parity contract and the failed sequences are stated where the caller reads them
    for word in ("8 * ceil(max_points / 64) + 4 * ceil(max_points / 1024) + 28", "16 * 24 * n_seq", "Parity contract",
                 "mld_estimate_ground_plane", "ExceptionPclInvalid", "caller's business"):
        assert word in header, word


def test_the_record_is_32_bytes_with_the_fields_where_the_header_puts_them():
    R = capi.MldRansacPlaneResult
    assert C.sizeof(R) == 32
    assert (R.coeffs.offset, R.coeffs.size) == (0, 16)
    assert (R.n_inliers.offset, R.iterations.offset, R.status.offset, R.n_candidates.offset) == (16, 20, 24, 28)
    assert all(getattr(R, f).size == 4 for f in ("n_inliers", "iterations", "status", "n_candidates"))
    header = (ROOT / "include" / "mld.h").read_text()
    body = re.search(r"typedef struct mld_ransac_plane_result \{(.*?)\} mld_ransac_plane_result;", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert fields == [("float", "coeffs"), ("int32_t", "n_inliers"), ("int32_t", "iterations"), ("int32_t", "status"),
                      ("int32_t", "n_candidates")]


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "RansacPlanes" in m.__all__
    for name in ("estimate", "close", "mask_words"):
        assert hasattr(m.RansacPlanes, name), name
    assert m.RansacPlanes.mask_words(0) == 0 and m.RansacPlanes.mask_words(33) == 2
    assert hasattr(m.TrackletBatch, "attach_ransac_planes") and hasattr(m.TrackletBatch, "ransac_planes")


@pytest.mark.parametrize("n_seq,max_points,word", [(0, 100, "n_seq"), (-1, 100, "n_seq"), (65537, 100, "n_seq"),
                                                   (4, 0, "max_points"), (4, -5, "max_points"), (4, 8388608, "max_points")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_points, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_ransac_planes_create(None, n_seq, max_points, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_ransac_planes_last_error(None).decode()
    assert "mld_ransac_planes_create" in text and word in text and "context" not in text


def test_create_without_a_context_or_without_params_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    P = capi.params_c0()
    assert not lib.mld_ransac_planes_create(None, 4, 1000, C.byref(P), C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_ransac_planes_last_error(None).decode()
    assert not lib.mld_ransac_planes_create(None, 65536, 8388607, None, None)  # (status_out is optional)
    assert "null context" in lib.mld_ransac_planes_last_error(None).decode()
    # Null params behind a context that is not null: the arguments are judged before the context is used, so any
    # non-null address will do here; nothing is dereferenced.
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert not lib.mld_ransac_planes_create(fake, 4, 1000, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null params" in lib.mld_ransac_planes_last_error(None).decode()
    bad = capi.params_c0().replace(ransac_plane_max_iterations=-1)
    assert not lib.mld_ransac_planes_create(fake, 4, 1000, C.byref(bad), C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "ransac_plane_max_iterations" in lib.mld_ransac_planes_last_error(None).decode()


def _good_args():
    tab = (C.c_void_p * 1)(None)
    return dict(pts=tab, n=(C.c_int64 * 1)(0), stride=16, seeds=(C.c_uint32 * 1)(7), res=None, mask=tab)


REFUSALS = [dict(), dict(pts=None), dict(n=None), dict(seeds=None), dict(mask=None), dict(n=(C.c_int64 * 1)(-1)),
            dict(stride=12), dict(stride=0), dict(n=(C.c_int64 * 1)(5))]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: ",".join(d) or "good")
def test_estimate_on_no_object_is_refused_whatever_the_arguments(bad):
    """Every refusal of the call, and a call with nothing else wrong, made on a null object: MLD_ERR_INVALID_ARG with a
    text that names the object - decided on the host, no GPU is looked for."""
    lib = capi.load()
    lib.mld_ransac_planes_destroy(None)
    assert not lib.mld_ransac_planes_create(None, 0, 1, None, None)  # (leaves another text behind)
    a = dict(_good_args(), **bad)
    rc = lib.mld_ransac_planes_estimate_device(None, a["pts"], a["n"], a["stride"], a["seeds"], a["res"], a["mask"])
    assert rc == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_ransac_planes_last_error(None).decode()
    assert "mld_ransac_planes_estimate_device" in text and "null object" in text and "(rp)" in text


def test_the_planes_are_a_translation_unit_of_their_own():
    """In planes/ beside the semantic unit, on the public header only, linked into both libraries; the depth path's
    sources do not know of it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "planes" / "mld_ransac_planes.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(RPLANES)" in ln for ln in link_lines)
    assert re.search(r"^RPLANES\s*:=\s*planes/mld_ransac_planes\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(RPLANES\)", mk, flags=re.M)
    for name in ("mld_api.hip", "mld_kernels.hip", "mld_ransac.hip", "mld_device.h"):
        assert "mld_ransac_planes" not in (csrc / name).read_text(), name
