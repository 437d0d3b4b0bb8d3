"""The batched semantic plane estimator's C-ABI without a GPU: symbols, the record's layout, refusals before the device
is touched, where the source sits."""
import ctypes as C
import re
from pathlib import Path

import pytest

from mono_lidar_depth_amd import capi

ROOT = Path(__file__).resolve().parent.parent

PLANE_SYMBOLS = ("mld_semantic_planes_create", "mld_semantic_planes_destroy", "mld_semantic_planes_last_error",
                 "mld_semantic_planes_estimate_device")


def test_header_declares_the_planes_and_keeps_the_abi_version():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    lib = capi.load()
    for name in PLANE_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct mld_semantic_planes mld_semantic_planes;" in code
    assert lib.mld_abi_version() == 8
    # the byte formula, the failed sequences and the round trip that remains are stated where the caller reads them
    for word in ("40 * ceil(max_points / 64)", "16 * 32 * n_seq", "ExceptionPclInvalid", "caller's business", "round trip remains"):
        assert word in header, word


def test_the_record_is_32_bytes_with_the_fields_where_the_header_puts_them():
    R = capi.MldSemanticPlaneResult
    assert C.sizeof(R) == 32
    assert (R.coeffs.offset, R.coeffs.size) == (0, 16)
    assert (R.n_candidates.offset, R.n_inliers.offset, R.status.offset, R.reserved.offset) == (16, 20, 24, 28)
    assert all(getattr(R, f).size == 4 for f in ("n_candidates", "n_inliers", "status", "reserved"))
    header = (ROOT / "include" / "mld.h").read_text()
    body = re.search(r"typedef struct mld_semantic_plane_result \{(.*?)\} mld_semantic_plane_result;", header, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert fields == [("float", "coeffs"), ("int32_t", "n_candidates"), ("int32_t", "n_inliers"), ("int32_t", "status"),
                      ("int32_t", "reserved")]


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "SemanticPlanes" in m.__all__ and hasattr(m.SemanticPlanes, "estimate") and hasattr(m.SemanticPlanes, "close")
    assert hasattr(m.TrackletBatch, "attach_planes") and hasattr(m.TrackletBatch, "semantic_planes")


@pytest.mark.parametrize("n_seq,max_points,word", [(0, 100, "n_seq"), (-1, 100, "n_seq"), (65537, 100, "n_seq"),
                                                   (4, 0, "max_points"), (4, -5, "max_points"), (4, 8388608, "max_points")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_points, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_semantic_planes_create(None, n_seq, max_points, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_semantic_planes_last_error(None).decode()
    assert "mld_semantic_planes_create" in text and word in text


def test_create_without_a_context_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_semantic_planes_create(None, 4, 1000, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_semantic_planes_last_error(None).decode()
    assert not lib.mld_semantic_planes_create(None, 65536, 8388607, None, None, None)  # (status_out is optional)
    assert "null context" in lib.mld_semantic_planes_last_error(None).decode()


def _good_args():
    tab = (C.c_void_p * 1)(None)
    n = (C.c_int64 * 1)(0)
    lab = (C.c_int32 * 4)(6, 7, 8, 9)
    return dict(pts=tab, n=n, stride=16, img=tab, rows=4, cols=4, row_stride=4, labels=C.addressof(lab), n_labels=4, thr=0.1,
                res=None, mask=tab, keep=lab)


def _estimate(lib, sp, a):
    return lib.mld_semantic_planes_estimate_device(sp, a["pts"], a["n"], a["stride"], a["img"], a["rows"], a["cols"],
                                                   a["row_stride"], a["labels"], a["n_labels"], a["thr"], a["res"], a["mask"])


REFUSALS = [dict(), dict(pts=None), dict(n=None), dict(img=None), dict(mask=None), dict(rows=0), dict(cols=-1),
            dict(row_stride=3), dict(n=(C.c_int64 * 1)(-1)), dict(stride=12), dict(stride=0), dict(n_labels=-1),
            dict(labels=None), dict(n=(C.c_int64 * 1)(5))]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: ",".join(d) or "good")
def test_estimate_on_no_object_is_refused_whatever_the_arguments(bad):
    """Every refusal of the call, and a call with nothing else wrong, made on a null object: MLD_ERR_INVALID_ARG with a
    text that names the object - decided on the host, no GPU is looked for."""
    lib = capi.load()
    lib.mld_semantic_planes_destroy(None)
    assert not lib.mld_semantic_planes_create(None, 0, 1, None, None, None)  # (leaves another text behind)
    assert _estimate(lib, None, dict(_good_args(), **bad)) == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_semantic_planes_last_error(None).decode()
    assert "mld_semantic_planes_estimate_device" in text and "null object" in text and "(sp)" in text


def test_the_planes_are_a_translation_unit_of_their_own():
    """In a subdirectory of csrc/, on the public header only, linked into both libraries; the depth path's sources do not
    know of it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "planes" / "mld_semantic_planes.hip").read_text()
    # public header only: through the shared header of the batch objects, which itself includes nothing else of the project
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h"]
    shared = (csrc / "batch" / "mld_batch_object.h").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', shared) == ["../../../include/mld.h"]
    for src in (text, shared):
        assert '#include "mld_' not in src and "mld_device.h" not in src and "mld_diag.h" not in src
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(PLANES)" in ln and "$(LABELS)" in ln and "$(TRACKS)" in ln for ln in link_lines)
    assert re.search(r"^PLANES\s*:=\s*planes/mld_semantic_planes\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(PLANES\)", mk, flags=re.M)
    for name in ("mld_api.hip", "mld_kernels.hip", "mld_ransac.hip", "mld_device.h"):
        assert "mld_semantic_planes" not in (csrc / name).read_text(), name
