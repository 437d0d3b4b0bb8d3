"""The batched depth reports (statistics + interpolated clouds) without a GPU: symbols, the record's layout, what the
header states, refusals before the device is touched, the Python names, where the source sits."""
import ctypes as C
import re
from pathlib import Path

import pytest

from mono_lidar_depth_amd import capi, synth

ROOT = Path(__file__).resolve().parent.parent

REPORT_SYMBOLS = ("mld_depth_reports_create", "mld_depth_reports_destroy", "mld_depth_reports_last_error",
                  "mld_depth_reports_collect_device", "mld_depth_reports_collect_tracks_device")


def _camera(f=synth.KITTI_F):
    return capi.MldCamera(f, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_W, synth.KITTI_H)


def test_header_capi_and_library_carry_the_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    lib = capi.load()
    for name in REPORT_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct mld_depth_reports mld_depth_reports;" in code
    assert re.search(r"typedef struct mld_depth_report \{\s*int64_t counts\[MLD_RESULT_TYPE_COUNT\];\s*int64_t other;\s*"
                     r"int64_t point_count;\s*int64_t n_interpolated;\s*\} mld_depth_report;", code)
    assert lib.mld_abi_version() == 8


def test_the_record_is_24_int64():
    assert C.sizeof(capi.MldDepthReport) == 192 and C.alignment(capi.MldDepthReport) == 8
    assert capi.MldDepthReport.counts.offset == 0 and capi.MldDepthReport.counts.size == 8 * capi.MLD_RESULT_TYPE_COUNT
    assert capi.MldDepthReport.other.offset == 168
    assert capi.MldDepthReport.point_count.offset == 176
    assert capi.MldDepthReport.n_interpolated.offset == 184


def test_the_header_states_what_a_caller_needs():
    """The byte formulas, the criterion depth >= 0 with its edge values, the truncation of the tracks form, how a
    truncated sequence shows, which results the tracks form serves, and that the reference's own push is commented out."""
    header = " ".join((ROOT / "include" / "mld.h").read_text().replace("\n *", " ").split())
    for words in ("8 * ceil(max_features / 64) + 92 * ceil(max_features / 1024) + 60", "16 * 56 * n_seq",
                  "iff depth >= 0", "NaN is out, -0.0 and +inf are in", "(double)truncf(u)", "(double)(int)u",
                  "n_interpolated > capacity[s]", "x = (u - cu) / f * d", "y = (v - cv) / f * d",
                  "commented out (DepthEstimator.cpp:1028-1034)", "d_last is written only for new tracks and is not a valid input",
                  "Every record is written completely on every call", "IN FEATURE ORDER",
                  "nothing at or beyond min(n_interpolated, capacity[s]) is touched"):
        assert words in header, words


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "DepthReports" in m.__all__
    for name in ("collect", "collect_tracks", "close"):
        assert hasattr(m.DepthReports, name), name
    assert hasattr(m.TrackletBatch, "attach_reports") and hasattr(m.TrackletBatch, "reports")
    assert m.DepthReports.WORDS * 8 == C.sizeof(capi.MldDepthReport)


@pytest.mark.parametrize("n_seq,max_features,word", [(0, 100, "n_seq"), (-1, 100, "n_seq"), (65537, 100, "n_seq"),
                                                     (4, 0, "max_features"), (4, -5, "max_features"),
                                                     (4, 16777217, "max_features")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_features, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_depth_reports_create(None, n_seq, max_features, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_depth_reports_last_error(None).decode()
    assert "mld_depth_reports_create" in text and word in text and "context" not in text


def test_create_without_a_context_a_camera_or_a_focal_length_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    cam = _camera()
    assert not lib.mld_depth_reports_create(None, 4, 1000, C.byref(cam), C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_depth_reports_last_error(None).decode()
    assert not lib.mld_depth_reports_create(None, 65536, 16777216, None, None)  # (status_out is optional)
    assert "null context" in lib.mld_depth_reports_last_error(None).decode()
    # A null / unusable camera behind a context that is not null: the arguments are judged before the context is used, so
    # any non-null address will do here; nothing is dereferenced.
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert not lib.mld_depth_reports_create(fake, 4, 1000, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_depth_reports_last_error(None).decode()
    assert "mld_depth_reports_create" in text and "null camera" in text
    for f in (0.0, -0.0, float("nan"), float("inf"), float("-inf")):
        bad = _camera(f)
        st.value = 0
        assert not lib.mld_depth_reports_create(fake, 4, 1000, C.byref(bad), C.byref(st))
        assert st.value == capi.MLD_ERR_INVALID_ARG
        text = lib.mld_depth_reports_last_error(None).decode()
        assert "mld_depth_reports_create" in text and "focal_length" in text


def _good_args():
    tab = (C.c_void_p * 1)(None)
    zero = (C.c_int64 * 1)(0)
    return dict(a=tab, b=tab, depth=tab, type=None, n=zero, cap=None, report=None, points=None, feature=None)


REFUSALS = [dict(), dict(a=None), dict(b=None), dict(depth=None), dict(n=None), dict(n=(C.c_int64 * 1)(-1)),
            dict(n=(C.c_int64 * 1)(5)), dict(n=(C.c_int64 * 1)(16777217)), dict(points=(C.c_void_p * 1)(None)),
            dict(points=(C.c_void_p * 1)(None), cap=(C.c_int64 * 1)(-1)),
            dict(n=(C.c_int64 * 1)(5), a=(C.c_void_p * 1)(0x1002)), dict(report=C.c_void_p(0x1004)),
            dict(type=(C.c_void_p * 1)(None), feature=(C.c_void_p * 1)(None))]


@pytest.mark.parametrize("form", ["collect_device", "collect_tracks_device"])
@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: ",".join(d) or "good")
def test_collect_on_no_object_is_refused_whatever_the_arguments(bad, form):
    """Every refusal of the two calls, and a call with nothing else wrong, made on a null object: MLD_ERR_INVALID_ARG with
    a text that names the function and the object - decided on the host, no GPU is looked for."""
    lib = capi.load()
    lib.mld_depth_reports_destroy(None)
    assert not lib.mld_depth_reports_create(None, 0, 1, None, None)  # (leaves another text behind)
    a = dict(_good_args(), **bad)
    if form == "collect_device":
        rc = lib.mld_depth_reports_collect_device(None, a["a"], a["depth"], a["type"], a["n"], a["cap"], a["report"], a["points"],
                                                  a["feature"])
    else:
        rc = lib.mld_depth_reports_collect_tracks_device(None, a["a"], a["b"], a["depth"], a["type"], a["n"], a["cap"],
                                                         a["report"], a["points"], a["feature"])
    assert rc == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_depth_reports_last_error(None).decode()
    assert f"mld_depth_reports_{form}" in text and "null object" in text and "(dr)" in text


def test_the_reports_are_a_translation_unit_of_their_own():
    """In reports/, on the shared header only, linked into both libraries behind the clouds; the depth path's sources do
    not know of it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "reports" / "mld_depth_reports.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    for name in ("DescRing<", "create_object<", "destroy_object("):
        assert name in text, name
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(PCLOUDS) $(REPORTS) mld_params.cpp mld_host.cpp" in ln for ln in link_lines)
    assert all("$(TRACKS) $(LABELS) $(PLANES) $(RPLANES) $(PCLOUDS)" in ln for ln in link_lines)
    assert re.search(r"^REPORTS\s*:=\s*reports/mld_depth_reports\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(PCLOUDS\) \$\(REPORTS\)", mk, flags=re.M)
    for name in ("mld_api.hip", "mld_kernels.hip", "mld_ransac.hip", "mld_device.h", "mld_diag.h", "mld_host.cpp", "mld_params.cpp"):
        assert "mld_depth_reports" not in (csrc / name).read_text(), name
