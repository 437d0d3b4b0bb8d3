"""Import, reset and the per-lane calls of the batched tracklet layer without a GPU: the header declares the four
functions with their argument lists, the library exports them, capi binds them, calls without a store or context are
refused, the ABI version did not move, the classes offer the methods, and the restatement the GPU tests compare with
passes its self-test."""
import ctypes as C
import re
from pathlib import Path

from mono_lidar_depth_amd import TrackletBatch, TrackletStore, capi

import track_import_restatement

ROOT = Path(__file__).resolve().parent.parent

FEATURES = ["const float* const* u_new", "const float* const* v_new", "const float* const* u_old", "const float* const* v_old"]
OUTPUTS = ["const int64_t* n_tracks", "float* const* d_cur_out", "float* const* d_last_out", "int32_t* const* type_cur_out",
           "int32_t* const* type_last_out"]
ARGS = {
    "mld_tracks_import_packed_device": ["mld_tracks* tr", "const uint8_t* select", "const int32_t* const* ids",
                                        "const int64_t* n_tracks", "const int64_t* const* offsets", "const float* const* fp",
                                        "const int64_t* n_entries"],
    "mld_tracks_reset_device": ["mld_tracks* tr", "const uint8_t* select"],
    "mld_tracklets_depths_lanes_device": ["mld_ctx* ctx", "int n_seq", "int bank_cur", "const uint8_t* have_last"] + FEATURES +
                                         ["const uint8_t* const* is_new"] + OUTPUTS,
    "mld_tracklets_step_lanes_device": ["mld_ctx* ctx", "mld_tracks* tr", "int bank_cur", "const uint8_t* have_last",
                                        "const uint8_t* restart", "const int32_t* const* ids"] + FEATURES + OUTPUTS,
}


def _declared(code, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
    assert m, name + " is not declared"
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_them_and_the_library_exports_them():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = capi.load()
    for name, args in ARGS.items():
        assert _declared(code, name) == args, name
        assert name in capi.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
    # the scalar calls are the lanes calls with an int in place of the flags (and no restart)
    scalar = _declared(code, "mld_tracklets_depths_device")
    assert scalar == [a if a != "const uint8_t* have_last" else "int have_last" for a in ARGS["mld_tracklets_depths_lanes_device"]]
    scalar = _declared(code, "mld_tracklets_step_device")
    assert scalar == [a if a != "const uint8_t* have_last" else "int have_last"
                      for a in ARGS["mld_tracklets_step_lanes_device"] if a != "const uint8_t* restart"]
    assert lib.mld_abi_version() == 8
    # deviations and bounds are stated where the caller reads them
    doc = header[header.index("mld_tracks_import_packed_device:"):]
    doc = doc[:doc.index("mld_tracks_counts:")]
    for word in ("select", "n_entries", "clamped", "max_history", "bit for bit", "MLD_ERR_CAPACITY", "abandoned", "repeated id"):
        assert word in doc, word


def test_calls_without_a_store_or_context_are_refused():
    lib = capi.load()
    tab = (C.c_void_p * 1)(None)
    n = (C.c_int64 * 1)(0)
    flag = (C.c_uint8 * 1)(1)
    bad = capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_import_packed_device(None, flag, tab, n, tab, tab, n) == bad
    assert lib.mld_tracks_import_packed_device(None, None, None, None, None, None, None) == bad
    assert lib.mld_tracks_reset_device(None, flag) == bad
    assert lib.mld_tracks_reset_device(None, None) == bad
    assert lib.mld_tracklets_depths_lanes_device(None, 1, 0, flag, tab, tab, tab, tab, tab, n, tab, tab, None, None) == bad
    assert lib.mld_tracklets_step_lanes_device(None, None, 0, flag, None, tab, tab, tab, tab, tab, n, tab, tab, None, None) == bad


def test_the_python_classes_offer_the_methods():
    import inspect
    assert callable(TrackletStore.import_packed) and callable(TrackletStore.reset)
    assert list(inspect.signature(TrackletStore.import_packed).parameters) == ["self", "ids", "offsets", "fp", "select"]
    assert callable(TrackletBatch.set_previous)
    assert list(inspect.signature(TrackletBatch.set_previous).parameters) == ["self", "lane", "cloud", "coeffs", "mask"]
    for method in (TrackletBatch.step, TrackletBatch.run):
        p = inspect.signature(method).parameters
        assert "restart" in p and p["restart"].default is None
    # the per-lane bookkeeping: alike lanes and no restart make today's scalar call, anything else the lanes call
    tb = TrackletBatch.__new__(TrackletBatch)  # (no context: only the bookkeeping)
    tb.S, tb.lane_has_last = 3, [False] * 3
    assert tb.have_last is False and tb._lane_flags(None) == (False, None, None)
    tb.have_last = True
    assert tb.lane_has_last == [True] * 3 and tb._lane_flags([0, 0, 0]) == (True, None, None)
    uniform, last, again = tb._lane_flags([0, 1, 0])
    assert uniform is None and list(last) == [1, 0, 1] and list(again) == [0, 1, 0]
    tb.lane_has_last = [True, False, True]
    uniform, last, again = tb._lane_flags(None)
    assert tb.have_last is False and uniform is None and list(last) == [1, 0, 1] and again is None


def test_the_restatement_reproduces_itself():
    track_import_restatement.self_test()
