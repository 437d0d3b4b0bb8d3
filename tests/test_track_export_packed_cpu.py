"""The packed export of the tracklet store (mld_tracks_export_packed_device) without a GPU: the header declares it, the
library exports it, capi binds it with its four arguments, TrackletStore offers it, a call without a store is refused
and the ABI version did not move."""
import ctypes as C
import re
from pathlib import Path

from mono_lidar_depth_amd import TrackletStore, capi

ROOT = Path(__file__).resolve().parent.parent
NAME = "mld_tracks_export_packed_device"


def test_header_declares_it_and_the_library_exports_it():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, "not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["mld_tracks* tr", "float* const* fp_out", "const int64_t* capacity", "int64_t* const* offsets_out"]
    assert NAME in capi.EXPORTED_SYMBOLS
    lib = capi.load()
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 4
    assert lib.mld_abi_version() == 8
    # what a caller has to know is stated where the caller reads it
    doc = header[header.index(NAME + ":"):]
    for word in ("offsets_out", "capacity", "NULL", "truncat"):
        assert word in doc[:2000], word


def test_a_call_without_a_store_is_refused():
    lib = capi.load()
    tab = (C.c_void_p * 1)(None)
    cap = (C.c_int64 * 1)(0)
    assert lib.mld_tracks_export_packed_device(None, tab, cap, tab) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_export_packed_device(None, None, None, None) == capi.MLD_ERR_INVALID_ARG


def test_the_python_class_offers_it():
    assert callable(TrackletStore.export_packed) and callable(TrackletStore.packed_capacity)
    store = TrackletStore.__new__(TrackletStore)  # (no context: only the arithmetic)
    store.max_history = 16
    assert store.packed_capacity(10000) == 160000 and store.packed_capacity(0) == 0
    store._tr = None  # (what close() leaves; __del__ has nothing to destroy)
