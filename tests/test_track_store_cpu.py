"""The tracklet store's C-ABI without a GPU: the symbols exist, creation refuses bad arguments before it touches the
context or the device, destroying nothing is a no-op, and the ABI version did not move."""
import ctypes as C
import re
from pathlib import Path

import pytest

from mono_lidar_depth_amd import capi

ROOT = Path(__file__).resolve().parent.parent

STORE_SYMBOLS = ("mld_tracks_create", "mld_tracks_destroy", "mld_tracks_last_error", "mld_tracks_begin_device",
                 "mld_tracks_commit_device", "mld_tracks_export_device", "mld_tracks_counts", "mld_tracklets_step_device")


def test_header_declares_the_store_and_keeps_the_abi_version():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    lib = capi.load()
    for name in STORE_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct mld_tracks mld_tracks;" in code
    assert lib.mld_abi_version() == 8
    # the deviation from the reference's unbounded deque is stated where the caller reads it
    assert "max_history" in header and "unbounded" in header


def test_create_without_a_context_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_tracks_create(None, 4, 100, 8, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_tracks_last_error(None).decode()
    assert not lib.mld_tracks_create(None, 4, 100, 8, None)  # (status_out is optional)


@pytest.mark.parametrize("n_seq,max_tracks,max_history,word", [(0, 100, 8, "n_seq"), (-3, 100, 8, "n_seq"),
                                                               (4, 0, 8, "max_tracks"), (4, -1, 8, "max_tracks"),
                                                               (4, 100, 1, "max_history"), (4, 100, 0, "max_history"),
                                                               (4, 100, -2, "max_history")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_tracks, max_history, word):
    """The sizes are checked first, so the refusal names the size even without a context - and a context that exists is
    not touched (there is none on a box without a GPU; NULL stands in)."""
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_tracks_create(None, n_seq, max_tracks, max_history, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert word in lib.mld_tracks_last_error(None).decode()


def test_calls_on_no_store_are_refused_and_destroy_is_a_no_op():
    lib = capi.load()
    lib.mld_tracks_destroy(None)
    lib.mld_tracks_destroy(None)
    tab = (C.c_void_p * 1)(None)
    n = (C.c_int64 * 1)(0)
    assert lib.mld_tracks_begin_device(None, tab, n, None) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_commit_device(None, tab, tab, tab, tab, tab, tab) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_export_device(None, tab, tab) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_counts(None, (C.c_int64 * 6)()) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracklets_step_device(None, None, 0, 0, tab, tab, tab, tab, tab, n, tab, tab, None, None) == \
        capi.MLD_ERR_INVALID_ARG


def test_the_store_is_a_translation_unit_of_its_own():
    """It sits in a subdirectory of csrc/ (the depth path's sources, whose hash seeds the randomised sweeps, are the
    files directly in csrc/) and both libraries link it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    assert (csrc / "tracks" / "mld_tracks.hip").is_file()
    text = (csrc / "tracks" / "mld_tracks.hip").read_text()
    # public header only: through the shared header of the batch objects, which itself includes nothing else of the project
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h"]
    shared = (csrc / "batch" / "mld_batch_object.h").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', shared) == ["../../../include/mld.h"]
    for src in (text, shared):
        assert '#include "mld_' not in src and "mld_device.h" not in src and "mld_diag.h" not in src
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(TRACKS)" in ln for ln in link_lines)
    assert re.search(r"^TRACKS\s*:=\s*tracks/mld_tracks\.hip\s*$", mk, flags=re.M)
