"""The label assignment's C-ABI without a GPU (symbols, refusals before the device is touched, where the source sits)
and the plain-Python restatement of its rules (tests/label_restatement.py) against vectors worked out by hand."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi

from label_restatement import NO_LABEL, assign_labels

ROOT = Path(__file__).resolve().parent.parent

LABEL_SYMBOLS = ("mld_labels_create", "mld_labels_destroy", "mld_labels_last_error", "mld_labels_assign_device")


def test_header_declares_the_labels_and_keeps_the_abi_version():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    lib = capi.load()
    for name in LABEL_SYMBOLS:
        assert name in declared, name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct mld_labels mld_labels;" in code
    assert lib.mld_abi_version() == 8
    # the three places where the reference is undefined are stated where the caller reads them
    assert header.count("DEVIATION (") >= 3
    for word in ("SMALLEST label", "empty window", "-2", "exact integer arithmetic"):
        assert word in header, word


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "SemanticLabels" in m.__all__ and hasattr(m.SemanticLabels, "assign") and hasattr(m.SemanticLabels, "close")
    assert hasattr(m.TrackletBatch, "attach_labels") and hasattr(m.TrackletBatch, "labels")


def test_create_without_a_context_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_labels_create(None, 4, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_labels_last_error(None).decode()
    assert not lib.mld_labels_create(None, 4, None)  # (status_out is optional)


@pytest.mark.parametrize("n_seq", [0, -1, -70000])
def test_create_refuses_a_bad_n_seq_before_it_looks_at_the_context(n_seq):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_labels_create(None, n_seq, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "n_seq" in lib.mld_labels_last_error(None).decode()


def test_assign_on_no_object_is_refused_and_destroy_is_a_no_op():
    lib = capi.load()
    lib.mld_labels_destroy(None)
    lib.mld_labels_destroy(None)
    tab = (C.c_void_p * 1)(None)
    n = (C.c_int64 * 1)(0)
    assert not lib.mld_labels_create(None, 0, None)  # (leaves another text behind)
    assert lib.mld_labels_assign_device(None, tab, 4, 4, 4, 5, 5, tab, tab, n, tab, None) == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_labels_last_error(None).decode()
    assert "mld_labels_assign_device" in text and "null object" in text


def test_the_labels_are_a_translation_unit_of_their_own():
    """In a subdirectory of csrc/ (the files directly in csrc/ seed the randomised sweeps), on the public header only,
    and linked into both libraries."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    assert (csrc / "labels" / "mld_labels.hip").is_file()
    text = (csrc / "labels" / "mld_labels.hip").read_text()
    # public header only: through the shared header of the batch objects, which itself includes nothing else of the project
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h"]
    shared = (csrc / "batch" / "mld_batch_object.h").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', shared) == ["../../../include/mld.h"]
    for src in (text, shared):
        assert '#include "mld_' not in src and "mld_device.h" not in src and "mld_diag.h" not in src
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(LABELS)" in ln and "$(TRACKS)" in ln for ln in link_lines)
    assert re.search(r"^LABELS\s*:=\s*labels/mld_labels\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(LABELS\)", mk, flags=re.M)


# 6 rows x 7 columns; IMAGE[row][column]
IMAGE = np.array([[1, 1, 2, 2, 3, 3, 3],
                  [4, 1, 2, 2, 3, 3, 3],
                  [4, 4, 2, 5, 5, 3, 3],
                  [4, 4, 5, 5, 5, 6, 6],
                  [7, 7, 7, 5, 8, 6, 6],
                  [7, 7, 7, 8, 8, 8, 9]], dtype=np.uint8)

NAN, INF = float("nan"), float("inf")

# (what, roi (w, h), u, v, label, (votes of the winner, pixels in the window))
VECTORS = [
    # roi 5: 5 / 2 = 2, columns [3 - 2, 3 + 2) = 1..4, rows 1..4 - sixteen pixels, not twenty-five, column 5 and row 5
    # are not looked at.  Rows 1..4 of columns 1..4: 1 2 2 3 / 4 2 5 5 / 4 5 5 5 / 7 7 5 8 -> 5 six times
    ("the 4 x 4 window of roi 5, offset to the upper left", (5, 5), 3.0, 3.0, 5, (6, 16)),
    # (int)-0.7 = 0 (floor would give -1 and an empty window [0, 0)), (int)2.9 = 2: columns [0, 1), rows [1, 3):
    # IMAGE[1][0], IMAGE[2][0] = 4, 4
    ("-0.7 truncates to 0, 2.9 to 2", (2, 2), -0.7, 2.9, 4, (2, 2)),
    # (2, 2): columns [1, 3), rows [1, 3): 1 2 / 4 2 -> 2 twice.  (Rounded to (3, 3) it would be 2 5 / 5 5 -> 5.)
    ("2.9, 2.9 truncates to (2, 2)", (2, 2), 2.9, 2.9, 2, (2, 4)),
    # top border: rows [max(0, 1 - 2), 3) = 0..2, columns [2, 6): 2 2 3 3 / 2 2 3 3 / 2 5 5 3 -> 2 five times, 3 five
    # times, 5 twice: a tie of two, the smaller label wins
    ("clipped at the top; a two-way tie, the smaller label wins", (5, 5), 4.0, 1.0, 2, (5, 12)),
    # left border: columns [max(0, 0 - 2), 2) = 0..1, rows 1..4: 4 1 / 4 4 / 4 4 / 7 7 -> 4 five times
    ("clipped at the left", (5, 5), 0.0, 3.0, 4, (5, 8)),
    # right border: columns [4, min(7, 8)) = 4..6, rows [max(0, -1), 3) = 0..2: 3 3 3 / 3 3 3 / 5 3 3 -> 3 eight times
    ("clipped at the right (and the top)", (5, 5), 6.0, 1.0, 3, (8, 9)),
    # bottom border: rows [3, min(6, 7)) = 3..5, columns [0, 4): 4 4 5 5 / 7 7 7 5 / 7 7 7 8 -> 7 six times
    ("clipped at the bottom", (5, 5), 2.0, 5.0, 7, (6, 12)),
    # bottom right corner: columns 4..6, rows 3..5: 5 6 6 / 8 6 6 / 8 8 9 -> 6 four times, 8 three times
    ("clipped at the bottom right corner", (5, 5), 6.0, 5.0, 6, (4, 9)),
    # one pixel left of the image: columns [max(0, -3), 1) = 0, rows 1..4: 4 4 4 7
    ("a point one pixel outside still sees the image", (5, 5), -1.0, 3.0, 4, (3, 4)),
    # roi (4, 2): columns [0, 4), rows [1, 3): 4 1 2 2 / 4 4 2 5 -> 4 three times, 2 three times; 4 is met first in
    # scan order, 2 is smaller and wins
    ("a tie whose larger label comes first", (4, 2), 2.0, 2.0, 2, (3, 8)),
    # 1 / 2 = 0: [p, p) is empty whatever the point
    ("roi 1 is an empty window", (1, 1), 3.0, 3.0, NO_LABEL, (0, 0)),
    ("roi width 1 alone empties the window", (1, 5), 3.0, 3.0, NO_LABEL, (0, 0)),
    ("roi height 0 alone empties the window", (5, 0), 3.0, 3.0, NO_LABEL, (0, 0)),
    # columns [104, min(7, 108)): min >= max
    ("100 px to the right", (5, 5), 106.0, 3.0, NO_LABEL, (0, 0)),
    ("100 px above", (5, 5), 3.0, -100.0, NO_LABEL, (0, 0)),
    # the offset window seen from outside: p = (8, 0), two columns right of the last one, still sees column
    # [8 - 2, min(7, 10)) = 6, rows [max(0, -2), 2) = 0..1: 3 3; p = (-2, 3), two columns left of the first one, sees
    # [max(0, -4), 0): nothing
    ("two pixels right of the last column", (5, 5), 8.0, 0.0, 3, (2, 2)),
    ("two pixels left of the first column", (5, 5), -2.0, 3.0, NO_LABEL, (0, 0)),
    ("NaN u", (5, 5), NAN, 3.0, NO_LABEL, (0, 0)),
    ("NaN v", (5, 5), 3.0, NAN, NO_LABEL, (0, 0)),
    ("+inf u", (5, 5), INF, 3.0, NO_LABEL, (0, 0)),
    ("-inf v", (5, 5), 3.0, -INF, NO_LABEL, (0, 0)),
    ("3e9 is beyond int", (5, 5), 3e9, 3.0, NO_LABEL, (0, 0)),
    ("-3e9 is beyond int, even with a roi that would reach back", (2**31 - 1, 5), -3e9, 3.0, NO_LABEL, (0, 0)),
    # a roi of 2^31 - 1 around an ordinary point: the whole image, exact arithmetic.  The image holds 1 x3, 2 x5, 3 x8,
    # 4 x5, 5 x6, 6 x4, 7 x6, 8 x4, 9 x1 = 42 pixels
    ("the largest roi is the whole image", (2**31 - 1, 2**31 - 1), 3.0, 3.0, 3, (8, 42)),
]


@pytest.mark.parametrize("what,roi,u,v,label,votes", VECTORS, ids=[x[0] for x in VECTORS])
def test_restatement_against_hand_vectors(what, roi, u, v, label, votes):
    got_l, got_v, tied = assign_labels(IMAGE, roi, np.array([u], dtype=np.float32), np.array([v], dtype=np.float32))
    assert got_l.dtype == np.int16 and got_v.dtype == np.int32
    assert int(got_l[0]) == label, what
    assert tuple(int(x) for x in got_v[0]) == votes, what
    assert bool(tied[0]) == bool(re.search(r"\btie\b", what))
