"""assignLabels (matches_conversion_ros_tool/src/semantic_labels/semantic_labels.cpp:50-72) restated in plain Python /
NumPy, with the three cases the reference leaves undefined defined as include/mld.h states them.  TEST INFRASTRUCTURE:
written to be read, one loop per track; tests/test_labels_cpu.py checks it against hand-written vectors.

Per track, with p = ((int)u, (int)v) (C++ truncation toward zero) and integer w / 2, h / 2:
    columns [max(0, p.x - w/2), min(cols, p.x + w/2)),  rows [max(0, p.y - h/2), min(rows, p.y + h/2))
    label = the most frequent uchar value in that window
  ties            the smallest label among the most frequent
  empty window    label -2, votes (0, 0)
  u or v NaN, +-inf or beyond the range of int: an empty window
Python's integers do not overflow, so p +- w/2 is exact for every finite float.
"""
import math

import numpy as np

NO_LABEL = -2


def to_int(x):
    """(int)x of a float32, or None where C++ leaves the conversion undefined."""
    x = float(np.float32(x))
    if not math.isfinite(x) or not -2**31 <= x < 2**31:
        return None
    return int(x)  # (truncates toward zero)


def window(rows, cols, roi, u, v):
    """(row0, row1, col0, col1) of the clipped window, or None when it is empty."""
    px, py = to_int(u), to_int(v)
    if px is None or py is None:
        return None
    half_w, half_h = int(roi[0]) // 2, int(roi[1]) // 2
    col0, col1 = max(0, px - half_w), min(cols, px + half_w)
    row0, row1 = max(0, py - half_h), min(rows, py + half_h)
    if col0 >= col1 or row0 >= row1:
        return None
    return row0, row1, col0, col1


def assign_labels(image, roi, u, v):
    """image: [rows, cols] uint8; roi: (width, height); u, v: float32 [n].  Returns
    labels int16 [n], votes int32 [n, 2] (count of the winner, pixels in the window) and tied bool [n] (more than one
    label had the highest count)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    n = len(u)
    labels = np.full(n, NO_LABEL, dtype=np.int16)
    votes = np.zeros((n, 2), dtype=np.int32)
    tied = np.zeros(n, dtype=bool)
    for i in range(n):
        win = window(image.shape[0], image.shape[1], roi, u[i], v[i])
        if win is None:
            continue
        row0, row1, col0, col1 = win
        counts = np.bincount(image[row0:row1, col0:col1].ravel(), minlength=256)
        best = int(counts.max())
        labels[i] = int(np.flatnonzero(counts == best)[0])  # the smallest label with the highest count
        votes[i] = best, (row1 - row0) * (col1 - col0)
        tied[i] = int((counts == best).sum()) > 1
    return labels, votes, tied
