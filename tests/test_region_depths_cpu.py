"""The batched region depths without a GPU: symbols, the record's layout, the refusals of create before the device is
touched, the Python names, where the source sits, and the restatement the GPU tests compare against
(region_depth_restatement) - checked against the oracle's trace at the pixels of two frames, against the reference's own
Histogram object code, and against np.partition / np.sort."""
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi
from oracle import oracle

import coverage_restatement as V
import depth_image_frames as F
import region_depth_restatement as G

ROOT = Path(__file__).resolve().parent.parent

REGION_SYMBOLS = ("mld_region_depths_create", "mld_region_depths_destroy", "mld_region_depths_last_error",
                  "mld_region_depths_collect_device")
# include/mld.h, mld_region_depth: (field, offset, bytes)
LAYOUT = [("n_points", 0, 4), ("n_ground", 4, 4), ("n_seg", 8, 4), ("flags", 12, 4), ("nearest_orig", 16, 4), ("clip", 20, 16),
          ("pad_", 36, 4), ("z_min", 40, 8), ("z_max", 48, 8), ("z_median", 56, 8), ("hist_lower", 64, 8), ("hist_higher", 72, 8)]

ref = oracle.load_reference_parts()
GOLDEN = Path(__file__).resolve().parent / "golden" / "region_depth_reference_parts.npz"
RECORDED = {}   # every answer of the live reference library in this process (what make_region_depth_reference_parts.py stores)


def test_header_capi_and_both_libraries_carry_the_four_symbols():
    """(Fails on the parent commit: the symbols are new.)"""
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in REGION_SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_region_depths mld_region_depths;" in code
    for word in ("64 * n_seq bytes", "16 * 64 * n_seq bytes", "two launches", "ONE BLOCK PER BOX", "no global atomics",
                 "no floating-point accumulation", "MLD_REGION_LIST_CAPACITY", "MLD_REGION_HIST_BINS"):
        assert word in header, word
    for name, value in (("MLD_REGION_FLAG_BAD_INPUT", 1), ("MLD_REGION_FLAG_EMPTY_BOX", 2), ("MLD_REGION_FLAG_HIST_FOUND", 4),
                        ("MLD_REGION_FLAG_HIST_CAPPED", 8), ("MLD_REGION_FLAG_HAS_MASK", 16)):
        assert re.search(rf"\b{name} = {value}\b", code), name
        assert getattr(capi, name) == value
    for name in ("MLD_REGION_LIST_CAPACITY", "MLD_REGION_HIST_BINS"):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", code).group(1)) == getattr(capi, name)
    assert (G.BAD_INPUT, G.EMPTY_BOX, G.HIST_FOUND, G.HIST_CAPPED, G.HAS_MASK) == (1, 2, 4, 8, 16)


def test_the_record_has_the_size_and_the_offsets_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mld_region_depth \{(.*?)\} mld_region_depth;", header, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * int(m.group(2) or 1)))
    offset, laid = 0, []
    for name, size in fields:
        laid.append((name, offset, size))
        offset += size
    assert laid == LAYOUT and offset == 80  # (every field is naturally aligned where it falls: no padding)
    assert C.sizeof(capi.MldRegionDepth) == 80 and C.alignment(capi.MldRegionDepth) == 8
    assert [(n, getattr(capi.MldRegionDepth, n).offset, getattr(capi.MldRegionDepth, n).size)
            for n, _ in capi.MldRegionDepth._fields_] == LAYOUT
    assert G.DTYPE.itemsize == 80 and [(n, G.DTYPE.fields[n][1]) for n in G.DTYPE.names] == [(n, o) for n, o, _ in LAYOUT]
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "regions" / "mld_region_depths.hip").read_text()
    assert "static_assert(sizeof(mld_region_depth) == 80" in source


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "RegionDepths" in m.__all__
    for name in ("collect", "records", "close"):
        assert hasattr(m.RegionDepths, name), name
    assert m.RegionDepths.WORDS * 8 == 80 and m.RegionDepths.DTYPE == G.DTYPE
    assert (m.RegionDepths.LIST_CAPACITY, m.RegionDepths.HIST_BINS) == (capi.MLD_REGION_LIST_CAPACITY, capi.MLD_REGION_HIST_BINS)
    assert hasattr(m.TrackletBatch, "attach_region_depths") and hasattr(m.TrackletBatch, "region_depths")


def _create(ctx, n_seq, max_boxes, P, cam):
    lib = capi.load()
    st = C.c_int(0)
    handle = lib.mld_region_depths_create(ctx, n_seq, max_boxes, C.byref(P) if P is not None else None,
                                          C.byref(cam) if cam is not None else None, C.byref(st))
    assert not handle
    return st.value, lib.mld_region_depths_last_error(None).decode()


@pytest.mark.parametrize("n_seq,max_boxes,word", [(0, 4, "n_seq"), (-1, 4, "n_seq"), (65537, 4, "n_seq"), (4, 0, "max_boxes"),
                                                  (4, -3, "max_boxes")])
def test_create_refuses_a_bad_size_before_it_looks_at_anything_else(n_seq, max_boxes, word):
    code, text = _create(None, n_seq, max_boxes, None, None)
    assert code == capi.MLD_ERR_INVALID_ARG
    assert "mld_region_depths_create" in text and word in text and "context" not in text and "params" not in text


def test_create_judges_its_arguments_before_it_looks_at_the_context():
    """Sizes, then params and camera, the context last: every refusal below is made with a NULL context, which is only
    named when nothing else is wrong."""
    P = capi.params_c0()
    cam = capi.MldCamera(64.0, 32.0, 32.0, 64, 64)
    assert _create(None, 4, 8, None, cam) == (capi.MLD_ERR_INVALID_ARG, "mld_region_depths_create: null params")
    assert _create(None, 4, 8, P, None) == (capi.MLD_ERR_INVALID_ARG, "mld_region_depths_create: null camera")
    for bw in (0.0, -0.3, np.nan, np.inf):
        code, text = _create(None, 4, 8, P.replace(histogram_segmentation_bin_witdh=bw), cam)
        assert code == capi.MLD_ERR_INVALID_ARG and "mld_region_depths_create" in text and "histogram_segmentation_bin_witdh" in text
    code, text = _create(None, 4, 8, P, capi.MldCamera(64.0, 1.0, 1.0, 0, 64))
    assert code == capi.MLD_ERR_INVALID_ARG and "bad image size" in text
    code, text = _create(None, 4, 8, P, capi.MldCamera(64.0, 1.0, 1.0, 65536, 4))
    assert code == capi.MLD_ERR_CAPACITY and "65535" in text
    code, text = _create(None, 65536, 32768, P, cam)
    assert code == capi.MLD_ERR_CAPACITY and "2^31 - 1 blocks" in text
    assert _create(None, 65536, 32767, P, cam) == (capi.MLD_ERR_INVALID_ARG, "mld_region_depths_create: null context")
    # parameters the object does not read are not judged: a search mode mld_create refuses gets as far as the context
    assert _create(None, 4, 8, P.replace(neighbor_search_mode=1, pixelarea_search_witdh=-1), cam)[1].endswith("null context")
    assert not capi.load().mld_region_depths_create(None, 4, 8, None, None, None)  # (status_out is optional)


def test_collect_on_no_object_is_refused():
    lib = capi.load()
    assert not lib.mld_region_depths_create(None, 0, 1, None, None, None)  # (leaves another text behind)
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    rc = lib.mld_region_depths_collect_device(None, tab, tab, zero, tab, zero, None, tab, zero, tab)
    assert rc == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_region_depths_last_error(None).decode() == "mld_region_depths_collect_device: null object (rd)"
    lib.mld_region_depths_destroy(None)


def test_the_region_depths_are_a_translation_unit_of_their_own():
    """In regions/, on the shared batch headers and the public header only, linked into both libraries; no other source
    knows of it; one kernel, two launches with the upload, nothing allocated per call, no global atomics (the atomics
    are integer adds on LDS arrays), no fence."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "regions" / "mld_region_depths.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h",
                                                           "../../../include/mld.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    code = re.sub(r"//.*", "", text)
    assert "asm" not in code and "__threadfence" not in code
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_region_depths"]
    assert len(re.findall(r"hipLaunchKernelGGL\(", text)) == 1  # (+ the descriptor upload: two launches)
    shared = set(re.findall(r"__shared__\s+(?:unsigned long long|int)\s+([^;]+);", code))
    lds = {re.match(r"\w+", item.strip()).group(0) for decl in shared for item in decl.split(",")}
    targets = re.findall(r"atomic\w*\(&(\w+)", code)
    assert targets and set(targets) <= lds, targets
    assert set(re.findall(r"\batomic\w*", code)) == {"atomicAdd"}
    tail = text.split("mld_region_depths_collect_device(")[-1]
    assert "hipMalloc" not in tail and "Synchronize" not in tail
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(REGIONS)" in ln for ln in link_lines)
    assert re.search(r"^REGIONS\s*:=\s*regions/mld_region_depths\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(IMAGES\) \$\(REGIONS\)", mk, flags=re.M)
    for path in csrc.rglob("*"):
        if path.is_file() and path.name != "Makefile" and path.parent.name != "regions":
            assert "mld_region" not in path.read_text(), path.name


# ---- the restatement against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mixed", "golden_c0"])
def test_the_restatement_agrees_with_the_oracles_trace_at_every_pixel_it_scans(which):
    """At every integer pixel, the box equal to the narrow window (the reference's clamp and (int) rule), without a mask:
    n_points is the trace's n_nb everywhere; where the trace ran the histogram - enough neighbours, histogram segmentation
    on - HIST_FOUND, n_seg and the borders are the trace's.  The pixels where the trace never reaches the histogram (type
    2, too few neighbours) are left out of the second part: 25.1 % of the mixed frame (its empty quarter) and 47.7 % of the
    golden frame (a sparse cloud), below one half on both."""
    fr = {"mixed": F.mixed_frame, "golden_c0": F.golden_frame}[which]()
    P = fr.P
    assert P.do_use_histogram_segmentation and not P.set_all_depths_to_zero
    (hx, hy), _ = V.half_sizes(P)
    count_min = int(P.radiusSearch_count_min) & 0xFFFFFFFF
    left_out = found = 0
    for y in range(fr.H):
        for x in range(fr.W):
            t = fr.ref.trace_feature(float(x), float(y))
            nb = t["nb_idx"]
            box = G.window_box(x, y, hx, hy, fr.W, fr.H)
            rec = G.region_record(fr.pm, fr.index, fr.cam, fr.n_points, box, P.histogram_segmentation_bin_witdh,
                                  P.histogram_segmentation_min_pointcount)
            assert rec["n_points"] == nb.size and rec["n_ground"] == 0 and not rec["flags"] & ~G.HIST_FOUND, (x, y)
            assert tuple(rec["clip"]) == box, (x, y)
            if nb.size < count_min:
                assert t["type"] == 2, (x, y)
                left_out += 1
                continue
            z = fr.cam[fr.index[nb], 2]
            assert z.max() < 999.0  # (the depth path's clamp, DepthEstimator.cpp:743, does not act on these frames)
            ok, keep, lo, hi = oracle.filter_points_min_dist_blob(z, P.histogram_segmentation_bin_witdh,
                                                                  P.histogram_segmentation_min_pointcount)
            n_seg = t["seg_pos"].size
            assert bool(rec["flags"] & G.HIST_FOUND) == (n_seg > 0) == ok, (x, y)
            assert rec["n_seg"] == n_seg == keep.size, (x, y)
            assert (rec["hist_lower"], rec["hist_higher"]) == (lo, hi), (x, y)
            assert rec["nearest_orig"] == fr.index[nb[np.argmin(z)]] and rec["z_min"] == z.min() and rec["z_max"] == z.max(), (x, y)
            found += n_seg > 0
    share = left_out / (fr.W * fr.H)
    print(f"{which}: {left_out} of {fr.W * fr.H} pixels never reach the histogram ({100 * share:.1f} %), {found} with a bin")
    assert share < 0.5 and found > 100


# ---- the binning against the reference's own object code --------------------------------------------------------------
def _key(kind, *arrays):
    h = hashlib.sha1(kind.encode())
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return f"{kind}_{h.hexdigest()[:20]}"


def _ref_counts(values, bin_width, bin_count):
    """The bin counts of the reference's Histogram class (oracle/_ref/libmld_ref.so, used as tests/test_reference_parts.py
    uses it): live where the library has been built - and then equal to the stored answer -, else the stored answer for
    exactly these inputs; an input without one fails, never skips."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    key = _key("hist", v, np.float64(bin_width), np.int64(bin_count))
    stored = dict(np.load(GOLDEN)).get(key) if GOLDEN.exists() else None
    if ref is None:
        assert stored is not None, f"{key}: no stored reference answer (tests/golden/make_region_depth_reference_parts.py)"
        return stored
    out = np.zeros(bin_count, dtype=np.int32)
    ref.ref_histogram_counts(v.ctypes.data, v.size, float(bin_width), int(bin_count), out.ctypes.data)
    RECORDED[key] = out
    if stored is not None:
        assert np.array_equal(stored, out), f"{key}: the reference library disagrees with its stored answer"
    return out


def box_sized_list(seed, n, bin_width, z_lo, z_hi):
    """n depths as a box of thousands of cells holds them: uniform in z_lo .. z_hi, a cluster, exact bin edges and the
    values one ulp below them."""
    rng = np.random.default_rng(9100 + seed)
    edges = np.arange(int(z_lo / bin_width) + 1, int(z_hi / bin_width)) * bin_width
    z = np.concatenate([rng.uniform(z_lo, z_hi, n), rng.normal(0.5 * (z_lo + z_hi), 0.2, n // 2).clip(z_lo, z_hi), edges,
                        np.nextafter(edges, 0.0), [z_hi]])
    return rng.permutation(z)


@pytest.mark.parametrize("seed,n,bin_width,z_lo,z_hi", [(0, 3000, 0.3, 2.0, 80.0), (1, 9000, 0.3, 5.0, 119.7), (2, 2500, 0.5, 0.4, 30.0),
                                                         (3, 4000, 0.1, 10.0, 12.0), (4, 2049, 1.0, 1.0, 200.0)])
def test_the_binning_of_box_sized_lists_equals_the_reference_class(seed, n, bin_width, z_lo, z_hi):
    z = box_sized_list(seed, n, bin_width, z_lo, z_hi)
    assert z.size > 2048
    bin_count = G.histogram_frame(float(z.max()), bin_width)
    assert bin_count == int(int(np.ceil(z.max())) / bin_width + 1) > 1
    assert np.array_equal(G.bin_counts(z, bin_width, bin_count), _ref_counts(z, bin_width, bin_count))
    # and the borders of the restatement are those of the oracle's FilterPointsMinDistBlob end to end
    for min_count in (0, 3, 40):
        ok, keep, lo, hi = oracle.filter_points_min_dist_blob(z, bin_width, min_count)
        flag, lower, higher = G.blob_borders(z, bin_width, min_count, hist_bins=1 << 20)
        assert (flag == G.HIST_FOUND) == ok and (lower, higher) == (lo, hi), min_count


# ---- order statistics and the cap ---------------------------------------------------------------------------------------
def one_row(z, orig=None):
    """A 1-row image with one point per cell at the depths z (cloud order shuffled): (pixel_map, index, cam, n_points)."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    rng = np.random.default_rng(n)
    orig = rng.permutation(n) if orig is None else np.asarray(orig)
    cam = np.zeros((n, 3))
    cam[orig, 2] = z
    return np.arange(n, dtype=np.int32).reshape(1, n), orig.astype(np.int32), cam, n


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 64, 2047, 2048, 2049, 5000])
def test_median_extremes_and_nearest_point_against_numpy(n):
    """z quantised to 0.25 m: many duplicates.  The median is np.partition's element of rank (n - 1) // 2, an element of the
    set; the nearest point is the first of the smallest in scan order (np.argmin's rule)."""
    rng = np.random.default_rng(n)
    z = np.round(rng.uniform(4.0, 40.0, n) * 4.0) / 4.0
    if n >= 4:
        z[[n // 3, n // 2]] = z.min() - 0.25  # (a tie for the nearest point)
    pm, index, cam, n_points = one_row(z)
    rec = G.region_record(pm, index, cam, n_points, (0, 0, n - 1, 0), 0.3, 3)
    k = (n - 1) // 2
    assert rec["n_points"] == n and rec["z_median"] == np.partition(z, k)[k] == np.sort(z)[k] and rec["z_median"] in z
    assert rec["z_min"] == z.min() and rec["z_max"] == z.max()
    assert rec["nearest_orig"] == index[np.argmin(z)]
    if n >= 4:
        assert rec["nearest_orig"] == index[n // 3]
    # a sub-box: its own rank, its own first minimum
    if n > 4:
        a, b = n // 4, n - 2
        sub = G.region_record(pm, index, cam, n_points, (a, -5, b, 7), 0.3, 3)
        zs = z[a:b + 1]
        assert sub["z_median"] == np.sort(zs)[(zs.size - 1) // 2] and sub["nearest_orig"] == index[a + np.argmin(zs)]
        assert tuple(sub["clip"]) == (a, 0, b, 0)


def test_empty_inverted_and_outside_boxes_and_the_mask():
    z = np.array([9.0, 5.0, 5.0, 7.0, 30.0, 30.1, 30.2])
    pm, index, cam, n_points = one_row(z, orig=[3, 0, 6, 1, 2, 5, 4])
    for box in ((3, 0, 2, 0), (0, 1, 5, 0), (7, 0, 9, 0), (-4, 0, -1, 0), (0, 1, 3, 4), (0, -3, 3, -1)):
        rec = G.region_record(pm, index, cam, n_points, box, 0.3, 1)
        assert rec["flags"] == G.EMPTY_BOX and tuple(rec["clip"]) == (-1,) * 4 and rec["n_points"] == 0 and rec["z_median"] == -1.0
    rec = G.region_record(pm, index, cam, n_points, (-10, -10, 10, 10), 0.3, 1)
    assert rec["nearest_orig"] == 0 and rec["z_median"] == 9.0 and tuple(rec["clip"]) == (0, 0, 6, 0) and rec["n_points"] == 7
    bits = np.zeros(7, dtype=bool)
    bits[[0, 6]] = True  # the two points at 5 m
    rec = G.region_record(pm, index, cam, n_points, (0, 0, 6, 0), 0.3, 1, mask_bits=bits)
    assert rec["flags"] & G.HAS_MASK and rec["n_ground"] == 2 and rec["n_points"] == 5 and rec["z_min"] == 7.0 and rec["nearest_orig"] == 1
    rec = G.region_record(pm, index, cam, n_points, (0, 0, 6, 0), 0.3, 1, mask_bits=np.ones(7, dtype=bool))
    assert rec["n_ground"] == 7 and rec["n_points"] == 0 and rec["z_min"] == -1.0 and rec["flags"] == G.HAS_MASK
    cam_bad = cam.copy()
    cam_bad[3, 2] = np.nan   # the point at 9 m
    cam_bad[1, 2] = -7.0
    rec = G.region_record(pm, index, cam_bad, n_points, (0, 0, 6, 0), 0.3, 1)
    assert rec["flags"] & G.BAD_INPUT and rec["n_points"] == 5 and rec["z_max"] == 30.2


def test_a_run_of_bins_beyond_the_histogram_storage_is_capped_and_one_just_short_is_not():
    """One point in each of k consecutive bins of width 1, minimal count 1: the scan never meets a smaller bin inside the
    run, so it walks to its end.  With the run ending on the last bin (z_max an integer) the scan looks at k bins: k =
    HIST_BINS fits the storage, HIST_BINS + 1 does not.  With an empty bin behind the run (z_max = x.5) the scan looks at
    that one too and ends there: k = HIST_BINS - 1 fits, HIST_BINS does not."""
    for first, k, capped in ((3.0, G.HIST_BINS, False), (3.0, G.HIST_BINS + 1, True), (3.5, G.HIST_BINS - 1, False),
                             (3.5, G.HIST_BINS, True), (3.5, G.HIST_BINS + 40, True)):
        z = first + np.arange(k, dtype=np.float64)
        flag, lo, hi = G.blob_borders(z, 1.0, 1)
        assert (flag == G.HIST_CAPPED) == capped, (first, k)
        if capped:
            assert (lo, hi) == (-1.0, -1.0)
            assert G.blob_borders(z, 1.0, 1, hist_bins=1 << 20) == (G.HIST_FOUND, 3.0, 4.0)
        else:
            assert (flag, lo, hi) == (G.HIST_FOUND, 3.0, 4.0)
        assert (flag, lo, hi) == G.blob_borders(z[::-1], 1.0, 1)
        ok, _, lo, hi = oracle.filter_points_min_dist_blob(z, 1.0, 1)
        assert ok and (lo, hi) == (3.0, 4.0)
    # a decreasing second bin ends the scan at once, however long the run behind it
    z = np.concatenate([[3.1, 3.2], 4.5 + np.arange(2000, dtype=np.float64)])
    assert G.blob_borders(z, 1.0, 2) == (G.HIST_FOUND, 3.0, 4.0)
