"""mld_feature_traces_collect_*_device (FeatureTraces, TrackletBatch.traces) against the restatement built from the oracle
(feature_trace_restatement.py) and against the product's own depth calls: every comparison is of integers or of raw float
bits; there is no tolerance anywhere.  Every output array lies between guard words, and the rows of the lists are checked
whole: what a call must not touch still holds the guard pattern.

List lengths and what they reach (a ballot takes 64 window cells or list entries):
  0, 1, 2, 3          the sparse cloud: empty lists, no triangle
  63, 64, 65, .. 78   the dense cloud with an 8 x 8 search area: a ballot not full / full / a second one
  129 .. 205          its wide window (17 x 13 cells): a third and a fourth ballot
"""
import collections
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import CameraPinhole, FeatureTraces, GroundPlane, TrackletBatch, capi, synth

import feature_trace_restatement as R
from helpers import kitti_camera, make_estimator

pytestmark = pytest.mark.gpu

GUARD = 0x5A5AA5A5
LEAD, PAD = 2, 4  # guard words before (8-byte alignment kept) and after every array
SMALL_CAM = CameraPinhole(64, 64, 64.0, 32.0, 32.0)
SMALL_T = np.eye(4)[:3].copy()  # x_cam = x_lidar, exactly
WORDS = 46  # int32 words of a record

C0 = capi.params_c0()
VARIANTS = {
    "c0": C0,
    "search_8x8": C0.replace(pixelarea_search_witdh=8, pixelarea_search_height=8),
    "no_histogram": C0.replace(do_use_histogram_segmentation=0),
    "no_trimax": C0.replace(do_use_triangle_size_maximation=0),
    "no_planar_check": C0.replace(do_check_triangleplanar_condition=0),
    "orthogonality_off": C0.replace(viewray_plane_orthoganality_treshold=0.0),
    "orthogonality_high": C0.replace(viewray_plane_orthoganality_treshold=0.999),
    "dispose_relative": C0.replace(treshold_depth_mode=0, treshold_depth_local_mode=0, treshold_depth_local_valuetype=1,
                                   treshold_depth_local_value=0.05, treshold_depth_min=9, treshold_depth_max=11),
    "dispose_absolute": C0.replace(treshold_depth_mode=0, treshold_depth_local_mode=0, treshold_depth_local_valuetype=0,
                                   treshold_depth_local_value=0.01, treshold_depth_min=9, treshold_depth_max=11),
    "adjust_relative": C0.replace(treshold_depth_mode=1, treshold_depth_local_mode=1, treshold_depth_local_valuetype=1,
                                  treshold_depth_local_value=0.05, treshold_depth_min=9, treshold_depth_max=11),
    "adjust_absolute": C0.replace(treshold_depth_mode=1, treshold_depth_local_mode=1, treshold_depth_local_valuetype=0,
                                  treshold_depth_local_value=0.01, treshold_depth_min=9, treshold_depth_max=11),
    "count_min_3_no_cut": C0.replace(radiusSearch_count_min=3, do_use_cut_behind_camera=0, histogram_segmentation_min_pointcount=1),
}

CLOUDS = {"sparse": R.sparse_cloud, "dense": R.dense_cloud, "empty": lambda: np.zeros((0, 4), np.float32)}
_FRAMES, _TRACES = {}, {}


def frame(variant, cloud, plane="half"):
    """The restated frame of a small cloud under a parameter variant; made once and shared.  plane: None, "half" (z =
    10.3 m, a random half of the cloud), "zero" (no inlier), "shifted" (z = 15.3 m, every point an inlier)."""
    key = (variant, cloud, plane)
    if key not in _FRAMES:
        cl = CLOUDS[cloud]()
        gp = None
        if plane == "half":
            gp = R.small_plane(cl)
        elif plane == "zero":
            gp = (R.small_plane(cl)[0], np.zeros(0, np.int32))
        elif plane == "shifted":
            gp = (R.small_plane(cl, offset=15.3)[0], np.arange(cl.shape[0], dtype=np.int32))
        _FRAMES[key] = R.Restatement(VARIANTS[variant], cl, gp, SMALL_CAM, SMALL_T)
    return _FRAMES[key]


def expected(key, fr, uv):
    """(records, lists) of the restatement; computed once per key and left unchanged."""
    if key not in _TRACES:
        rec, lists, _ = fr.trace(uv)
        rec.setflags(write=False)
        _TRACES[key] = (rec, lists)
    return _TRACES[key]


@pytest.fixture(scope="module")
def small_est():
    e = make_estimator(C0, camera=SMALL_CAM, T=SMALL_T, max_frames=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def objects(small_est):
    """FeatureTraces objects on the small camera, one per (variant, n_seq): the parameters are copied at creation."""
    made = {}

    def get(variant, n_seq):
        if (variant, n_seq) not in made:
            made[(variant, n_seq)] = FeatureTraces(small_est, n_seq, 1024, parameters=VARIANTS[variant])
        return made[(variant, n_seq)]

    yield get
    for ft in made.values():
        ft.close()


class Guarded:
    """`words` int32 words between guard words, all of them the guard pattern before the call."""

    def __init__(self, words, dev):
        import torch
        self.words = words
        self.buf = torch.full((LEAD + words + PAD,), GUARD, dtype=torch.int32, device=dev)

    def view(self, dtype):
        return self.buf[LEAD:LEAD + self.words].view(dtype)

    def read(self):
        """(payload as int32 words, guards before and after untouched)"""
        whole = self.buf.cpu().numpy()
        ok = bool((whole[:LEAD] == GUARD).all() and (whole[LEAD + self.words:] == GUARD).all())
        return whole[LEAD:LEAD + self.words].copy(), ok


def upload(fr, dev, plane=True):
    """The device arrays of a restated frame, as mld_projected_clouds_export_device writes them."""
    import torch
    words = fr.mask_words() if plane else None
    return dict(map=torch.from_numpy(fr.pixel_map.reshape(-1).copy()).to(dev),
                index=torch.from_numpy(fr.index.copy()).to(dev) if fr.index.size else None,
                cam=torch.from_numpy(fr.cam.copy()).to(dev) if fr.cam.size else None,
                mask=torch.from_numpy(words.view(np.int32).copy()).to(dev) if words is not None and words.size else None,
                coeffs=np.asarray(fr.plane[0], np.float32) if plane and fr.plane is not None else np.zeros(4, np.float32))


def prepare(frames, uvs, cap, tables=(True, True, True, True), tracks=False, planes=True):
    """The device buffers and the argument list of one call.  frames: per sequence a Restatement; uvs: per sequence
    [n, 2] float64 (n may be 0); tables: per list False (null table), True, or a list of S booleans; planes: False (coeffs
    and masks NULL) or True (a sequence whose frame has no plane gets a NULL mask).  The buffers are made on torch's
    stream, which nothing orders against the context's: torch.cuda.synchronize() before the call."""
    import torch
    dev = torch.device("cuda:0")
    S = len(frames)
    ns = [int(uv.shape[0]) for uv in uvs]
    d = [upload(fr, dev, planes) for fr in frames]
    if tracks:
        feats = ([torch.from_numpy(uv[:, 0].astype(np.float32)).to(dev) if len(uv) else None for uv in uvs],
                 [torch.from_numpy(uv[:, 1].astype(np.float32)).to(dev) if len(uv) else None for uv in uvs])
    else:
        feats = ([torch.from_numpy(np.ascontiguousarray(uv)).to(dev) if len(uv) else None for uv in uvs],)
    g = dict(trace=[Guarded(WORDS * n, dev) for n in ns])
    for name, flag in zip(R.LISTS, tables):
        want = [bool(flag) if isinstance(flag, bool) else bool(flag[s]) for s in range(S)]
        g[name] = None if flag is False else [Guarded(cap * n, dev) if want[s] else None for s, n in enumerate(ns)]
    tab = lambda gs, dt: None if gs is None else [x.view(dt) if x is not None and x.words else None for x in gs]  # noqa: E731
    kw = dict(coeffs=np.stack([x["coeffs"] for x in d]) if planes else None, masks=[x["mask"] for x in d] if planes else None,
              list_capacity=cap, **{name: tab(g[name], torch.int32) for name in R.LISTS})
    args = feats + ([x["map"] for x in d], [x["index"] for x in d], [x["cam"] for x in d], tab(g["trace"], torch.int64))
    return dict(ns=ns, cap=cap, g=g, args=args, kw=kw, tracks=tracks, keep=d)


def issue(ft, q):
    """Queues the call on the context's stream.  No synchronisation."""
    (ft.collect_tracks if q["tracks"] else ft.collect)(*q["args"], **q["kw"])


def collect(q):
    """Per sequence: the records, the rows of every list ([n, cap] int32, None where not asked for), guards untouched."""
    out = []
    for s, n in enumerate(q["ns"]):
        words, ok = q["g"]["trace"][s].read()
        r = dict(rec=words.view(R.DTYPE) if n else np.zeros(0, R.DTYPE), guards=ok)
        for name in R.LISTS:
            r[name] = None
            gs = q["g"][name]
            if gs is not None and gs[s] is not None:
                rows, ok = gs[s].read()
                r[name] = rows.reshape(n, q["cap"])
                r["guards"] = r["guards"] and ok
        out.append(r)
    return out


def rows_of(lists, name, cap):
    """What the rows of a list must hold: the first min(count, cap) entries, the guard pattern behind them."""
    want = np.full((len(lists), cap), GUARD, dtype=np.int32)
    for i, ls in enumerate(lists):
        m = min(ls[name].size, cap)
        want[i, :m] = ls[name][:m]
    return want


def run(ft, q):
    import torch
    torch.cuda.synchronize()
    issue(ft, q)
    ft._est.synchronize()
    return collect(q)


def check(got, want_rec, want_lists, cap, what=""):
    assert got["guards"], what
    assert R.same_records(got["rec"], want_rec) == [], what
    for name in R.LISTS:
        if got[name] is not None:
            assert np.array_equal(got[name], rows_of(want_lists, name, cap)), (what, name)


FEATURE_COUNTS = (0, 1, 63, 64, 65, 257)


def _small_batch(n_seq):
    """n_seq sequences over the sparse, the empty and the dense cloud, their feature counts cycling through
    FEATURE_COUNTS; every third sequence without a plane."""
    kinds = ("sparse", "empty", "dense")
    seqs = []
    for s in range(n_seq):
        kind = kinds[s % 3] if n_seq > 1 else "sparse"
        n = FEATURE_COUNTS[(s + (5 if n_seq == 1 else 2)) % len(FEATURE_COUNTS)]
        plane = None if s % 3 == 2 and s > 2 else "half"
        seqs.append((kind, plane, n, s))
    return seqs


@pytest.mark.parametrize("n_seq", [1, 2, 13])
def test_small_shapes_equal_the_restatement(objects, n_seq):
    """Sequences of 0, 1, 63, 64, 65 and 257 features - on the borders and corners of the image, outside it, NaN and
    +-inf among them - over a sparse, an empty and a dense cloud, one sequence of the larger batch without a mask."""
    seqs = _small_batch(n_seq)
    assert n_seq < 13 or ({n for _, _, n, _ in seqs} == set(FEATURE_COUNTS) and any(p is None for _, p, _, _ in seqs))
    frames = [frame("c0", kind, plane) for kind, plane, _, _ in seqs]
    uvs = [R.small_features(n, seed=s) for _, _, n, s in seqs]
    got = run(objects("c0", n_seq), prepare(frames, uvs, 96))
    seen = collections.Counter()
    for (kind, plane, n, s), fr, uv, g in zip(seqs, frames, uvs, got):
        rec, lists = expected(("small", kind, plane, n, s), fr, uv)
        check(g, rec, lists, 96, (kind, plane, n))
        seen.update(rec["n_nb"].tolist())
        if kind == "empty":
            assert (rec["n_nb"] == 0).all() and (rec["main_type"] == 2).all()
        if plane is None:
            assert (rec["road_state"] == R.NOT_REACHED).all()
    assert n_seq == 2 or {0, 1, 2, 3} <= set(seen)


def test_lists_beyond_a_ballot_on_the_dense_cloud(objects):
    """An 8 x 8 search area over one point per pixel: narrow lists of 63, 64, 65 and more entries, wide lists beyond 128,
    segmented lists of 65 and more with corners found - asserted on the oracle's trace, then compared."""
    fr = frame("search_8x8", "dense")
    uv = R.dense_features()
    rec, lists = expected(("dense8",), fr, uv)
    counts = collections.Counter(rec["n_nb"].tolist())
    assert counts[63] and counts[64] and counts[65] and max(counts) > 65 and rec["n_road"].max() > 128
    assert ((rec["n_seg"] >= 65) & (rec["corner_pos"][:, 0] >= 0)).sum() >= 1
    assert {R.NOT_REACHED, R.FAR_NEIGHBOUR, R.FIT} <= set(rec["road_state"].tolist())
    got = run(objects("search_8x8", 1), prepare([fr], [uv], 256))
    check(got[0], rec, lists, 256)


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "search_8x8"])
def test_parameter_variants_equal_the_restatement(objects, variant):
    frames = [frame(variant, "sparse"), frame(variant, "dense")]
    uvs = [R.small_features(129, seed=7), R.small_features(130, seed=8)]
    got = run(objects(variant, 2), prepare(frames, uvs, 80))
    types = set()
    for kind, fr, uv, g in zip(("sparse", "dense"), frames, uvs, got):
        rec, lists = expected(("variant", variant, kind), fr, uv)
        check(g, rec, lists, 80, (variant, kind))
        types |= set(rec["main_type"].tolist())
    assert len(types) >= 3, types  # (an empty class cannot pass silently)
    if variant.startswith("adjust"):
        assert not types & {4, 5, 6, 7}
    if variant.startswith("dispose"):
        assert types & {4, 5, 6, 7}
    if variant == "orthogonality_high":
        assert 11 in types


@pytest.mark.parametrize("plane,planes", [("half", True), ("zero", True), ("shifted", True), ("half", False), (None, True)])
def test_road_states(objects, plane, planes):
    """The synthetic mask; an all-zero mask (every reached feature ends FAR_NEIGHBOUR or FEW_INLIERS); coefficients
    shifted by 5 m with an all-ones mask (every reached feature ends FAR_NEIGHBOUR); coeffs / mask_dev NULL; masks NULL
    entry by entry."""
    variant = "search_8x8"
    fr = frame(variant, "dense", plane)
    bare = frame(variant, "dense", None)
    uv = R.dense_features()
    got = run(objects(variant, 1), prepare([fr], [uv], 224, planes=planes))[0]
    rec, lists = expected(("road", plane if planes else None), fr if planes else bare, uv)
    check(got, rec, lists, 224, (plane, planes))
    reached = rec["road_state"] != R.NOT_REACHED
    if plane is None or not planes:
        assert not reached.any() and (rec["n_road"] == 0).all()
    else:
        assert reached.sum() >= 5 and (rec["road_state"] != R.FEW_NEIGHBOURS).all()
    if plane == "zero":
        assert np.isin(rec["road_state"][reached], (R.FAR_NEIGHBOUR, R.FEW_INLIERS)).all() and (rec["n_road_inl"] == 0).all()
        assert (rec["road_state"] == R.FEW_INLIERS).sum() >= 1
    if plane == "shifted":
        assert (rec["road_state"][reached] == R.FAR_NEIGHBOUR).all()
    if plane == "half" and planes:
        assert (rec["road_state"] == R.FIT).sum() >= 1 and (rec["n_road_inl"] > 64).any()


def test_tracks_form_equals_the_f64_form_on_the_truncated_coordinates(objects):
    fr = frame("c0", "dense")
    uv = R.small_features(200, seed=11)
    uv[20:60] += 0.37  # (fractions that the truncation drops)
    uv[25] = (-0.5, 3.9)  # truncates to (-0, 3)
    uv32 = uv.astype(np.float32)
    with np.errstate(invalid="ignore"):
        trunc = np.trunc(uv32.astype(np.float64))
    assert (trunc != uv).any()
    ft = objects("c0", 1)
    a = run(ft, prepare([fr], [uv32.astype(np.float64)], 80, tracks=True))[0]
    b = run(ft, prepare([fr], [trunc], 80))[0]
    rec, lists = expected(("tracks",), fr, trunc)
    check(a, rec, lists, 80, "tracks")
    check(b, rec, lists, 80, "f64")


@pytest.mark.parametrize("cap", [0, 1, 7, 1024])
def test_list_capacity_bounds_every_row(objects, cap):
    """Nothing behind min(count, capacity) is written, the counts stay complete; capacity 0 needs no list array."""
    fr = frame("search_8x8", "dense")
    uv = R.dense_features()[:70]
    rec, lists = expected(("cap",), fr, uv)
    assert rec["n_nb"].max() > 7 and rec["n_road"].max() > 7
    got = run(objects("search_8x8", 1), prepare([fr], [uv], cap, tables=(True, True, True, True) if cap else (False,) * 4))[0]
    check(got, rec, lists, cap, cap)
    assert cap == 0 or got["nb"].shape == (70, cap)


def test_optional_tables_absent_as_a_whole_and_per_entry(objects):
    frames = [frame("c0", "dense"), frame("c0", "sparse"), frame("c0", "dense")]
    uvs = [R.small_features(65, seed=s) for s in range(3)]
    ft = objects("c0", 3)
    for tables in ((True, False, True, False), (False, True, False, True), ([1, 0, 1], [0, 1, 1], [0, 0, 0], [1, 1, 0])):
        got = run(ft, prepare(frames, uvs, 40, tables=tables))
        for s, g in enumerate(got):
            rec, lists = expected(("optional", s), frames[s], uvs[s])
            check(g, rec, lists, 40, (tables, s))
            for name, flag in zip(R.LISTS, tables):
                assert (g[name] is not None) == (bool(flag) if isinstance(flag, bool) else bool(flag[s]))


def test_bad_map_and_index_values_count_as_empty_cells(objects):
    """Map values >= index_len and < -1, and index values >= n_points, that still point INSIDE the allocations: a missing
    check shows as a wrong record, not as a fault.  Expected: the cell counts as empty and the flag is set - the oracle's
    trace of the cloud WITHOUT those points, its visible indices translated through the original ones."""
    import torch
    dev = torch.device("cuda:0")
    variant = "search_8x8"
    fr = frame(variant, "dense")
    cloud = CLOUDS["dense"]()
    rng = np.random.default_rng(5)
    vis_bad = np.sort(rng.choice(fr.index.size, 90, replace=False))
    how = rng.integers(0, 3, vis_bad.size)  # 0: map >= index_len, 1: map < -1, 2: index >= n_points
    clean = cloud.copy()
    clean[fr.index[vis_bad], :3] = np.nan  # (not visible: the rest of the cloud keeps its original indices)
    plane = R.small_plane(cloud)
    want_fr = R.Restatement(VARIANTS[variant], clean, plane, SMALL_CAM, SMALL_T)
    uv = R.dense_features()
    want, want_lists, _ = want_fr.trace(uv)
    # the device arrays: slack behind (and ahead of) what the host tables declare
    n_vis, n_pts = fr.index.size, fr.n_points
    pm = fr.pixel_map.reshape(-1).copy()
    cells = {int(v): int(np.nonzero(pm == v)[0][0]) for v in vis_bad}
    index = np.concatenate([np.arange(64, dtype=np.int32) % n_pts, fr.index, np.arange(64, dtype=np.int32) % n_pts])
    for v, h in zip(vis_bad, how):
        if h == 0:
            pm[cells[int(v)]] = n_vis + int(rng.integers(0, 64))
        elif h == 1:
            pm[cells[int(v)]] = -2 - int(rng.integers(0, 60))
        else:
            index[64 + v] = n_pts + int(rng.integers(0, 64))
    cam = np.concatenate([fr.cam, fr.cam[:64] + 1.0])
    d_index = torch.from_numpy(index).to(dev)[64:64 + n_vis]
    d_cam = torch.from_numpy(cam).to(dev)[:n_pts]
    q = prepare([fr], [uv], 224)
    q["args"] = (q["args"][0], [torch.from_numpy(pm).to(dev)], [d_index], [d_cam], q["args"][4])
    got = run(objects(variant, 1), q)[0]
    assert got["guards"]
    # the windows that met a bad cell: the narrow one, and the wide one where the road was reached
    u, v = uv[:, 0], uv[:, 1]
    by, bx = np.divmod(np.array([cells[int(x)] for x in vis_bad]), 64)
    finite = np.isfinite(uv).all(axis=1)

    def met(hx, hy):
        with np.errstate(invalid="ignore"):
            x0, x1 = np.maximum(u - hx, 0).astype(int), np.minimum(u + hx, 63).astype(int)
            y0, y1 = np.maximum(v - hy, 0).astype(int), np.minimum(v + hy, 63).astype(int)
        inside = (bx[None] >= x0[:, None]) & (bx[None] <= x1[:, None]) & (by[None] >= y0[:, None]) & (by[None] <= y1[:, None])
        return inside.any(axis=1) & finite

    flag = met(4.0, 4.0) | (met(8.0, 6.0) & (want["road_state"] != R.NOT_REACHED))
    assert flag.sum() >= 20 and (~flag).sum() >= 20
    want = want.copy()
    want["flags"] |= np.where(flag, R.BAD_INPUT, 0).astype(np.int32)
    # visible indices -> original indices on both sides
    to_orig = lambda idx, arr: np.where(arr >= 0, idx[np.clip(arr, 0, idx.size - 1)], -1)  # noqa: E731
    rec = got["rec"].copy()
    rec["corner_vis"] = to_orig(fr.index, rec["corner_vis"])
    want["corner_vis"] = to_orig(want_fr.index, want["corner_vis"])
    assert R.same_records(rec, want) == []
    for name in ("seg", "road_inl"):
        assert np.array_equal(got[name], rows_of(want_lists, name, 224)), name
    for name in ("nb", "road"):
        mine, theirs = got[name], rows_of(want_lists, name, 224)
        written = theirs != GUARD
        assert np.array_equal(mine != GUARD, written), name
        assert np.array_equal(fr.index[mine[written]], want_fr.index[theirs[written]]), name


def test_two_calls_back_to_back_and_a_reused_array(objects):
    """Two calls queued without a synchronise between them; the second writes the arrays of the first: every record is
    overwritten completely, and a row keeps behind the second call's entries what the first call's longer list left."""
    import torch
    ft = objects("c0", 1)
    fa, fb = frame("c0", "dense"), frame("c0", "sparse")
    uva, uvb = R.small_features(100, seed=21), R.small_features(100, seed=22)
    qa, qb = prepare([fa], [uva], 80), prepare([fb], [uvb], 80)
    qb["g"], qb["kw"] = qa["g"], dict(qb["kw"], **{name: qa["kw"][name] for name in R.LISTS})
    qb["args"] = qb["args"][:4] + (qa["args"][4],)
    torch.cuda.synchronize()
    issue(ft, qa)
    issue(ft, qb)
    ft._est.synchronize()
    got = collect(qb)[0]
    ra, la = expected(("b2b", "a"), fa, uva)
    rb, lb = expected(("b2b", "b"), fb, uvb)
    assert got["guards"] and R.same_records(got["rec"], rb) == []
    assert (ra["n_nb"] > rb["n_nb"]).any()
    for name in R.LISTS:  # the second call's entries in front, behind them what the first call left
        first, second = rows_of(la, name, 80), rows_of(lb, name, 80)
        assert np.array_equal(got[name], np.where(second != GUARD, second, first)), name


@pytest.fixture(scope="module")
def hdl64():
    """One HDL-64 frame, 600 features, C0: the restatement, made once."""
    cloud = synth.make_cloud(synth.HDL64_KITTI, seed=31, frame=2)
    plane = synth.make_ground_plane(cloud)
    uv = synth.make_features(600, seed=31)
    fr = R.Restatement(C0, cloud, plane)
    rec, lists, final = fr.trace(uv)
    return dict(cloud=cloud, plane=plane, uv=uv, fr=fr, rec=rec, lists=lists, final=final)


def test_hdl64_frame_against_the_restatement_and_the_product(hdl64):
    """The records and lists equal the restatement; the product on the same frame agrees with what a record implies; the
    corners equal mld_calculate_depth_debug's, NaN pattern included."""
    import torch
    h = hdl64
    rec, fr, uv = h["rec"], h["fr"], h["uv"]
    states, types = collections.Counter(rec["road_state"].tolist()), collections.Counter(rec["main_type"].tolist())
    assert states[R.NOT_REACHED] >= 5 and states[R.FIT] >= 5 and states[R.FAR_NEIGHBOUR] >= 5
    assert all(types[t] >= 5 for t in (1, 2, 3, 8, 9, 11))
    est = make_estimator(C0, max_frames=1)
    try:
        ft = FeatureTraces(est, 1, 600)
        got = run(ft, prepare([fr], [uv], 32))[0]
        check(got, rec, h["lists"], 32, "hdl64")
        # the product: mld_calculate_depths_device on the slot that holds the frame
        dev = torch.device("cuda:0")
        est.setInputCloud(h["cloud"], GroundPlane(*h["plane"]))
        depth = torch.empty(600, dtype=torch.float64, device=dev)
        types_d = torch.empty(600, dtype=torch.int32, device=dev)
        est.CalculateDepths([torch.from_numpy(uv).to(dev)], [depth], [types_d])
        est.synchronize()
        depth, types_d = depth.cpu().numpy(), types_d.cpu().numpy()
        g = got["rec"]
        fit = g["road_state"] == R.FIT
        assert np.array_equal(types_d[~fit], g["main_type"][~fit])
        implied = np.where(g["road_state"] == R.NOT_REACHED, g["main_depth"], -1.0)
        assert np.array_equal(depth[~fit].view(np.int64), implied[~fit].view(np.int64))
        assert np.isin(types_d[fit], (16, 4, 5, 6, 7)).all() and fit.sum() >= 5
        # the one-slot debug call
        est.ActivateDebugMode()
        est.CalculateDepth(uv)
        corners = est.getTriangleCorners()
        assert np.array_equal(np.isnan(corners), np.isnan(g["corners"]))
        assert np.array_equal(corners.view(np.int64)[~np.isnan(corners)], g["corners"].view(np.int64)[~np.isnan(corners)])
        assert (~np.isnan(corners[:, 0])).sum() >= 50
        ft.close()
    finally:
        est.close()


def test_three_collinear_neighbours_take_the_degenerate_plane_like_the_depth_call():
    """16 x 16, one sequence, one feature whose narrow window holds exactly three points on a line: Hyperplane::Through
    takes its smallest-eigenvector branch.  main_type and main_depth equal mld_calculate_depths_device on the same cloud,
    bit for bit."""
    import torch
    P, cl = R.collinear_parameters(), R.collinear_cloud()
    cam = CameraPinhole(*R.COLLINEAR_CAM)
    uv = np.array([R.COLLINEAR_PIXEL], dtype=np.float64)
    fr = R.Restatement(P, cl, None, cam, SMALL_T)
    est = make_estimator(P, camera=cam, T=SMALL_T, max_frames=1)
    try:
        ft = FeatureTraces(est, 1, 1)
        got = run(ft, prepare([fr], [uv], 8, planes=False))[0]
        assert got["guards"]
        g = got["rec"][0]
        assert (g["n_nb"], g["n_seg"], g["road_state"]) == (3, 3, R.NOT_REACHED) and g["corner_pos"].tolist() == [0, 2, 1]
        c = g["corners"].reshape(3, 3)
        assert np.array_equal(np.cross(c[2] - c[0], c[1] - c[0]), np.zeros(3))  # (the triangle is degenerate exactly)
        dev = torch.device("cuda:0")
        est.setInputCloud(cl)
        depth = torch.empty(1, dtype=torch.float64, device=dev)
        types = torch.empty(1, dtype=torch.int32, device=dev)
        est.CalculateDepths([torch.from_numpy(uv).to(dev)], [depth], [types])
        est.synchronize()
        depth, types = depth.cpu().numpy(), types.cpu().numpy()
        print(f"collinear: depth call type {types[0]} depth {depth[0]!r}; trace type {g['main_type']} depth {g['main_depth']!r} "
              f"plane {g['plane_n'].tolist()} {g['plane_offset']!r}")
        assert g["main_type"] == types[0]
        assert np.array_equal(np.array([g["main_depth"]]).view(np.int64), depth.view(np.int64))
        ft.close()
    finally:
        est.close()


@pytest.mark.parametrize("tracks", [False, True])
def test_the_exits_of_the_main_path_without_histogram_and_triangle_maximisation(tracks):
    """16 x 16, one sequence, histogram segmentation and triangle maximisation off, radiusSearch_count_min 2, a 2 x 2 search
    area (windows of 3 x 3 cells).  A window of two returns leaves at DepthEstimator.cpp:920-921 - the type of a failed
    histogram, but n_seg 2 and its seg row written; a window of three takes the corners (0, 1, 2); windows of one return and
    of none fail the count test.  With a plane, so the road stage follows the exit.  Records and rows equal the
    restatement, between guard words."""
    P = C0.replace(do_use_histogram_segmentation=0, do_use_triangle_size_maximation=0, radiusSearch_count_min=2,
                   pixelarea_search_witdh=2, pixelarea_search_height=2)
    cam = CameraPinhole(*R.COLLINEAR_CAM)
    pixels = np.array([(2, 2), (3, 2), (9, 2), (10, 2), (10, 3), (3, 10)], dtype=np.float64)
    z = np.array([10.0, 10.25, 10.0, 10.125, 10.25, 10.0])
    cl = np.zeros((6, 4), dtype=np.float32)
    cl[:, 0], cl[:, 1], cl[:, 2] = (pixels[:, 0] + 0.5 - 8.0) / 16.0 * z, (pixels[:, 1] + 0.5 - 8.0) / 16.0 * z, z
    plane = (np.array([0.0, 0.0, 1.0, -10.125], dtype=np.float32), np.arange(6, dtype=np.int32))
    uv = np.array([(2, 2), (10, 2), (3, 10), (12, 12)], dtype=np.float64)
    fr = R.Restatement(P, cl, plane, cam, SMALL_T)
    rec, lists, _ = fr.trace(uv)
    assert rec["n_nb"].tolist() == [2, 3, 1, 0] and rec["n_seg"].tolist() == [2, 3, 0, 0]
    assert rec["main_type"][[0, 2, 3]].tolist() == [3, 2, 2] and rec["corner_pos"].tolist() == [[-1] * 3, [0, 1, 2], [-1] * 3, [-1] * 3]
    assert lists[0]["seg"].tolist() == [0, 1] and rec["road_state"][0] != R.NOT_REACHED
    est = make_estimator(P, camera=cam, T=SMALL_T, max_frames=1)
    try:
        ft = FeatureTraces(est, 1, 4)
        check(run(ft, prepare([fr], [uv], 4, tracks=tracks))[0], rec, lists, 4, tracks)
        ft.close()
    finally:
        est.close()


def test_tracklet_batch_traces_runs_on_the_exported_clouds(hdl64):
    """TrackletBatch.traces on the products of projected_clouds(cam=True, pixel_map=True) and the planes of the frame
    table: the records of the integer-pixel features equal the restatement."""
    import torch
    h = hdl64
    dev = torch.device("cuda:0")
    uv = np.floor(h["uv"][:300])
    rec, lists, _ = h["fr"].trace(uv)
    tb = TrackletBatch(C0, kitti_camera(), synth.T_CAM_LIDAR, 1, 300)
    try:
        tb.attach_projected_clouds(h["cloud"].shape[0])
        tb.attach_traces()
        cloud = torch.from_numpy(h["cloud"]).to(dev)
        mask = torch.from_numpy(h["fr"].mask_words().view(np.int32).copy()).to(dev)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
        u, v = f32(uv[:, 0]), f32(uv[:, 1])
        d = [torch.empty(300, dtype=torch.float32, device=dev) for _ in range(2)]
        f = tb.prepare([cloud], np.asarray(h["plane"][0], np.float32)[None], [mask], [u], [v], [u], [v],
                       [torch.zeros(300, dtype=torch.uint8, device=dev)], [d[0]], [d[1]])
        pc = tb.projected_clouds([cloud], cam=True, pixel_map=True)
        out = tb.traces(f, pc, list_capacity=24)
        got = FeatureTraces.records(out["trace"][0])
        assert R.same_records(got, rec) == []
        nb = out["nb"][0].cpu().numpy()
        for i in (0, 17, 299):
            m = min(lists[i]["nb"].size, 24)
            assert np.array_equal(nb[i, :m], lists[i]["nb"][:m])
        bare = FeatureTraces.records(tb.traces(f, pc, planes=False)["trace"][0])
        assert (bare["road_state"] == R.NOT_REACHED).all() and np.array_equal(bare["main_type"], rec["main_type"])
    finally:
        tb.close()
        tb.est.close()


def _tables(S=1):
    tab, zero = (C.c_void_p * S)(*[None] * S), (C.c_int64 * S)(*[0] * S)
    return dict(uv=tab, n=zero, map=tab, index=tab, index_len=zero, cam=tab, n_points=zero, coeffs=None, mask=None, cap=0,
                trace=tab, nb=None, seg=None, road=None, road_inl=None)


ONE = (C.c_int64 * 1)(1)
REFUSALS = [
    (dict(uv=None), capi.MLD_ERR_INVALID_ARG, "null table uv"),
    (dict(n=None), capi.MLD_ERR_INVALID_ARG, "null table n_features"),
    (dict(map=None), capi.MLD_ERR_INVALID_ARG, "null table map"),
    (dict(index=None), capi.MLD_ERR_INVALID_ARG, "null table index"),
    (dict(index_len=None), capi.MLD_ERR_INVALID_ARG, "null table index_len"),
    (dict(cam=None), capi.MLD_ERR_INVALID_ARG, "null table cam"),
    (dict(n_points=None), capi.MLD_ERR_INVALID_ARG, "null table n_points"),
    (dict(trace=None), capi.MLD_ERR_INVALID_ARG, "null table trace_out"),
    (dict(cap=-1), capi.MLD_ERR_INVALID_ARG, "list_capacity"),
    (dict(cap=1025), capi.MLD_ERR_INVALID_ARG, "list_capacity"),
    (dict(coeffs=(C.c_float * 4)()), capi.MLD_ERR_INVALID_ARG, "coeffs and mask_dev"),
    (dict(mask=(C.c_void_p * 1)(None)), capi.MLD_ERR_INVALID_ARG, "coeffs and mask_dev"),
    (dict(n=(C.c_int64 * 1)(-1)), capi.MLD_ERR_INVALID_ARG, "negative n_features"),
    (dict(index_len=(C.c_int64 * 1)(-1)), capi.MLD_ERR_INVALID_ARG, "negative index_len"),
    (dict(n_points=(C.c_int64 * 1)(-1)), capi.MLD_ERR_INVALID_ARG, "negative n_points"),
    (dict(n=(C.c_int64 * 1)(601)), capi.MLD_ERR_CAPACITY, "max_features"),
    (dict(n_points=(C.c_int64 * 1)(8388608)), capi.MLD_ERR_CAPACITY, "8 388 607"),
    (dict(n=ONE), capi.MLD_ERR_INVALID_ARG, "null array uv"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000)), capi.MLD_ERR_INVALID_ARG, "null array map"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000), map=(C.c_void_p * 1)(0x1000)), capi.MLD_ERR_INVALID_ARG, "null array trace_out"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1004), map=(C.c_void_p * 1)(0x1000), trace=(C.c_void_p * 1)(0x1000)),
     capi.MLD_ERR_INVALID_ARG, "uv must be 8-byte aligned"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000), map=(C.c_void_p * 1)(0x1002), trace=(C.c_void_p * 1)(0x1000)),
     capi.MLD_ERR_INVALID_ARG, "map must be 4-byte aligned"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000), map=(C.c_void_p * 1)(0x1000), trace=(C.c_void_p * 1)(0x1004)),
     capi.MLD_ERR_INVALID_ARG, "trace_out must be 8-byte aligned"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000), map=(C.c_void_p * 1)(0x1000), trace=(C.c_void_p * 1)(0x1000),
          index_len=ONE), capi.MLD_ERR_INVALID_ARG, "null array index"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000), map=(C.c_void_p * 1)(0x1000), trace=(C.c_void_p * 1)(0x1000),
          n_points=ONE), capi.MLD_ERR_INVALID_ARG, "null array cam"),
    (dict(n=ONE, uv=(C.c_void_p * 1)(0x1000), map=(C.c_void_p * 1)(0x1000), trace=(C.c_void_p * 1)(0x1000), cap=4,
          seg=(C.c_void_p * 1)(0x1002)), capi.MLD_ERR_INVALID_ARG, "seg_out must be 4-byte aligned"),
]


@pytest.fixture(scope="module")
def kitti_object():
    est = make_estimator(C0, max_frames=1)
    ft = FeatureTraces(est, 1, 600)
    yield ft
    ft.close()
    est.close()


@pytest.mark.parametrize("bad,code,word", REFUSALS, ids=[r[2].replace(" ", "_") for r in REFUSALS])
def test_collect_refuses_with_a_text_that_names_the_function_and_the_argument(kitti_object, bad, code, word):
    """Decided on the host before anything is queued: none of the made-up addresses is touched.  The tracks form is given
    the same tables for u and v, where the refusal does not depend on the element type of the features."""
    ft = kitti_object
    lib = capi.load()
    a = dict(_tables(), **bad)
    rc = lib.mld_feature_traces_collect_device(ft._ft, a["uv"], a["n"], a["map"], a["index"], a["index_len"], a["cam"],
                                               a["n_points"], a["coeffs"], a["mask"], a["cap"], a["trace"], a["nb"], a["seg"],
                                               a["road"], a["road_inl"])
    text = lib.mld_feature_traces_last_error(ft._ft).decode()
    assert rc == code and text.startswith("mld_feature_traces_collect_device: ") and word in text, text
    if "uv" not in word:
        rc = lib.mld_feature_traces_collect_tracks_device(ft._ft, a["uv"], a["uv"], a["n"], a["map"], a["index"],
                                                          a["index_len"], a["cam"], a["n_points"], a["coeffs"], a["mask"],
                                                          a["cap"], a["trace"], a["nb"], a["seg"], a["road"], a["road_inl"])
        text = lib.mld_feature_traces_last_error(ft._ft).decode()
        assert rc == code and text.startswith("mld_feature_traces_collect_tracks_device: ") and word in text, text
    good = _tables()
    assert lib.mld_feature_traces_collect_device(ft._ft, good["uv"], good["n"], good["map"], good["index"], good["index_len"],
                                                 good["cam"], good["n_points"], None, None, 0, good["trace"], None, None, None,
                                                 None) == capi.MLD_OK  # (no features: nothing to do)
