"""mld_depth_reports_collect_device / _collect_tracks_device (DepthReports, TrackletBatch.reports): every comparison is
for EQUALITY, points as raw f64 bits.  Expected points: the NumPy restatement below, (u - cu) / f * d in float64, with
np.trunc(...).astype(float64) for the tracks form.  Expected counts: mld_result_histogram on the host copy of the types
plus a NumPy count of the types out of range.  Neither is the code under test; there is no tolerance.

Feature counts and what they reach (a wavefront takes 64 features, a block 1024):
  0                  no arrays, an all-zero record
  1, 63, 64, 65      one ballot word not full / full / a second one
  1023, 1024, 1025   a second chunk
  4097               a fifth chunk

NaNs are compared as bits like everything else: a NaN coordinate propagates with its bits, and the NaN that inf * 0
generates (an inf coordinate beside a depth of +-0) is the same quiet NaN on the GPU and on the host.
"""
import ctypes as C

import numpy as np
import pytest

from mono_lidar_depth_amd import DepthEstimator, DepthReports, GroundPlane, TrackletBatch, capi, synth

from helpers import kitti_camera, make_estimator

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097)
FORMS = ("f64", "tracks")
GUARD = 0x5A5AA5A5
LEAD, PAD = 2, 4  # guard words before (8-byte alignment kept) and after every array
WORDS = 24        # int64 words of a record
F, CU, CV = synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV


def make_inputs(form, n, seed, layout="mixed"):
    """One sequence: u, v (float64 / float32), depth (float64 / float32), types (int32).
    layout: mixed (-1, positive, NaN, -0.0, +inf, 0), all (every depth positive), none (-1 and NaN only), last (only the
    last feature - the last lane of the last ballot word - has a depth)."""
    rng = np.random.default_rng(seed)
    ft = np.float64 if form == "f64" else np.float32
    u = rng.uniform(-5, synth.KITTI_W + 5, n)
    v = rng.uniform(-5, synth.KITTI_H + 5, n)
    u[rng.random(n) < 0.05] = -0.7  # truncates to (-)0 in the tracks form
    v[rng.random(n) < 0.05] = -0.7
    positive = rng.uniform(0.5, 80, n)
    if layout == "mixed":
        pick = rng.choice(6, n, p=[0.3, 0.4, 0.1, 0.07, 0.06, 0.07])
        depth = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4], [-1.0, positive, np.nan, -0.0, np.inf], 0.0)
    elif layout == "all":
        depth = positive
    elif layout == "none":
        depth = np.where(rng.random(n) < 0.5, -1.0, np.nan)
    else:
        depth = np.full(n, -1.0)
        depth[n - 1:] = positive[n - 1:]
    u, v, depth = u.astype(ft), v.astype(ft), depth.astype(ft)
    if form == "tracks" and n:
        # coordinates no int holds; beside a depth of +-0 an inf makes inf * 0
        for arr in (u, v):
            k = rng.random(n)
            arr[k < 0.04] = np.nan
            arr[(k >= 0.04) & (k < 0.08)] = 1e20
            arr[(k >= 0.08) & (k < 0.11)] = np.inf
            arr[(k >= 0.11) & (k < 0.14)] = -np.inf
    types = rng.integers(-3, 25, n).astype(np.int32)  # -3 .. 24: other is exercised
    return dict(form=form, n=n, u=u, v=v, depth=depth, types=types)


def restate(q, with_types=True):
    """(report [24] int64, points [m, 3] float64, feature [m] int32) of one sequence, computed once and left unchanged."""
    key = ("want", with_types)
    if key in q:
        return q[key]
    n = q["n"]
    with np.errstate(all="ignore"):
        if q["form"] == "tracks":
            u, v = np.trunc(q["u"]).astype(np.float64), np.trunc(q["v"]).astype(np.float64)
        else:
            u, v = q["u"], q["v"]
        d = q["depth"].astype(np.float64)
        idx = np.flatnonzero(d >= 0).astype(np.int32)
        pts = np.stack([(u[idx] - CU) / F * d[idx], (v[idx] - CV) / F * d[idx], d[idx]], axis=1) if n else np.empty((0, 3))
    report = np.zeros(WORDS, np.int64)
    if with_types and n:
        report[:21] = DepthEstimator.resultHistogram(q["types"])  # mld_result_histogram on the host copy
        report[21] = int(((q["types"] < 0) | (q["types"] >= capi.MLD_RESULT_TYPE_COUNT)).sum())
        assert report[:22].sum() == n
    report[22], report[23] = n, idx.size
    for a in (report, pts, idx):
        a.setflags(write=False)
    q[key] = (report, pts, idx)
    return q[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def est():
    e = make_estimator(capi.params_c0(), max_frames=1)
    yield e
    e.close()


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


def wanted(flag, s):
    """Is the optional array given for sequence s?  flag: False (null table), True, or a list of S booleans."""
    return bool(flag) if isinstance(flag, bool) else bool(flag[s])


def prepare(seqs, caps=None, types=True, points=True, feature=True):
    """The device buffers of one call: inputs, guarded outputs, the arguments of collect() / collect_tracks().  The output
    buffers exist whether they are handed over or not, so that what is NOT handed over can be seen to stay untouched.  They
    are made by work on torch's stream, which nothing orders against the context's stream: torch.cuda.synchronize() before
    issue()."""
    import torch
    dev = torch.device("cuda:0")
    S, form = len(seqs), seqs[0]["form"]
    ns = [q["n"] for q in seqs]
    caps = list(ns) if caps is None else list(caps)
    to = lambda a, n: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if n else None  # noqa: E731
    if form == "f64":
        coords = ([to(np.stack([q["u"], q["v"]], axis=1), q["n"]) for q in seqs],)
    else:
        coords = ([to(q["u"], q["n"]) for q in seqs], [to(q["v"], q["n"]) for q in seqs])
    depth = [to(q["depth"], q["n"]) for q in seqs]
    d_types = [to(q["types"], q["n"]) if wanted(types, s) else None for s, q in enumerate(seqs)]
    g = dict(report=Guarded(2 * WORDS * S, dev), points=[Guarded(6 * k, dev) for k in caps], feature=[Guarded(k, dev) for k in caps])
    given = dict(points=points, feature=[wanted(feature, s) and points for s in range(S)])
    args = coords + (depth, None if types is False else d_types, g["report"].view(torch.int64).view(S, WORDS),
                     caps if points else None, [x.view(torch.float64) for x in g["points"]] if points else None,
                     None if feature is False or not points else
                     [x.view(torch.int32) if wanted(feature, s) else None for s, x in enumerate(g["feature"])])
    return dict(form=form, seqs=seqs, caps=caps, types=types, g=g, given=given, args=args)


def issue(dr, p):
    """Queues the call on the context's stream.  No synchronisation."""
    (dr.collect if p["form"] == "f64" else dr.collect_tracks)(*p["args"])


def verify(p, what=""):
    """Every sequence of a finished call against the restatement: the record complete, the first min(n_interpolated,
    capacity) points and feature indices equal, everything at and beyond them - and every array that was not handed over -
    still the guard pattern, the guard words around every array intact."""
    words, ok = p["g"]["report"].read()
    assert ok, what
    report = words.view(np.int64).reshape(len(p["seqs"]), WORDS)
    for s, q in enumerate(p["seqs"]):
        tag = f"{what} [{s}] n={q['n']}"
        want_report, want_pts, want_idx = restate(q, wanted(p["types"], s))
        assert np.array_equal(report[s], want_report), (tag, report[s].tolist(), want_report.tolist())
        cap = p["caps"][s]
        m = min(want_idx.size, cap) if p["given"]["points"] else 0
        pts, ok = p["g"]["points"][s].read()
        assert ok and pts.size == 6 * cap, tag
        assert np.array_equal(pts[:6 * m].view(np.uint64), bits(want_pts[:m]).reshape(-1)), tag
        assert (pts[6 * m:] == GUARD).all(), tag
        k = m if p["given"]["feature"][s] else 0
        feat, ok = p["g"]["feature"][s].read()
        assert ok, tag
        assert np.array_equal(feat[:k], want_idx[:k]), tag
        assert (feat[k:] == GUARD).all(), tag


def run(est, seqs, max_features=None, dr=None, **kw):
    import torch
    p = prepare(seqs, **kw)
    own = dr is None
    if own:
        dr = DepthReports(est, len(seqs), max_features or max(max(q["n"] for q in seqs), 1))
    torch.cuda.synchronize()  # every buffer of the call is made before the context's stream touches one
    issue(dr, p)
    est.synchronize()
    if own:
        dr.close()
    return p


def test_the_inputs_reach_what_they_are_meant_to():
    """On the CPU: the mixed layout holds every kind of depth and types on both sides of the range; the tracks form holds
    coordinates no int holds, and both propagated and generated (inf * 0) NaNs among the points; -0.7 is there to truncate
    to zero."""
    for form in FORMS:
        q = make_inputs(form, 4097, 4097)
        d, t = q["depth"], q["types"]
        assert (d == -1).any() and np.isnan(d).any() and np.isposinf(d).any() and (d > 0).any()
        assert ((d == 0) & np.signbit(d)).any() and ((d == 0) & ~np.signbit(d)).any()
        assert t.min() == -3 and t.max() == 24
        report, pts, idx = restate(q)
        assert 0 < idx.size < q["n"] and report[21] > 0 and report[:21].min() > 0
        assert (q["u"] == q["u"].dtype.type(-0.7)).any()
        nan_pts = np.isnan(pts[:, :2])
        if form == "tracks":
            assert np.isnan(q["u"]).any() and np.isinf(q["v"]).any() and (q["u"] == np.float32(1e20)).any()
            u, v = np.trunc(q["u"]).astype(np.float64)[idx], np.trunc(q["v"]).astype(np.float64)[idx]
            propagated = np.isnan(np.stack([u, v], axis=1))
            assert (nan_pts & propagated).any() and (nan_pts & ~propagated).any() and not (propagated & ~nan_pts).any()
            assert np.isinf(pts[:, :2]).any()
        else:
            assert not nan_pts.any()
    for layout, count in (("all", 1025), ("none", 0), ("last", 1)):
        q = make_inputs("f64", 1025, 7, layout)
        assert restate(q)[2].size == count
    assert restate(make_inputs("f64", 1025, 7, "last"))[2].tolist() == [1024]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_single_sequences(est, n, form):
    verify(run(est, [make_inputs(form, n, 100 + n)]), f"{form} n={n}")


RAGGED = {1: (4097,), 2: (0, 1025), 8: (64, 0, 4097, 1, 1023, 0, 65, 1024),
          13: (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 0, 64, 0, 1023)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", sorted(RAGGED))
def test_ragged_calls(est, S, form):
    """Mixed counts inside one call, sequences of 0 features among them."""
    seqs = [make_inputs(form, n, 200 + 17 * s + n) for s, n in enumerate(RAGGED[S])]
    verify(run(est, seqs, max_features=5000), f"{form} S={S}")


LONG = (65537, 262145, 1)  # 65 chunks: the scan's second wavefront; 257: its second round, the last chunk of one feature


def test_long_sequences_whose_chunk_counts_leave_the_first_wavefront_and_the_first_round_of_the_scan(est):
    """One call on an object of max_features 262 145: the prefix over the chunk counts crosses from wavefront 0 to
    wavefront 1 (65 chunks) and carries into a second round of 256 chunks (257 chunks); the histogram sum likewise."""
    seqs = [make_inputs("f64", n, 100 + n) for n in LONG]
    assert all(0 < restate(q)[2].size < q["n"] for q in seqs[:2])
    verify(run(est, seqs, max_features=262145), "long")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", ["all", "none", "last"])
def test_layouts(est, layout, form):
    """All valid, none valid, valid only in the last lane of the last word - the word full (64, 1024), not full (65, 4097:
    lane 0), and in a later chunk."""
    seqs = [make_inputs(form, n, 300 + n, layout) for n in (64, 65, 1024, 4097, 1)]
    p = run(est, seqs)
    verify(p, f"{form} {layout}")
    nint = [restate(q)[2].size for q in seqs]
    assert nint == dict(all=[64, 65, 1024, 4097, 1], none=[0] * 5, last=[1] * 5)[layout]


CAPACITIES = {"0": lambda m: 0, "1": lambda m: 1, "n_interpolated - 1": lambda m: m - 1, "n_interpolated": lambda m: m,
              "n_interpolated + 3": lambda m: m + 3}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", list(CAPACITIES))
def test_capacity(est, which, form):
    """Nothing at or beyond min(n_interpolated, capacity) changes (the arrays are the guard pattern before the call, with
    guard words around them) and the record stays complete: n_interpolated > capacity shows the truncation."""
    seqs = [make_inputs(form, n, 100 + n) for n in (4097, 65, 0, 1025)]
    caps = [max(0, CAPACITIES[which](restate(q)[2].size)) for q in seqs]
    p = run(est, seqs, caps=caps)
    verify(p, f"{form} capacity {which}")
    if which in ("0", "1", "n_interpolated - 1"):
        assert restate(seqs[0])[0][23] > caps[0]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", ["types null table", "types null entries", "points null table", "feature null table",
                                  "feature null entries"])
def test_optional_arguments(est, case, form):
    seqs = [make_inputs(form, n, 100 + n) for n in (1025, 65, 0, 4097)]
    kw = {"types null table": dict(types=False), "types null entries": dict(types=[True, False, False, True]),
          "points null table": dict(points=False), "feature null table": dict(feature=False),
          "feature null entries": dict(feature=[False, True, True, False])}[case]
    p = run(est, seqs, **kw)
    verify(p, f"{form} {case}")
    if case.startswith("types"):
        words, _ = p["g"]["report"].read()
        report = words.view(np.int64).reshape(4, WORDS)
        assert (report[1, :22] == 0).all() and report[1, 22] == 65 and report[1, 23] == restate(seqs[1])[2].size > 0


@pytest.mark.parametrize("form", FORMS)
def test_a_second_call_leaves_nothing_of_the_first(est, form):
    """One object, two calls with other shapes: fewer chunks, fewer words, other validity, types given then not."""
    dr = DepthReports(est, 3, 5000)
    first = run(est, [make_inputs(form, n, 400 + n, "all") for n in (4097, 1025, 1024)], dr=dr)
    second = run(est, [make_inputs(form, n, 500 + n, lay) for n, lay in ((65, "mixed"), (0, "mixed"), (1023, "last"))], dr=dr,
                 types=[False, True, True])
    third = run(est, [make_inputs(form, n, 600 + n, lay) for n, lay in ((1, "none"), (4097, "mixed"), (64, "all"))], dr=dr)
    dr.close()
    for k, p in enumerate((first, second, third)):
        verify(p, f"{form} call {k}")


def test_collect_past_the_last_generation_of_the_descriptor_ring(est):
    """35 calls with different inputs and outputs, both forms in turn, are queued without a synchronisation in between
    (the ring has 16 generations); every call's outputs are checked after one synchronisation."""
    import torch
    S, calls = 3, 35
    sizes = (0, 1, 63, 64, 65, 130, 257, 1023, 1024, 1025, 1500)
    pool = {(form, n): make_inputs(form, n, 700 + n) for form in FORMS for n in sizes}
    dr = DepthReports(est, S, max(sizes))
    queued = []
    for k in range(calls):  # the buffers of ALL calls first ...
        form = FORMS[k % 2]
        seqs = [pool[form, sizes[(k + 3 * s) % len(sizes)]] for s in range(S)]
        caps = [q["n"] if (k + s) % 3 else q["n"] // 4 for s, q in enumerate(seqs)]
        queued.append(prepare(seqs, caps=caps, types=bool(k % 5), feature=bool(k % 4)))
    torch.cuda.synchronize()
    for p in queued:  # ... then the calls back to back
        issue(dr, p)
    est.synchronize()
    dr.close()
    for k, p in enumerate(queued):
        verify(p, f"call {k}")
    assert sum(restate(q)[2].size for q in pool.values()) > 0


def test_inf_times_zero(est):
    """The four combinations of +-inf coordinates and +-0 depths, by hand: NaN components, equal as bits to NumPy's."""
    import torch
    dev = torch.device("cuda:0")
    u = np.array([np.inf, np.inf, -np.inf, -np.inf], np.float32)
    v = np.array([20.9, 311.0, 3.0, -0.7], np.float32)
    d = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    dr = DepthReports(est, 1, 4)
    report = torch.full((1, WORDS), -7, dtype=torch.int64, device=dev)
    pts = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    dr.collect_tracks([torch.from_numpy(u).to(dev)], [torch.from_numpy(v).to(dev)], [torch.from_numpy(d).to(dev)], None, report,
                      None, [pts], None)
    est.synchronize()
    dr.close()
    got = pts.cpu().numpy()
    assert report.cpu().numpy()[0].tolist() == [0] * 22 + [4, 4]
    with np.errstate(all="ignore"):
        want = np.stack([(np.trunc(u).astype(np.float64) - CU) / F * d.astype(np.float64),
                         (np.trunc(v).astype(np.float64) - CV) / F * d.astype(np.float64), d.astype(np.float64)], axis=1)
    generated = np.zeros((4, 3), bool)
    generated[:, 0] = True
    assert np.isnan(want[generated]).all() and not np.isnan(want[~generated]).any()
    assert np.array_equal(bits(got), bits(want))
    assert np.signbit(got[1, 2]) and got[1, 2] == 0  # -0.0 is in, and stays -0.0


def test_arguments_are_refused_by_name(est):
    """Misaligned arrays and more features than the object was made for, on a live object; nothing is written by a
    refused call and the object serves the next one."""
    import torch
    dev = torch.device("cuda:0")
    lib = capi.load()
    dr = DepthReports(est, 2, 100)
    f32 = torch.zeros(128, dtype=torch.float32, device=dev)
    f64 = torch.zeros(256, dtype=torch.float64, device=dev)
    i32 = torch.ones(128, dtype=torch.int32, device=dev)
    report = torch.full((2 * WORDS + PAD,), -7, dtype=torch.int64, device=dev)
    points = torch.full((600 + PAD,), GUARD, dtype=torch.int32, device=dev)
    feature = torch.full((100 + PAD,), GUARD, dtype=torch.int32, device=dev)
    tab = lambda t, off=0: (C.c_void_p * 2)(t.data_ptr(), t.data_ptr() + off)  # noqa: E731
    half = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)  # noqa: E731
    i64 = lambda a, b: (C.c_int64 * 2)(a, b)  # noqa: E731
    good = dict(u=tab(f32), v=tab(f32), uv=tab(f64), depth32=tab(f32), depth64=tab(f64), type=tab(i32), n=i64(100, 100),
                cap=i64(100, 100), report=report.data_ptr(), points=tab(points), feature=tab(feature))

    def call(form, **kw):
        a = dict(good, **kw)
        if form == "f64":
            rc = lib.mld_depth_reports_collect_device(dr._dr, a["uv"], a["depth64"], a["type"], a["n"], a["cap"], a["report"],
                                                      a["points"], a["feature"])
        else:
            rc = lib.mld_depth_reports_collect_tracks_device(dr._dr, a["u"], a["v"], a["depth32"], a["type"], a["n"], a["cap"],
                                                             a["report"], a["points"], a["feature"])
        return rc, lib.mld_depth_reports_last_error(dr._dr).decode()

    torch.cuda.synchronize()
    cases = [("tracks", dict(u=tab(f32, 2)), "u must be 4-byte aligned"), ("tracks", dict(v=tab(f32, 2)), "v must be 4-byte aligned"),
             ("tracks", dict(depth32=tab(f32, 2)), "depth must be 4-byte aligned"),
             ("f64", dict(uv=tab(f64, 4)), "uv must be 8-byte aligned"), ("f64", dict(depth64=tab(f64, 4)), "depth must be 8-byte aligned"),
             ("tracks", dict(u=None), "null table u"), ("tracks", dict(v=None), "null table v"), ("f64", dict(uv=None), "null table uv"),
             ("f64", dict(depth64=None), "null table depth"), ("tracks", dict(n=None), "null table n_features"),
             ("tracks", dict(report=None), "report_out_dev"), ("f64", dict(cap=None), "capacity"),
             ("tracks", dict(u=half(f32)), "null array u"), ("tracks", dict(v=half(f32)), "null array v"),
             ("f64", dict(uv=half(f64)), "null array uv"), ("f64", dict(depth64=half(f64)), "null array depth"),
             ("tracks", dict(points=half(points)), "null array points_out"),
             ("tracks", dict(n=i64(100, -1)), "negative n_features"), ("f64", dict(cap=i64(100, -1)), "negative capacity")]
    for form in FORMS:
        cases += [(form, dict(type=tab(i32, 2)), "type must be 4-byte aligned"),
                  (form, dict(report=report.data_ptr() + 4), "report_out_dev must be 8-byte aligned"),
                  (form, dict(points=tab(points, 4)), "points_out must be 8-byte aligned"),
                  (form, dict(feature=tab(feature, 2)), "feature_out must be 4-byte aligned")]
    for form, kw, word in cases:
        rc, text = call(form, **kw)
        fn = "mld_depth_reports_collect_device" if form == "f64" else "mld_depth_reports_collect_tracks_device"
        assert rc == capi.MLD_ERR_INVALID_ARG and word in text and fn + ":" in text, (form, list(kw), text)
    for form in FORMS:
        rc, text = call(form, n=i64(100, 101))
        assert rc == capi.MLD_ERR_CAPACITY and "max_features" in text and "n_features" in text
    est.synchronize()
    assert (report.cpu().numpy() == -7).all() and (points.cpu().numpy() == GUARD).all() and (feature.cpu().numpy() == GUARD).all()
    # a sequence without features needs no arrays, one without capacity no outputs; statistics only needs no capacity
    for form, kw in (("tracks", dict(n=i64(100, 0), u=half(f32), v=half(f32), depth32=half(f32), type=half(i32), points=half(points),
                                     feature=half(feature))),
                     ("f64", dict(cap=i64(100, 0), points=half(points), feature=half(feature))),
                     ("f64", dict(points=None, cap=None, feature=None))):
        rc, text = call(form, **kw)
        assert rc == capi.MLD_OK, text
        est.synchronize()
        got = report.cpu().numpy()[:2 * WORDS].reshape(2, WORDS)
        n1 = int(kw["n"][1]) if "n" in kw else 100
        want = np.zeros((2, WORDS), np.int64)
        want[0, 1], want[0, 22], want[0, 23] = 100, 100, 100  # types all 1 (Success), depths all 0: every feature has one
        want[1, 1], want[1, 22], want[1, 23] = n1, n1, n1
        assert np.array_equal(got, want), (form, got.tolist())
    assert (report.cpu().numpy()[2 * WORDS:] == -7).all()
    dr.close()


def _mask_of(inl, n, dev):
    import torch
    m = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(m, inl >> 5, (np.uint32(1) << (inl & 31).astype(np.uint32)))
    return torch.from_numpy(m.view(np.int32)).to(dev)


def check_real(form, u, v, depth, types, report, points, feature, what):
    """Read-back results of the depth path against the restatement; returns (n_interpolated, n)."""
    q = dict(form=form, n=depth.size, u=u, v=v, depth=depth, types=types)
    want_report, want_pts, want_idx = restate(q)
    assert np.array_equal(report, want_report), (what, report.tolist(), want_report.tolist())
    assert np.array_equal(report[:21], DepthEstimator.resultHistogram(types)) and report[21] == 0, what
    m = want_idx.size
    assert np.array_equal(bits(points[:m]), bits(want_pts)), what
    with np.errstate(invalid="ignore"):
        assert np.array_equal(feature[:m], np.flatnonzero(depth >= 0)), what
    return m, depth.size


def test_depth_estimator_layer_end_to_end():
    """Three slots of synthetic frames through mld_calculate_depths_device (C0 parameters, a plane), then collect() directly
    behind it on the same stream: counts equal resultHistogram of the read-back types, points the restatement on the
    read-back depths."""
    import torch
    dev = torch.device("cuda:0")
    S, ns = 3, (300, 1025, 64)
    e = make_estimator(capi.params_c0(), max_frames=S)
    dr = DepthReports(e, S, max(ns))
    host_uv = []
    for s in range(S):
        cloud = synth.make_cloud(synth.VLP16, seed=80 + s, frame=s)
        coeffs, inl = synth.make_ground_plane(cloud)
        e.setInputCloud(torch.from_numpy(cloud).to(dev), GroundPlane(coeffs, inl), s)
        host_uv.append(np.ascontiguousarray(synth.make_features_near_points(cloud, ns[s], seed=s)))
    uvs = [torch.from_numpy(a).to(dev) for a in host_uv]
    depths = [torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for n in ns]
    types = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
    report = torch.full((S, WORDS), -7, dtype=torch.int64, device=dev)
    points = [torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev) for n in ns]
    feature = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
    torch.cuda.synchronize()
    e.CalculateDepths(uvs, depths, types)
    dr.collect(uvs, depths, types, report, None, points, feature)  # (directly behind the depth call)
    e.synchronize()
    got, valid, total = report.cpu().numpy(), 0, 0
    for s in range(S):
        m, n = check_real("f64", host_uv[s][:, 0], host_uv[s][:, 1], depths[s].cpu().numpy(), types[s].cpu().numpy(), got[s],
                          points[s].cpu().numpy(), feature[s].cpu().numpy(), f"slot {s}")
        valid, total = valid + m, total + n
    assert 0 < valid < total  # (real depths, and features without one)
    dr.close()
    e.close()


def test_tracklet_layer_end_to_end():
    """A two-frame TrackletBatch run with step(), S = 3, then reports(f, points=True), consumed by a torch operation
    without an explicit synchronisation: the same equalities on the read-back d_cur / t_cur, and `feature` indexes exactly
    the tracks with d_cur >= 0, in order."""
    import torch
    dev = torch.device("cuda:0")
    S, H, ns = 3, 4, (300, 257, 64)
    cam, rng = kitti_camera(), np.random.default_rng(41)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tb = TrackletBatch(capi.params_c0(), cam, synth.T_CAM_LIDAR, S, max(ns))
    with pytest.raises(Exception, match="attach_reports"):
        tb.reports({})
    tb.attach_store(H)
    assert tb.attach_reports() is tb.attach_reports() and tb.depth_reports.max_features == max(ns)
    valid = total = 0
    for f in range(2):
        per = []
        for s in range(S):
            cloud = synth.make_cloud(synth.VLP16, seed=90 + s, frame=2 * f)
            coeffs, inl = synth.make_ground_plane(cloud)
            ids = np.arange(ns[s], dtype=np.int32)
            ids[rng.random(ns[s]) < 0.3 * f] += 1000 * f  # frame 1: a third of the tracks are new
            uv = synth.make_features_near_points(cloud, ns[s], seed=10 * f + s).astype(np.float32)
            u1 = (uv[:, 0] + rng.normal(0, 3, ns[s])).astype(np.float32)
            v1 = (uv[:, 1] + rng.normal(0, 2, ns[s])).astype(np.float32)
            per.append((cloud, coeffs, inl, ids, np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1]), u1, v1))
        clouds = [to(p[0]) for p in per]
        masks = [_mask_of(p[2], p[0].shape[0], dev) for p in per]
        feats = [[to(p[k]) for p in per] for k in (4, 5, 6, 7)]
        ids_d = [to(p[3]) for p in per]
        d_cur = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in ns]
        d_last = [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in ns]
        t_cur = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
        t_last = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in ns]
        table = tb.prepare_step(clouds, np.stack([p[1] for p in per]), masks, ids_d, *feats, d_cur, d_last, t_cur, t_last)
        torch.cuda.synchronize()
        tb.step(table)
        out = tb.reports(table, points=True)
        # torch consumes the tensors at once, on its own stream, with no synchronisation of the caller's
        report = out["report"].clone()
        sums = torch.stack([p[:0].sum() + r[23] for p, r in zip(out["points"], out["report"])])
        copies = [(p.clone(), i.clone()) for p, i in zip(out["points"], out["feature"])]
        got = report.cpu().numpy()
        assert np.array_equal(sums.cpu().numpy(), got[:, 23].astype(np.float64))
        assert tuple(out["report"].shape) == (S, WORDS) and got[:, 22].tolist() == list(ns)
        for s in range(S):
            assert tuple(out["points"][s].shape) == (ns[s], 3) and tuple(out["feature"][s].shape) == (ns[s],)
            m, n = check_real("tracks", per[s][4], per[s][5], d_cur[s].cpu().numpy(), t_cur[s].cpu().numpy(), got[s],
                              copies[s][0].cpu().numpy(), copies[s][1].cpu().numpy(), f"frame {f}, sequence {s}")
            valid, total = valid + m, total + n
    assert 0 < valid < total  # (real depths, and tracks without one)
    stats = tb.reports(table, capacity=[5, 0, 1000])  # statistics only: capacity is ignored
    assert stats["points"] is None and stats["feature"] is None
    assert np.array_equal(stats["report"].cpu().numpy(), got)
    few = tb.reports(table, points=True, capacity=[5, 0, 1000])
    assert [tuple(p.shape) for p in few["points"]] == [(5, 3), (0, 3), (64, 3)]
    assert np.array_equal(few["report"].cpu().numpy(), got)
    k = min(5, int(got[0, 23]))
    assert k > 0 and np.array_equal(few["feature"][0].cpu().numpy()[:k], np.flatnonzero(d_cur[0].cpu().numpy() >= 0)[:k])
    tb.close()
