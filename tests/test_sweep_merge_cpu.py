"""The batched sweep merge without a GPU: symbols, the record's layout, the Python names, where the source sits, the
refusals of create before the device is touched, the restatement the GPU tests compare against (against a plain loop
over the records), and what the merge is for: more Success on the oracle, the current sweep keeping its map cells."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi, synth

import sweep_merge_restatement as R
from helpers import make_oracle

ROOT = Path(__file__).resolve().parent.parent

SYMBOLS = ("mld_sweep_merge_create", "mld_sweep_merge_destroy", "mld_sweep_merge_last_error", "mld_sweep_merge_run_device")
# include/mld.h, mld_sweep_merge_record: (field, offset, bytes)
LAYOUT = [("n_in", 0, 8), ("n_kept", 8, 8), ("n_written", 16, 8), ("n_nonfinite", 24, 8), ("n_out_of_range", 32, 8),
          ("kept", 40, 64), ("flags", 104, 4), ("pad_", 108, 4)]


def test_header_capi_and_both_libraries_carry_the_four_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_sweep_merge mld_sweep_merge;" in code
    assert re.search(r"#define\s+MLD_SWEEP_MAX_SWEEPS\s+16\b", code) and capi.MLD_SWEEP_MAX_SWEEPS == 16
    assert re.search(r"\bMLD_SWEEP_FLAG_TRUNCATED = 1\b", code) and capi.MLD_SWEEP_FLAG_TRUNCATED == 1


def test_the_record_has_the_size_and_the_offsets_of_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mld.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct mld_sweep_merge_record \{(.*?)\} mld_sweep_merge_record;", header, flags=re.S).group(1)
    fields = []
    for kind, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\w+)\])?\s*$", item)
            count = {None: 1, "MLD_SWEEP_MAX_SWEEPS": 16}[m.group(2)]
            fields.append((m.group(1), (4 if kind == "int32_t" else 8) * count))
    offset, laid = 0, []
    for name, size in fields:
        laid.append((name, offset, size))
        offset += size
    assert laid == LAYOUT and offset == 112  # (every field is naturally aligned where it falls: no padding)
    rec = capi.MldSweepMergeRecord
    assert C.sizeof(rec) == 112 and C.alignment(rec) == 8
    assert [(n, getattr(rec, n).offset, getattr(rec, n).size) for n, _ in rec._fields_] == LAYOUT
    assert R.DTYPE.itemsize == 112 and [(n, R.DTYPE.fields[n][1]) for n in R.DTYPE.names] == [(n, o) for n, o, _ in LAYOUT]
    source = (ROOT / "mono_lidar_depth_amd" / "csrc" / "sweeps" / "mld_sweep_merge.hip").read_text()
    assert "static_assert(sizeof(mld_sweep_merge_record) == 112" in source


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "SweepMerge" in m.__all__
    for name in ("merge", "records", "close"):
        assert hasattr(m.SweepMerge, name), name
    assert m.SweepMerge.WORDS == 14 and m.SweepMerge.DTYPE.itemsize == 112 and m.SweepMerge.MAX_SWEEPS == 16
    assert hasattr(m.TrackletBatch, "attach_sweep_merge") and hasattr(m.TrackletBatch, "merge_sweeps")
    rows = [(attr, row) for attr, row in m.TrackletBatch._ATTACHABLE.items() if row[0] is m.SweepMerge]
    assert len(rows) == 1 and rows[0][1][1] == "attach_sweep_merge"
    assert "synchronisation" in m.TrackletBatch.merge_sweeps.__doc__ and "112" in m.TrackletBatch.merge_sweeps.__doc__


def test_the_sweep_merge_is_a_translation_unit_of_its_own():
    """In sweeps/, on the shared batch headers only, linked into both libraries; the depth path's sources do not know of
    it; three kernels with stable names; no atomics, no inline assembly, no synchronisation."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "sweeps" / "mld_sweep_merge.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h"]
    code = re.sub(r"//.*", "", text)
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    for word in ("asm", "atomic", "Synchronize", "hipMalloc", "hipMemcpy"):
        assert word not in code, word
    assert re.findall(r"__global__[^\n]*\bvoid (\w+)\(", text) == ["k_sm_pass", "k_sm_scan", "k_sm_write"]
    for helper in ("create_object", "DescRing", "DeviceBuffer", "CompactScratch", "scan_inclusive", "group_ranks", "lane_rank"):
        assert helper in code, helper
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("$(SWEEPS)" in ln for ln in link_lines)
    assert re.search(r"^SWEEPS\s*:=\s*sweeps/mld_sweep_merge\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(SWEEPS\)", mk, flags=re.M)
    assert "-ffp-contract=off" in mk
    for path in csrc.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert "mld_sweep_merge" not in path.read_text(), path.name


@pytest.mark.parametrize("n_seq,max_sweeps,max_points,word", [
    (0, 3, 100, "n_seq"), (65537, 3, 100, "n_seq"), (4, 0, 100, "max_sweeps"), (4, 17, 100, "max_sweeps"), (4, -1, 100, "max_sweeps"),
    (4, 3, 0, "max_points"), (4, 3, 8388608, "max_points"), (4, 2, 4194304, "max_sweeps * max_points"),
    (4, 16, 524288, "max_sweeps * max_points")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_sweeps, max_points, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_sweep_merge_create(None, n_seq, max_sweeps, max_points, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_sweep_merge_last_error(None).decode()
    assert "mld_sweep_merge_create" in text and word in text and "context" not in text


def test_create_judges_the_sizes_before_the_context_and_run_refuses_no_object():
    lib = capi.load()
    st = C.c_int(0)
    # the largest sizes that pass are refused for the context alone, of which nothing is used
    for sizes in ((65536, 16, 524287), (1, 1, 8388607), (7, 3, 2796202)):
        assert not lib.mld_sweep_merge_create(None, *sizes, C.byref(st))
        assert st.value == capi.MLD_ERR_INVALID_ARG
        assert lib.mld_sweep_merge_last_error(None).decode() == "mld_sweep_merge_create: null context"
    assert not lib.mld_sweep_merge_create(None, 1, 1, 1, None)  # (status_out is optional)
    tab, zero = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    rc = lib.mld_sweep_merge_run_device(None, 1, tab, zero, 16, None, 0.0, float("inf"), zero, tab, None, None, None)
    assert rc == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_sweep_merge_last_error(None).decode() == "mld_sweep_merge_run_device: null object (sm)"
    lib.mld_sweep_merge_destroy(None)


# ---- the restatement against a plain loop ---------------------------------------------------------------------------------

def rotation_translation(yaw_deg, t):
    c, s = np.cos(np.deg2rad(yaw_deg)), np.sin(np.deg2rad(yaw_deg))
    return np.array([[c, -s, 0.0, t[0]], [s, c, 0.0, t[1]], [0.0, 0.0, 1.0, t[2]]], dtype=np.float64)


def random_records(rng, n, width=4, scale=30.0, specials=True):
    """n records of `width` floats: coordinates within +-scale, every float of the record filled, and - with specials - some
    NaN, +-inf and +-0.0 coordinates."""
    cloud = rng.uniform(-scale, scale, (n, width)).astype(np.float32)
    if specials and n:
        for value in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            rows = rng.integers(0, n, max(1, n // 25))
            cloud[rows, rng.integers(0, 3, len(rows))] = value
    return cloud


@pytest.mark.parametrize("width", [4, 8])
def test_the_restatement_is_a_plain_loop_over_the_records(width):
    """200 random records in three sweeps - NaN, +-inf and +-0.0 among them, a rotation with a translation, a missing
    transform and a range gate that removes some - give the same bits, sweeps, indices and counts one record at a time."""
    rng = np.random.default_rng(20261021 + width)
    sweeps = [random_records(rng, 90, width), random_records(rng, 70, width), random_records(rng, 40, width)]
    sweeps[0][5, :3] = (-0.0, 0.0, 12.0)  # (kept by the gate below, through the missing transform: the sign survives)
    transforms = [None, rotation_translation(7.5, (-1.25, 0.3, 0.02)), rotation_translation(-171.0, (2.0, -0.7, 0.1))]
    got = R.merge_sequence(sweeps, transforms, 8.0, 35.0)
    bits, sw, og, (n_nf, n_or) = R.merge_by_loop(sweeps, transforms, 8.0, 35.0)
    rec = got["record"]
    assert [tuple(int(w) for w in row) for row in got["merged"]] == bits
    assert got["sweep"].tolist() == sw and got["orig"].tolist() == og
    assert (int(rec["n_in"]), int(rec["n_nonfinite"]), int(rec["n_out_of_range"])) == (200, n_nf, n_or)
    assert int(rec["n_kept"]) == len(bits) == 200 - n_nf - n_or == int(rec["kept"].sum()) and int(rec["flags"]) == 0
    assert n_nf >= 10 and n_or >= 20 and len(bits) >= 50 and all(rec["kept"][:3] > 0) and not rec["kept"][3:].any()
    row = got["merged"][list(zip(sw, og)).index((0, 5))]
    assert row[0] == 0x80000000 and row[1] == 0  # -0.0, +0.0
    # capacity: the first records, complete counts, the flag
    cut = R.merge_sequence(sweeps, transforms, 8.0, 35.0, capacity=len(bits) - 1)
    assert np.array_equal(cut["merged"], got["merged"][:-1]) and int(cut["record"]["n_written"]) == len(bits) - 1
    assert int(cut["record"]["n_kept"]) == len(bits) and int(cut["record"]["flags"]) == capi.MLD_SWEEP_FLAG_TRUNCATED
    assert np.array_equal(cut["record"]["kept"], rec["kept"])
    # no gate: only the records that are not finite go
    free = R.merge_sequence(sweeps, transforms)
    assert int(free["record"]["n_out_of_range"]) == 0 and int(free["record"]["n_nonfinite"]) == n_nf


# ---- what the merge is for ----------------------------------------------------------------------------------------------

FRAME = 6


def shift(frames_back):
    """Sweep `frames_back` frames ago into the current lidar frame: the sensor advances 1 m per frame along x."""
    return np.array([[1.0, 0.0, 0.0, -float(frames_back)], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


def three_sweeps(scanner, frame=FRAME, seed=3):
    return [synth.make_cloud(scanner, seed=seed, frame=frame - j) for j in range(3)], [None, shift(1), shift(2)]


@pytest.fixture(scope="module", params=["HDL64", "VLP16"])
def merged_frames(request):
    scanner = getattr(synth, request.param)
    sweeps, transforms = three_sweeps(scanner)
    return request.param, sweeps, R.merge_sequence(sweeps[:1]), R.merge_sequence(sweeps, transforms)


def test_three_merged_sweeps_give_strictly_more_success_than_the_current_one(merged_frames):
    """synth scene seed 3, current frame 6, C0, 2000 uniform features, no plane: the restatement's merge of frames 6, 5, 4
    against frame 6 alone on the oracle."""
    name, sweeps, _, merged = merged_frames
    P = capi.params_c0()
    uv = synth.make_features(2000, seed=5)
    success = []
    for cloud in (sweeps[0], R.merged_cloud(merged)):
        ref = make_oracle(P)
        ref.set_cloud(cloud)
        ref.set_ground_plane(None, None)
        _, types = ref.calculate_depth(uv)
        success.append(int((types == 1).sum()))
    print(f"{name}: Success of 2000 with 1 sweep {success[0]}, with 3 sweeps {success[1]}; "
          f"{int(merged['record']['n_kept'])} of {int(merged['record']['n_in'])} records kept")
    assert success[1] > success[0], (name, success)


def test_the_current_sweep_keeps_every_cell_it_occupies_alone(merged_frames):
    """The pixel map keeps the first return of a cell: with the current sweep in front of the merged cloud, every cell it
    occupies alone holds the same point of it in the merged map (the kept records of sweep 0 lead, in their order)."""
    name, sweeps, alone, merged = merged_frames
    P = capi.params_c0()
    k0 = int(merged["record"]["kept"][0])
    assert k0 == int(alone["record"]["n_kept"]) > 0 and np.array_equal(merged["merged"][:k0], alone["merged"])
    assert np.all(merged["sweep"][:k0] == 0) and np.all(merged["sweep"][k0:] > 0)
    maps = []
    for result in (alone, merged):
        ref = make_oracle(P)
        ref.set_cloud(R.merged_cloud(result))
        pm, index = ref.pixel_map(), ref.point_index()
        maps.append(np.where(pm >= 0, index[np.maximum(pm, 0)], -1))  # the cloud's own index of the point a cell holds
    own, both = maps
    cells = own >= 0
    assert cells.sum() > 1000 and np.array_equal(both[cells], own[cells])
    assert (both >= 0).sum() > cells.sum() and np.all(both[(both >= 0) & ~cells] >= k0)  # the older sweeps fill empty cells only
