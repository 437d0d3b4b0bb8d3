"""The batched export of the ground-plane inliers without a GPU: symbols, refusals before the device is touched, the
Python names, where the source sits, and the restatement the GPU tests compare against."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import capi, synth

from helpers import make_oracle
from plane_inliers_restatement import camera_cs, mask_bits, restate, words_of

ROOT = Path(__file__).resolve().parent.parent

INLIER_SYMBOLS = ("mld_plane_inliers_create", "mld_plane_inliers_destroy", "mld_plane_inliers_last_error",
                  "mld_plane_inliers_export_device")


def _transform():
    T = np.ascontiguousarray(np.asarray(synth.T_CAM_LIDAR, dtype=np.float64).reshape(-1)[:12])
    return T, T.ctypes.data_as(C.POINTER(C.c_double))


def test_header_capi_and_both_libraries_carry_the_four_symbols():
    header = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", header).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mld_[a-z0-9_]+)\s*\(", code))
    for lib in (capi.load(), capi.load_ab()):
        for name in INLIER_SYMBOLS:
            assert name in declared, name
            assert name in capi.EXPORTED_SYMBOLS, name
            assert hasattr(lib, name), name
        assert lib.mld_abi_version() == 8
    assert "typedef struct mld_plane_inliers mld_plane_inliers;" in code
    assert re.search(r"typedef struct mld_plane_inlier_counts \{\s*int64_t n_inliers;\s*int64_t n_cloud;\s*\} mld_plane_inlier_counts;",
                     code)
    assert C.sizeof(capi.MldPlaneInlierCounts) == 16
    assert [f[0] for f in capi.MldPlaneInlierCounts._fields_] == ["n_inliers", "n_cloud"]
    # the byte formulas, the ignored tail bits and the one-capacity rule are stated where the caller reads them
    for word in ("n_seq * (8 * ceil(max_points / 1024) + 56) bytes", "n_seq * 8 * ceil(max_points / 64) bytes more",
                 "16 * 48 * n_seq bytes", "in the last word are IGNORED", "nothing beyond the last word is read",
                 "ONE capacity bounds each list by its own rank", "n_inliers > capacity[s]"):
        assert word in header, word


def test_the_python_names_are_exported():
    import mono_lidar_depth_amd as m
    assert "PlaneInliers" in m.__all__
    for name in ("export", "close", "mask_words"):
        assert hasattr(m.PlaneInliers, name), name
    assert hasattr(m.TrackletBatch, "attach_plane_inliers") and hasattr(m.TrackletBatch, "plane_inliers")


@pytest.mark.parametrize("n_seq,max_points,word", [(0, 100, "n_seq"), (-1, 100, "n_seq"), (65537, 100, "n_seq"),
                                                   (4, 0, "max_points"), (4, -5, "max_points"), (4, 8388608, "max_points")])
def test_create_refuses_bad_sizes_before_it_looks_at_the_context(n_seq, max_points, word):
    lib = capi.load()
    st = C.c_int(0)
    assert not lib.mld_plane_inliers_create(None, n_seq, max_points, None, None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_plane_inliers_last_error(None).decode()
    assert "mld_plane_inliers_create" in text and word in text and "context" not in text


def test_create_without_a_context_params_or_a_transform_is_refused():
    lib = capi.load()
    st = C.c_int(0)
    P = capi.params_c0()
    T, Tp = _transform()
    assert not lib.mld_plane_inliers_create(None, 4, 1000, C.byref(P), Tp, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    assert "null context" in lib.mld_plane_inliers_last_error(None).decode()
    assert not lib.mld_plane_inliers_create(None, 65536, 8388607, None, None, None)  # (status_out is optional)
    assert "null context" in lib.mld_plane_inliers_last_error(None).decode()
    # Null params / transform behind a context that is not null: the arguments are judged before the context is used, so
    # any non-null address will do here; nothing is dereferenced.
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    assert not lib.mld_plane_inliers_create(fake, 4, 1000, None, Tp, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_plane_inliers_last_error(None).decode()
    assert "mld_plane_inliers_create" in text and "null params" in text
    assert not lib.mld_plane_inliers_create(fake, 4, 1000, C.byref(P), None, C.byref(st))
    assert st.value == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_plane_inliers_last_error(None).decode()
    assert "mld_plane_inliers_create" in text and "null T_cam_lidar" in text


def _good_args():
    tab = (C.c_void_p * 1)(None)
    zero = (C.c_int64 * 1)(0)
    return dict(pts=tab, n=zero, stride=16, mask=tab, cap=zero, counts=None, index=tab, lidar=None, cam=None)


REFUSALS = [dict(), dict(pts=None), dict(n=None), dict(mask=None), dict(cap=None), dict(index=None), dict(counts=0x1004),
            dict(n=(C.c_int64 * 1)(-1)), dict(cap=(C.c_int64 * 1)(-1)), dict(stride=12), dict(stride=0),
            dict(n=(C.c_int64 * 1)(5)), dict(n=(C.c_int64 * 1)(8388608)),
            dict(n=(C.c_int64 * 1)(5), pts=(C.c_void_p * 1)(0x1002)),
            dict(n=(C.c_int64 * 1)(5), pts=(C.c_void_p * 1)(0x1000), mask=(C.c_void_p * 1)(0x1002)),
            dict(lidar=(C.c_void_p * 1)(0x1002)), dict(cam=(C.c_void_p * 1)(0x1004))]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: ",".join(d) or "good")
def test_export_on_no_object_is_refused_whatever_the_arguments(bad):
    """Every refusal of the call, and a call with nothing else wrong, made on a null object: MLD_ERR_INVALID_ARG with a
    text that names the object - decided on the host, no GPU is looked for."""
    lib = capi.load()
    lib.mld_plane_inliers_destroy(None)
    assert not lib.mld_plane_inliers_create(None, 0, 1, None, None, None)  # (leaves another text behind)
    a = dict(_good_args(), **bad)
    rc = lib.mld_plane_inliers_export_device(None, a["pts"], a["n"], a["stride"], a["mask"], a["cap"], a["counts"], a["index"],
                                             a["lidar"], a["cam"])
    assert rc == capi.MLD_ERR_INVALID_ARG
    text = lib.mld_plane_inliers_last_error(None).decode()
    assert "mld_plane_inliers_export_device" in text and "null object" in text and "(pi)" in text


def test_the_inliers_are_a_translation_unit_of_their_own():
    """In planes/, on the shared batch header only, linked into both libraries; the depth path's sources do not know of it."""
    csrc = ROOT / "mono_lidar_depth_amd" / "csrc"
    text = (csrc / "planes" / "mld_plane_inliers.hip").read_text()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["../batch/mld_batch_object.h", "../batch/mld_batch_device.h"]
    assert "mld_device.h" not in text and "mld_diag.h" not in text
    assert "asm" not in re.sub(r"//.*", "", text)
    mk = (csrc / "Makefile").read_text()
    link_lines = [ln for ln in mk.splitlines() if "-shared" in ln]
    assert len(link_lines) == 2 and all("mld_api.hip $(INLIERS) $(TRACKS)" in ln for ln in link_lines)
    assert re.search(r"^INLIERS\s*:=\s*planes/mld_plane_inliers\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^SRC\s*:=.*\$\(REPORTS\) \$\(INLIERS\)", mk, flags=re.M)
    for path in csrc.iterdir():
        if path.is_file() and path.name != "Makefile":
            assert "mld_plane_inliers" not in path.read_text(), path.name


def _random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    cl = np.zeros((n, 4), np.float32)
    cl[:, 0] = rng.uniform(-30, 60, n)
    cl[:, 1] = rng.uniform(-10, 10, n)
    cl[:, 2] = rng.uniform(-3, 3, n)
    return cl


def test_the_restatement_equals_the_oracle_and_a_plain_loop():
    """On a 2000-point random cloud: the camera coordinates are the oracle's camera-frame cloud as raw bits, the index list
    is what a plain loop over the bits gives, and a mask with every bit beyond n set gives the same."""
    n = 2000
    cloud = _random_cloud(n, 77)
    cloud[5, 0] = np.nan
    rng = np.random.default_rng(78)
    bits = rng.random(n) < 0.5
    bits[5] = True
    words = words_of(bits)
    assert words.size == 63 and np.array_equal(mask_bits(words, n), bits)
    ref = make_oracle(capi.params_c0())
    ref.set_cloud(cloud)
    cam = np.ascontiguousarray(ref.cloud_camera_cs().T)
    assert np.array_equal(camera_cs(cloud).view(np.int64), cam.view(np.int64))
    loop = [i for i in range(n) if (int(words[i >> 5]) >> (i & 31)) & 1]
    for use, thr in ((False, 0.0), (True, 2.0)):
        r = restate(cloud, words, use, thr)
        assert r["index"].tolist() == loop and r["n_inliers"] == len(loop)
        assert np.array_equal(r["lidar"].view(np.int32), cloud[loop, :3].view(np.int32))
        kept = [i for i in loop if not use or abs(cam[i, 0]) <= thr]
        assert 5 in loop and (5 in kept) == (not use)  # the NaN record: in the cloud only with the filter off
        assert r["n_cloud"] == len(kept) and 0 < len(kept) and (not use or len(kept) < len(loop))
        assert np.array_equal(r["cam"].view(np.int64), cam[kept].view(np.int64))
        dirty = words.copy()
        dirty[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n & 31)
        assert dirty[-1] != words[-1]
        d = restate(cloud, dirty, use, thr)
        assert np.array_equal(d["index"], r["index"]) and d["n_cloud"] == r["n_cloud"]
