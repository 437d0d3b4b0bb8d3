"""The leaving export without a GPU: the header and the library declare and export the two new functions at ABI 8, and
TrackArchive fed the capped model's streams reproduces the reference's unbounded deques (track_leaving_restatement.py).
"""
import re
from pathlib import Path

import numpy as np
import pytest

from mono_lidar_depth_amd import TrackArchive, capi

from track_leaving_restatement import CappedStore, UnboundedMap, as_frame

ROOT = Path(__file__).resolve().parent.parent
NEW = ("mld_tracks_export_leaving_device", "mld_tracks_set_leaving_sink")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_header_declares_the_functions_at_abi_8():
    hdr = (ROOT / "include" / "mld.h").read_text()
    assert int(re.search(r"#define\s+MLD_ABI_VERSION\s+(\d+)", hdr).group(1)) == 8 == capi.MLD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*mld_tracks\s*\*\s*tr\b", code), name
    body = re.search(r"typedef struct mld_leaving_record \{(.*?)\} mld_leaving_record;", code, flags=re.S).group(1)
    assert re.findall(r"int64_t\s+(\w+);", body) == [f[0] for f in capi.MldLeavingRecord._fields_]
    import ctypes
    assert ctypes.sizeof(capi.MldLeavingRecord) == 32


def test_library_exports_and_capi_binds_them():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mld_abi_version() == 8
    # no object, no work: both refuse a null store before they look at anything else
    assert lib.mld_tracks_export_leaving_device(None, None, *([None] * 9)) == capi.MLD_ERR_INVALID_ARG
    assert lib.mld_tracks_set_leaving_sink(None, *([None] * 9)) == capi.MLD_ERR_INVALID_ARG
    sig = {s[0]: s for s in capi._SIGNATURES}
    assert len(sig[NEW[0]][2]) == 11 and len(sig[NEW[1]][2]) == 10  # the sink: the export's arguments without `flush`
    assert sig[NEW[0]][2][2:] == sig[NEW[1]][2][1:]


def _recording(rng, frames, n, keep_frac, immortal):
    """Per frame (ids, six feature arrays): `immortal` ids live through the whole recording, the rest churns; one
    frame without survivors among the mortal tracks and one in which nothing changes."""
    next_id, prev, out = 1000, np.zeros(0, np.int64), []
    for f in range(frames):
        if f == frames // 2:
            mortal = prev  # nothing leaves
        else:
            k = 0 if f == frames // 3 else int(len(prev) * keep_frac)
            kept = rng.choice(prev, k, replace=False) if k else np.zeros(0, np.int64)
            fresh = np.arange(next_id, next_id + n - k)
            next_id += n - k
            mortal = np.concatenate([kept, fresh])
        ids = np.concatenate([np.arange(immortal), mortal]).astype(np.int64)
        rng.shuffle(ids)
        m = len(ids)
        feats = [rng.uniform(-3, 1245, m).astype(np.float32) for _ in range(4)]
        depths = [rng.uniform(0, 80, m).astype(np.float32) for _ in range(2)]
        for d in depths:
            d[rng.random(m) < 0.2] = -1.0
            d[rng.random(m) < 0.02] = np.nan
        out.append((ids.astype(np.int32), *feats, *depths))
        prev = mortal
    return out


@pytest.mark.parametrize("max_history", [2, 3, 16])
def test_archive_of_the_capped_streams_equals_the_unbounded_deques(max_history):
    """Two sequences, 24 frames, 5 tracks that live for all of them (they outlive every max_history here) among 40 that
    churn: every track the unbounded model erases - and, at the end of the recording, every track that is left - comes
    out of the archive with the same deque, bit for bit, at the same frame."""
    rng = np.random.default_rng(max_history)
    S, frames = 2, 24
    recs = [_recording(rng, frames, 40, 0.7, 5) for _ in range(S)]
    full, capped, archive = [UnboundedMap() for _ in range(S)], [CappedStore(max_history) for _ in range(S)], TrackArchive(S)
    longest = 0

    def compare(done, erased, what):
        for s in range(S):
            got = {t.id: t.entries for t in done if t.sequence == s}
            assert len(got) == sum(1 for t in done if t.sequence == s)  # every track once
            assert sorted(got) == [k for k, _ in erased[s]], (what, s)
            for k, e in erased[s]:
                assert got[k].shape == e.shape and np.array_equal(bits(got[k]), bits(e)), (what, s, k)

    for f in range(frames):
        done = archive.push([as_frame(*capped[s].leaving(recs[s][f][0])) for s in range(S)])
        erased = []
        for s in range(S):
            capped[s].commit(*recs[s][f])
            erased.append(full[s].frame(*recs[s][f]))
        compare(done, erased, f)
        longest = max([longest] + [len(e) for er in erased for _, e in er])
    done = archive.push([as_frame(*capped[s].leaving(flush=True)) for s in range(S)])
    erased = [full[s].end() for s in range(S)]
    compare(done, erased, "end")
    assert max(len(e) for _, e in erased[0]) == frames + 1 > max_history  # the immortal tracks: 25 entries
    assert longest > max_history or max_history == 16  # churned tracks outlive the cap too
    assert all(not archive.open_tracks(s) for s in range(S))


def test_archive_refuses_a_truncated_frame():
    st = CappedStore(2)
    z = np.zeros(3, np.float32)
    st.commit(np.arange(3, dtype=np.int32), z, z, z, z, z, z)
    frame = as_frame(*st.leaving(flush=True))
    frame["ids"] = frame["ids"][:2]
    frame["offsets"] = frame["offsets"][:3]
    with pytest.raises(ValueError, match="truncated"):
        TrackArchive(1).push([frame])
