"""TrackArchive: every track once and complete, from the two streams of mld_tracks_export_leaving_device.

The store keeps at most max_history entries per track and forgets a track when it ends.  Ahead of every commit the
leaving export hands out the entries the commit is about to overwrite (spilled) and the tracks it is about to erase
(ended).  The archive appends a track's spilled entries to the tail of its record and closes the record when the track
ends: the closed record is the reference's unbounded deque at the moment TidyUpTracklets erases it
(tracklet_depth_module.cpp:171-193).  Host side, NumPy only.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np


class ArchivedTrack(NamedTuple):
    sequence: int
    id: int
    entries: np.ndarray  # [length, 3] float32 (u, v, d), newest first


class TrackArchive:
    """push() takes one leaving export (one frame) of all sequences and returns the tracks it completes.

    A frame is a list with one entry per sequence: a mapping with "ids" [t] int32, "offsets" [t + 1] int64, "fp"
    [e, 3] float32, "spill_ids" [p] int32, "spill_fp" [p, 3] float32 and optionally "record" (n_ended, n_ended_entries,
    n_spilled, ...) - what TrackletStore.leaving_host() returns.  With a record, a truncated sequence raises: an
    archive that misses entries is not complete."""

    def __init__(self, n_seq: int):
        self.S = int(n_seq)
        # per sequence: id -> the spilled entries of the open track, oldest first (the order in which they arrive)
        self._tails: List[Dict[int, List[np.ndarray]]] = [dict() for _ in range(self.S)]
        self.n_closed = 0

    def open_tracks(self, sequence: int) -> Tuple[int, ...]:
        """Ids of the tracks of a sequence that have spilled entries and have not ended."""
        return tuple(self._tails[sequence])

    def push(self, frame) -> List[ArchivedTrack]:
        if len(frame) != self.S:
            raise ValueError(f"expected {self.S} sequences")
        done: List[ArchivedTrack] = []
        for s, f in enumerate(frame):
            ids = np.asarray(f["ids"], dtype=np.int32).reshape(-1)
            off = np.asarray(f["offsets"], dtype=np.int64).reshape(-1)
            fp = np.asarray(f["fp"], dtype=np.float32).reshape(-1, 3)
            sp_ids = np.asarray(f["spill_ids"], dtype=np.int32).reshape(-1)
            sp_fp = np.asarray(f["spill_fp"], dtype=np.float32).reshape(-1, 3)
            rec = f.get("record") if hasattr(f, "get") else None
            if rec is not None and (int(rec[0]) != len(ids) or int(rec[1]) != len(fp) or int(rec[2]) != len(sp_ids)):
                raise ValueError(f"sequence {s}: the export was truncated (record {[int(x) for x in rec[:3]]}, held "
                                 f"{len(ids)} tracks, {len(fp)} entries, {len(sp_ids)} spills)")
            if len(ids) and (len(off) != len(ids) + 1 or int(off[-1]) > len(fp)):
                raise ValueError(f"sequence {s}: offsets do not match ids / fp")
            if len(sp_fp) != len(sp_ids):
                raise ValueError(f"sequence {s}: spill_fp does not match spill_ids")
            tails = self._tails[s]
            # a track either ends or spills in one frame, never both: the order of the two loops does not matter
            for k, tid in enumerate(sp_ids.tolist()):
                tails.setdefault(tid, []).append(sp_fp[k].copy())
            for k, tid in enumerate(ids.tolist()):
                head = fp[int(off[k]):int(off[k + 1])]
                tail = tails.pop(tid, [])
                entries = np.concatenate([head, np.asarray(tail[::-1], dtype=np.float32).reshape(-1, 3)]) if tail else head.copy()
                done.append(ArchivedTrack(s, tid, entries))
        self.n_closed += len(done)
        return done
