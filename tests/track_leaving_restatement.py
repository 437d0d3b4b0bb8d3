"""Plain Python / NumPy models for the leaving export of the tracklet store (mld_tracks_export_leaving_device).

UnboundedMap   `_trackletMap` as the reference keeps it: a dict of UNBOUNDED lists (newest first), driven by
               SaveFeatureDepths (tracklet_depth_module.cpp:119-169) and TidyUpTracklets (:171-193) as they are written:
               a new track is created with the previous feature ((int)u_old, (int)v_old, d_last) and then gets
               ((int)u_new, (int)v_new, d_cur) pushed to the front like every other track; every track without an update
               is erased, in the order of the std::map (ascending id).  d_last is indexed per track, as the store's
               commit takes it (the reference compacts it over the new tracks).  frame() returns the erased tracks
               with their deques at the moment of erasure.
CappedStore    the store: the same map with at most max_history entries per track, plus what the leaving export hands
               out between a begin and its commit - the ended tracks in the committed frame's order and, for the
               continuing tracks that are full, the entry the commit's push overwrites.

A repeated id within a frame is stored once; both models keep the FIRST occurrence (the store leaves open which one:
tests that repeat ids compare only what does not depend on it).
"""
import numpy as np


def trunc(a):
    """std::pair<int, int>: truncation toward zero, stored as the float of the integer."""
    return np.asarray(a, dtype=np.float32).astype(np.int32).astype(np.float32)


def _entries(hist):
    return np.array(hist, dtype=np.float32).reshape(len(hist), 3)


class UnboundedMap:
    def __init__(self):
        self.map = {}

    def frame(self, ids, u_new, v_new, u_old, v_old, d_cur, d_last):
        """One process() call.  Returns [(id, entries [L, 3] newest first)] of the tracks TidyUpTracklets erases."""
        un, vn, uo, vo = trunc(u_new), trunc(v_new), trunc(u_old), trunc(v_old)
        updated = set()
        for i, tid in enumerate(int(t) for t in ids):
            if tid in updated:
                continue
            if tid not in self.map:                                   # :134-151
                self.map[tid] = [(uo[i], vo[i], np.float32(d_last[i]))]
            self.map[tid].insert(0, (un[i], vn[i], np.float32(d_cur[i])))  # :154-160
            updated.add(tid)                                          # :165
        to_delete = [k for k in sorted(self.map) if k not in updated]  # :175-186
        return [(k, _entries(self.map.pop(k))) for k in to_delete]          # :189-192

    def end(self):
        """The end of the recording: every track that is left, by ascending id."""
        out = [(k, _entries(self.map[k])) for k in sorted(self.map)]
        self.map = {}
        return out


class CappedStore:
    def __init__(self, max_history):
        self.H = int(max_history)
        self.map = {}
        self.order = []  # the ids of the committed frame, message order

    def stored(self):
        """Ids of the committed frame in message order, every id once (its first occurrence)."""
        seen, out = set(), []
        for tid in self.order:
            if tid not in seen:
                seen.add(tid)
                out.append(tid)
        return out

    def leaving(self, next_ids=None, flush=False):
        """What the commit of a frame with `next_ids` removes: (ended [(id, entries)], spilled [(id, entry [3])]), both
        in the committed frame's order.  flush: every track ends, nothing spills (next_ids is not looked at)."""
        nxt = set() if flush else set(int(t) for t in next_ids)
        ended, spilled = [], []
        for tid in self.stored():
            h = self.map[tid]
            if tid not in nxt:
                ended.append((tid, _entries(h)))
            elif len(h) == self.H:
                spilled.append((tid, np.array(h[-1], dtype=np.float32)))
        return ended, spilled

    def commit(self, ids, u_new, v_new, u_old, v_old, d_cur, d_last):
        un, vn, uo, vo = trunc(u_new), trunc(v_new), trunc(u_old), trunc(v_old)
        updated = {}
        for i, tid in enumerate(int(t) for t in ids):
            if tid in updated:
                continue
            hist = self.map.get(tid)
            if hist is None:
                hist = [(uo[i], vo[i], np.float32(d_last[i]))]
            hist.insert(0, (un[i], vn[i], np.float32(d_cur[i])))
            del hist[self.H:]  # push_front on a full ring overwrites the oldest entry
            updated[tid] = hist
        self.map = updated
        self.order = [int(t) for t in ids]

    def reset(self):
        self.map, self.order = {}, []


def as_frame(ended, spilled):
    """The host view of one sequence of a leaving export (TrackletStore.leaving_host) from a model's lists."""
    lens = [len(e) for _, e in ended]
    off = np.zeros(len(ended) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return {"ids": np.array([t for t, _ in ended], dtype=np.int32), "offsets": off,
            "fp": np.concatenate([e for _, e in ended]).reshape(-1, 3) if ended else np.zeros((0, 3), np.float32),
            "spill_ids": np.array([t for t, _ in spilled], dtype=np.int32),
            "spill_fp": np.array([e for _, e in spilled], dtype=np.float32).reshape(-1, 3),
            "record": np.array([len(ended), int(off[-1]), len(spilled), 0], dtype=np.int64)}
