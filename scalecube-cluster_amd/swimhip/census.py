"""The cluster-wide view census (include/swimhip_census.h): who sees whom as ALIVE, SUSPECT or gone, over every counted
observer's membership table at once. It is what a host-side assertTrusted / assertSuspected / assertNoSuspected over all
members (MembershipProtocolTest.java:625-670) maps to: one read-only pass on the device instead of one row() per member.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi

KEY_NONE_MIN, KEY_NONE_MAX = 0xFFFFFFFF, 0  # key_min / key_max of a subject no counted observer holds


@dataclass
class ViewCensus:
    tick: int
    n_observers: int            # rows counted
    records: np.ndarray         # (4,) uint64: records by status over the counted rows
    by_subject: Optional[np.ndarray]   # (n, 4) uint32: counted observers that hold subject s with each status
    by_observer: Optional[np.ndarray]  # (n, 4) uint32: subjects with each status in o's row (zeros: not counted)
    key_min: Optional[np.ndarray]      # (n,) uint32: smallest / largest key (incarnation << 2 | status) among the
    key_max: Optional[np.ndarray]      # counted observers that hold s; nobody: 0xFFFFFFFF / 0
    path: int                   # _abi.CENSUS_PATH_*
    bytes_read: int

    def trusted_by(self, s):
        """Counted observers that hold subject s ALIVE (assertTrusted over all members)."""
        return int(self.by_subject[s, _abi.ST_ALIVE])

    def suspected_by(self, s):
        """Counted observers that hold subject s SUSPECT (assertSuspected / assertNoSuspected)."""
        return int(self.by_subject[s, _abi.ST_SUSPECT])

    def view_sizes(self):
        """Cluster.members().size() of every observer: its ALIVE + SUSPECT + DEAD records."""
        b = self.by_observer
        return b[:, _abi.ST_ALIVE] + b[:, _abi.ST_SUSPECT] + b[:, _abi.ST_DEAD]

    def converged(self):
        """Per subject: every counted observer holds a record of it, and they all hold the same key."""
        return (self.by_subject[:, _abi.ST_ABSENT] == 0) & (self.key_min == self.key_max)


def combine(parts: Sequence[ViewCensus]) -> ViewCensus:
    """The census of the whole cluster from its row shards' partial ones: counts add, key ranges widen, by_observer rows
    are disjoint (each shard leaves the other shards' observers zero)."""
    p0 = parts[0]

    def fold(name, op):
        arrs = [getattr(p, name) for p in parts]
        if any(a is None for a in arrs):
            return None
        out = arrs[0].copy()
        for a in arrs[1:]:
            out = op(out, a)
        return out

    bo = fold("by_observer", np.add)
    if bo is not None:
        counted = [p.by_observer.any(axis=1) for p in parts]
        assert not np.any(np.sum(counted, axis=0) > 1), "by_observer rows of the parts overlap"
    return ViewCensus(tick=p0.tick, n_observers=sum(p.n_observers for p in parts),
                      records=np.sum([p.records for p in parts], axis=0, dtype=np.uint64),
                      by_subject=fold("by_subject", np.add), by_observer=bo,
                      key_min=fold("key_min", np.minimum), key_max=fold("key_max", np.maximum),
                      path=p0.path, bytes_read=sum(p.bytes_read for p in parts))


def view_census(lib, handle, n, observers=None, by_subject=True, by_observer=True, keys=True):
    """swim_view_census on a handle of n members; returns (rc, ViewCensus). observers: None = every running member,
    else n flags (non-zero = count this observer's row)."""
    _abi.bind_census(lib)
    c = _abi.SwimCensus()
    mask = None
    if observers is not None:
        mask = np.ascontiguousarray(np.asarray(observers) != 0, dtype=np.uint8)
        assert mask.shape == (n,)
        c.observers = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    P = C.POINTER(C.c_uint32)
    bs = np.zeros((n, 4), dtype=np.uint32) if by_subject else None
    bo = np.zeros((n, 4), dtype=np.uint32) if by_observer else None
    mn = np.zeros(n, dtype=np.uint32) if keys else None
    mx = np.zeros(n, dtype=np.uint32) if keys else None
    if bs is not None:
        c.by_subject = bs.ctypes.data_as(P)
    if bo is not None:
        c.by_observer = bo.ctypes.data_as(P)
    if keys:
        c.key_min, c.key_max = mn.ctypes.data_as(P), mx.ctypes.data_as(P)
    rc = lib.swim_view_census(handle, C.byref(c))
    return rc, ViewCensus(tick=int(c.tick), n_observers=int(c.n_observers),
                          records=np.array(list(c.records), dtype=np.uint64), by_subject=bs, by_observer=bo,
                          key_min=mn, key_max=mx, path=int(c.path), bytes_read=int(c.bytes_read))
