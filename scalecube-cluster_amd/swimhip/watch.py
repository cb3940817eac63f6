"""The subject watch (include/swimhip_watch.h): per-subject tallies and per-observer first-seen ticks for up to 256
subjects, sampled by one read-only kernel over those columns of the membership table, and run_until on top of it. It is
what awaitUntil(assertSuspected / assertRemoved / assertTrusted ...) of the reference's tests maps to.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from . import _abi

NEVER = _abi.WATCH_NEVER
_P = C.POINTER(C.c_uint32)


@dataclass
class WatchSample:
    tick: int
    n_observers: int      # rows counted
    counts: np.ndarray    # (K, 4) uint32: counted observers that hold subject j with each status
    key_min: np.ndarray   # (K,) uint32: smallest / largest key (incarnation << 2 | status) among the counted observers
    key_max: np.ndarray   # that hold subject j; nobody: 0xFFFFFFFF / 0
    path: int             # _abi.CENSUS_PATH_KEY8 / KEY32


@dataclass
class WatchSeries:
    """Entries of a recording (include/swimhip_watch_series.h): entry i is the sample of tick ticks[i]."""
    ticks: np.ndarray        # (n,) uint64
    n_observers: np.ndarray  # (n,) uint64
    counts: np.ndarray       # (n, K, 4) uint32
    key_min: np.ndarray      # (n, K) uint32
    key_max: np.ndarray      # (n, K) uint32
    n_recorded: int = 0      # entries complete when it was read (the whole series, not only the range read)

    def __len__(self):
        return len(self.ticks)

    def entry(self, i, path=0) -> WatchSample:
        return WatchSample(tick=int(self.ticks[i]), n_observers=int(self.n_observers[i]), counts=self.counts[i],
                           key_min=self.key_min[i], key_max=self.key_max[i], path=path)


def met(cond, counts, key_min, key_max, inc_target=None) -> bool:
    """Whether condition `cond` (_abi.UNTIL_*) holds for every watched subject: swim_watch_met in numpy."""
    counts = np.asarray(counts).reshape(-1, 4)
    if cond == _abi.UNTIL_CONVERGED:
        ok = (counts[:, _abi.ST_ABSENT] == 0) & (np.asarray(key_min) == np.asarray(key_max))
    elif cond == _abi.UNTIL_NOT_ALIVE:
        ok = counts[:, _abi.ST_ALIVE] == 0
    elif cond == _abi.UNTIL_GONE:
        ok = (counts[:, _abi.ST_ALIVE] == 0) & (counts[:, _abi.ST_SUSPECT] == 0)
    elif cond == _abi.UNTIL_INC_GE:
        if inc_target is None:
            raise ValueError("UNTIL_INC_GE needs inc_target")
        ok = (counts[:, _abi.ST_ABSENT] == 0) & ((np.asarray(key_min, np.uint32) >> np.uint32(2))
                                                 >= np.asarray(inc_target, np.uint32))
    else:
        raise ValueError(f"unknown condition {cond}")
    return bool(np.all(ok))


def combine(parts: Sequence[WatchSample]) -> WatchSample:
    """The whole cluster's sample from its row shards' partial ones: counts and n_observers add, key ranges widen."""
    p0 = parts[0]
    assert all(p.tick == p0.tick for p in parts), "partial samples of different ticks"
    return WatchSample(tick=p0.tick, n_observers=sum(p.n_observers for p in parts),
                       counts=np.sum([p.counts for p in parts], axis=0, dtype=np.uint32),
                       key_min=np.minimum.reduce([p.key_min for p in parts]),
                       key_max=np.maximum.reduce([p.key_max for p in parts]), path=p0.path)


def combine_series(parts: Sequence[WatchSeries]) -> WatchSeries:
    """The whole cluster's series from its row shards' partial ones: combine, entry by entry."""
    p0 = parts[0]
    assert all(np.array_equal(p.ticks, p0.ticks) for p in parts), "partial series of different ticks"
    return WatchSeries(ticks=p0.ticks.copy(), n_observers=np.sum([p.n_observers for p in parts], axis=0, dtype=np.uint64),
                       counts=np.sum([p.counts for p in parts], axis=0, dtype=np.uint32),
                       key_min=np.minimum.reduce([p.key_min for p in parts]),
                       key_max=np.maximum.reduce([p.key_max for p in parts]),
                       n_recorded=min(p.n_recorded for p in parts))


def first_met(series: WatchSeries, cond, inc_target=None) -> Optional[int]:
    """The index of the first entry of `series` that meets `cond` (_abi.UNTIL_*), or None: a host scan with met."""
    for i in range(len(series)):
        if met(cond, series.counts[i], series.key_min[i], series.key_max[i], inc_target):
            return i
    return None


def combine_stamps(parts: Sequence[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """Stamp rows are disjoint: a shard stamps only its own observers and leaves every other word NEVER."""
    for name in parts[0]:
        assert not np.any(np.sum([p[name] != NEVER for p in parts], axis=0) > 1), "stamp rows of the parts overlap"
    return {name: np.minimum.reduce([p[name] for p in parts]) for name in parts[0]}


class Watch:
    """swim_watch on one handle of n members (a SimulatedCluster's, an n_gpus handle's or one shard's)."""

    def __init__(self, lib, handle, n, subjects, inc_target=None, observers=None, stamps=True, check=None):
        _abi.bind_watch(lib)
        self.lib, self.n = lib, n
        self.subjects = [int(s) for s in subjects]
        self.k = len(self.subjects)
        self.inc_target = None if inc_target is None else np.ascontiguousarray(inc_target, dtype=np.uint32)
        self.has_stamps = bool(stamps)
        self._check = check or _raise
        self._w = C.c_void_p()
        subj = np.ascontiguousarray(self.subjects, dtype=np.uint32)
        mask = None
        if observers is not None:
            mask = np.ascontiguousarray(np.asarray(observers) != 0, dtype=np.uint8)
            assert mask.shape == (n,)
        if self.inc_target is not None:
            assert self.inc_target.shape == (self.k,)
        rc = lib.swim_watch_create(handle, subj.ctypes.data_as(_P), self.k,
                                   self.inc_target.ctypes.data_as(_P) if self.inc_target is not None else None,
                                   mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None,
                                   _abi.WATCH_STAMPS if stamps else 0, C.byref(self._w))
        self._check(rc, "swim_watch_create")

    def _struct(self):
        counts, mn, mx = np.zeros((self.k, 4), np.uint32), np.zeros(self.k, np.uint32), np.zeros(self.k, np.uint32)
        s = _abi.SwimWatchSample()
        s.counts, s.key_min, s.key_max = counts.ctypes.data_as(_P), mn.ctypes.data_as(_P), mx.ctypes.data_as(_P)
        return s, (counts, mn, mx)

    @staticmethod
    def _sample_of(s, arrs):
        return WatchSample(tick=int(s.tick), n_observers=int(s.n_observers), counts=arrs[0], key_min=arrs[1],
                           key_max=arrs[2], path=int(s.path))

    def sample(self) -> WatchSample:
        s, arrs = self._struct()
        self._check(self.lib.swim_watch_sample(self._w, C.byref(s)), "swim_watch_sample")
        return self._sample_of(s, arrs)

    def stamps(self) -> Dict[str, np.ndarray]:
        """{"not_alive" | "gone" | "inc_ge": (K, n) uint32}: the tick of the first sample at which the predicate held
        for (subject j, observer o) while o was counted; NEVER until then."""
        out = {}
        for which, name in enumerate(_abi.STAMP_NAMES):
            a = np.zeros((self.k, self.n), np.uint32)
            self._check(self.lib.swim_watch_stamps(self._w, which, a.ctypes.data_as(_P), a.size), "swim_watch_stamps")
            out[name] = a
        return out

    def met(self, cond, sample: Optional[WatchSample] = None) -> bool:
        """Whether `cond` holds on `sample` (default: a fresh one), through swim_watch_met."""
        s = sample or self.sample()
        c, mn, mx = (np.ascontiguousarray(a, dtype=np.uint32) for a in (s.counts, s.key_min, s.key_max))
        rc = self.lib.swim_watch_met(cond, self.k, c.ctypes.data_as(_P), mn.ctypes.data_as(_P), mx.ctypes.data_as(_P),
                                     self.inc_target.ctypes.data_as(_P) if self.inc_target is not None else None)
        if rc < 0:
            self._check(rc, "swim_watch_met")
        return rc == 1

    def run_until(self, handle, cond, max_ticks, check_every=1):
        """swim_run_until on the watch's handle: (met, ticks_run, the last WatchSample)."""
        s, arrs = self._struct()
        ticks, ok = C.c_uint32(), C.c_uint32()
        self._check(self.lib.swim_run_until(handle, self._w, cond, max_ticks, check_every, C.byref(ticks), C.byref(ok),
                                            C.byref(s)), "swim_run_until")
        return bool(ok.value), int(ticks.value), self._sample_of(s, arrs)

    def record(self, every=1, cap=4096):
        """Arm recording (swim_watch_record): from the current tick on the engine samples every `every`-th tick inside
        step(), speculative batches included, into a device series of `cap` entries."""
        self._check(self.lib.swim_watch_record(self._w, every, cap), "swim_watch_record")

    def stop(self):
        """swim_watch_record_stop: the series stays readable."""
        self._check(self.lib.swim_watch_record_stop(self._w), "swim_watch_record_stop")

    def recorded(self) -> int:
        """Entries complete so far."""
        n = C.c_uint32()
        self._check(self.lib.swim_watch_series(self._w, 0, 0, None, None, None, None, None, C.byref(n)),
                    "swim_watch_series")
        return int(n.value)

    def series(self, first=0, n=None) -> WatchSeries:
        """Entries [first, first + n) of the recording (n = None: every complete entry from `first` on; none if `first`
        is past them). A stated range that reaches past the complete entries is refused (SWIM_EINVAL)."""
        have = self.recorded()
        if n is None:
            n = max(have - first, 0)
            first = min(first, have)
        ticks, nobs = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        counts, mn, mx = np.zeros((n, self.k, 4), np.uint32), np.zeros((n, self.k), np.uint32), \
            np.zeros((n, self.k), np.uint32)
        p64 = C.POINTER(C.c_uint64)
        got = C.c_uint32()
        self._check(self.lib.swim_watch_series(self._w, first, n, ticks.ctypes.data_as(p64), nobs.ctypes.data_as(p64),
                                               counts.ctypes.data_as(_P), mn.ctypes.data_as(_P), mx.ctypes.data_as(_P),
                                               C.byref(got)), "swim_watch_series")
        return WatchSeries(ticks, nobs, counts, mn, mx, int(got.value))

    def first_met(self, cond, first=0):
        """(tick, index) of the first recorded entry from `first` on that meets `cond`, or None."""
        s = self.series(first)
        i = first_met(s, cond, self.inc_target)
        return None if i is None else (int(s.ticks[i]), first + i)

    def run_until_recorded(self, handle, cond, max_ticks, chunk=64):
        """swim_run_until_recorded on the watch's handle: (met, met_tick, ticks_run)."""
        tick, ok, ran = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.swim_run_until_recorded(handle, self._w, cond, max_ticks, chunk, C.byref(tick),
                                                     C.byref(ok), C.byref(ran)), "swim_run_until_recorded")
        return bool(ok.value), int(tick.value), int(ran.value)

    def close(self):
        if self._w:
            self.lib.swim_watch_destroy(self._w)
            self._w = C.c_void_p()

    def _orphan(self):
        """The handle was destroyed, and the watch with it."""
        self._w = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupWatch:
    """One watch per shard of a ThreadShardGroup, combined in Python as the n_gpus handle combines them in C. A
    recording is one series per shard, combined on read (combine_series); there is no run_until_recorded here (one
    shard cannot give the verdict, swim_run_until_recorded refuses it): step the group and look at first_met()."""

    def __init__(self, parts: Sequence[Watch]):
        self.parts = list(parts)
        p0 = self.parts[0]
        self.k, self.n, self.subjects, self.inc_target = p0.k, p0.n, p0.subjects, p0.inc_target

    def sample(self) -> WatchSample:
        return combine([p.sample() for p in self.parts])

    def stamps(self):
        return combine_stamps([p.stamps() for p in self.parts])

    def met(self, cond, sample: Optional[WatchSample] = None) -> bool:
        return self.parts[0].met(cond, sample or self.sample())

    def record(self, every=1, cap=4096):
        for p in self.parts:
            p.record(every, cap)

    def stop(self):
        for p in self.parts:
            p.stop()

    def series(self, first=0, n=None) -> WatchSeries:
        return combine_series([p.series(first, n) for p in self.parts])

    def first_met(self, cond, first=0):
        s = self.series(first)
        i = first_met(s, cond, self.inc_target)
        return None if i is None else (int(s.ticks[i]), first + i)

    def close(self):
        for p in self.parts:
            p.close()


def _raise(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed rc={rc}")
