"""Recording on a subject watch at the C-ABI boundary (include/swimhip_watch_series.h) and its host-side helpers: no GPU
needed.

The four entry points live in a header of their own (include/swimhip_watch.h keeps its declarations as they are); the
header, the ctypes mirror and the built library must agree, and include/swimhip.h (which the oracle exports in full)
declares none of them. swimhip.watch.combine_series is combine applied entry by entry; first_met is a host scan that must
agree with tests/watch_ref.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from swimhip import LIB_PATH, _abi
from swimhip.watch import WatchSample, WatchSeries, combine, combine_series, first_met

import watch_ref as ref

INCLUDE = Path(__file__).resolve().parent.parent / "include"
HEADER = INCLUDE / "swimhip_watch_series.h"
NEW = {"swim_watch_record", "swim_watch_record_stop", "swim_watch_series", "swim_run_until_recorded"}


def code(header):
    return re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)


def declared_symbols(header):
    return set(re.findall(r"\b(swim_[a-z0-9_]+)\s*\(", code(header)))


@pytest.fixture(scope="module")
def lib():
    if not LIB_PATH.exists():
        pytest.skip("libswimhip.so not built (run __graft_entry__.build())")
    return _abi.bind_watch(_abi.load(LIB_PATH))  # loading initialises no device


def test_header_and_ctypes_agree():
    assert declared_symbols(HEADER) == set(_abi.WATCH_SERIES_SIGNATURES) == NEW
    m = re.search(r"#define SWIM_WATCH_SERIES_MAX_WORDS\s+\(1u << (\d+)\)", HEADER.read_text())
    assert m and 1 << int(m.group(1)) == _abi.WATCH_SERIES_MAX_WORDS
    # the watch's own header is as it was: the series header includes it, not the other way round
    assert not declared_symbols(INCLUDE / "swimhip_watch.h") & NEW
    assert '#include "swimhip_watch.h"' in HEADER.read_text()


def test_engine_library_exports_the_symbols(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    # null arguments are refused before any device call
    n = C.c_uint32(7)
    assert lib.swim_watch_record(None, 1, 1) == _abi.SWIM_EINVAL
    assert lib.swim_watch_record_stop(None) == _abi.SWIM_EINVAL
    assert lib.swim_watch_series(None, 0, 0, None, None, None, None, None, C.byref(n)) == _abi.SWIM_EINVAL
    t, m, r = C.c_uint64(), C.c_uint32(), C.c_uint32()
    assert lib.swim_run_until_recorded(None, None, 0, 1, 1, C.byref(t), C.byref(m), C.byref(r)) == _abi.SWIM_EINVAL


def test_main_header_declares_no_series_symbol(oracle):
    assert not declared_symbols(INCLUDE / "swimhip.h") & NEW
    assert not set(_abi.WATCH_SERIES_SIGNATURES) & (set(_abi.SIGNATURES) | set(_abi.WATCH_SIGNATURES))
    for name in NEW:  # the oracle has no watch
        assert not hasattr(oracle, name), name


# rows of four observers over three members, at three ticks: observer 3 alone holds member 2, a SUSPECT record spreads
def rows_at(step):
    A, S, D = 1 << 32, 2 << 32, 3 << 32
    r = {0: [A, S | 63 if step else A | 63, 0], 1: [A, A | 64 if step < 2 else D | 64, 0],
         2: [S | 1, A | 64, 0], 3: [A | 1, (D if step == 2 else A) | 63, A | 9]}
    return {o: np.array(v, np.uint64) for o, v in r.items()}


def series_of(ids, subjects, steps=(0, 1, 2), t0=5, every=3):
    ts = [ref.tally(rows_at(s), ids, subjects) for s in steps]
    return WatchSeries(ticks=np.array([t0 + every * i for i in range(len(steps))], np.uint64),
                       n_observers=np.array([t["n_observers"] for t in ts], np.uint64),
                       counts=np.stack([t["counts"] for t in ts]), key_min=np.stack([t["key_min"] for t in ts]),
                       key_max=np.stack([t["key_max"] for t in ts]), n_recorded=len(steps))


@pytest.mark.parametrize("split", [[(0, 2), (2, 4)], [(0, 1), (1, 3), (3, 4)]], ids=["two", "three"])
def test_combine_series(split):
    subjects = [2, 0, 1]
    whole = series_of(range(4), subjects)
    parts = [series_of(range(lo, hi), subjects) for lo, hi in split]
    got = combine_series(parts)
    assert np.array_equal(got.ticks, whole.ticks) and got.ticks.tolist() == [5, 8, 11]
    assert got.n_observers.tolist() == [4, 4, 4] and got.n_recorded == 3
    for f in ("counts", "key_min", "key_max"):
        assert np.array_equal(getattr(got, f), getattr(whole, f)), f
        assert getattr(got, f).dtype == np.uint32
    assert got.counts.shape == (3, 3, 4) and got.key_min.shape == (3, 3)
    assert not np.array_equal(got.counts[0], got.counts[2])  # the entries differ: nothing is compared with itself
    # ... and entry by entry it is combine
    for i in range(3):
        one = combine([p.entry(i) for p in parts])
        e = got.entry(i)
        assert (one.tick, one.n_observers) == (e.tick, e.n_observers)
        for f in ("counts", "key_min", "key_max"):
            assert np.array_equal(getattr(one, f), getattr(e, f)), (i, f)
    with pytest.raises(AssertionError):
        combine_series([series_of([0], subjects), series_of([1], subjects, t0=6)])


def test_first_met():
    everyone = range(4)
    # member 1 is not ALIVE anywhere only at the last step; member 0 is SUSPECT at observer 2 throughout
    mid = series_of(everyone, [1], steps=(0, 1, 1, 2, 2))
    want = [ref.met(ref.NOT_ALIVE, mid.counts[i], mid.key_min[i], mid.key_max[i]) for i in range(5)]
    assert want == [False, False, False, False, False]  # observer 2 keeps it ALIVE
    some = series_of([0, 1, 3], [1], steps=(0, 1, 1, 2, 2))
    want = [ref.met(ref.NOT_ALIVE, some.counts[i], some.key_min[i], some.key_max[i]) for i in range(5)]
    assert want == [False, False, False, True, True]
    assert first_met(some, _abi.UNTIL_NOT_ALIVE) == 3          # in the middle
    assert first_met(mid, _abi.UNTIL_NOT_ALIVE) is None        # never
    assert first_met(mid, _abi.UNTIL_GONE) is None
    held = series_of(everyone, [0, 1])                         # everyone holds members 0 and 1 from the start
    assert first_met(held, _abi.UNTIL_INC_GE, [0, 63]) == 0    # at entry 0
    assert first_met(held, _abi.UNTIL_INC_GE, [0, 64]) is None
    assert first_met(held, _abi.UNTIL_INC_GE, [2, 0]) is None
    for s, subjects in ((mid, [1]), (some, [1]), (held, [0, 1])):
        for cond, inc in ((ref.CONVERGED, None), (ref.NOT_ALIVE, None), (ref.GONE, None), (ref.INC_GE, [0] * len(subjects))):
            want = [ref.met(cond, s.counts[i], s.key_min[i], s.key_max[i], inc) for i in range(len(s))]
            assert first_met(s, cond, inc) == (want.index(True) if True in want else None), (subjects, cond)
    empty = WatchSeries(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 1, 4), np.uint32),
                        np.zeros((0, 1), np.uint32), np.zeros((0, 1), np.uint32))
    assert len(empty) == 0 and first_met(empty, _abi.UNTIL_GONE) is None
