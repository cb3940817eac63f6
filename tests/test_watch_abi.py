"""The subject watch at the C-ABI boundary (include/swimhip_watch.h) and its host-side helpers: no GPU needed.

The header, the ctypes mirror and the built library must agree; the watch stays out of include/swimhip.h (the oracle
exports every symbol of that header and has no watch); swim_watch_met is pure host arithmetic and must agree with
tests/watch_ref.py; swimhip.watch.combine implements the shard combination the header documents."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from swimhip import LIB_PATH, _abi
from swimhip.watch import WatchSample, combine, combine_stamps, met

import watch_ref as ref

INCLUDE = Path(__file__).resolve().parent.parent / "include"
HEADER = INCLUDE / "swimhip_watch.h"
P = C.POINTER(C.c_uint32)

# struct swim_watch_sample as the header lays it out on LP64: (field, offset, size)
LAYOUT = [("tick", 0, 8), ("n_observers", 8, 8), ("counts", 16, 8), ("key_min", 24, 8), ("key_max", 32, 8),
          ("path", 40, 4), ("reserved", 44, 12)]
SIZE = 56
DEFINES = {"SWIM_WATCH_MAX_SUBJECTS": _abi.WATCH_MAX_SUBJECTS, "SWIM_WATCH_NEVER": _abi.WATCH_NEVER,
           "SWIM_WATCH_STAMPS": _abi.WATCH_STAMPS, "SWIM_WATCH_BLOCK_ROWS": _abi.WATCH_BLOCK_ROWS,
           "SWIM_STAMP_NOT_ALIVE": _abi.STAMP_NOT_ALIVE, "SWIM_STAMP_GONE": _abi.STAMP_GONE,
           "SWIM_STAMP_INC_GE": _abi.STAMP_INC_GE, "SWIM_UNTIL_CONVERGED": _abi.UNTIL_CONVERGED,
           "SWIM_UNTIL_NOT_ALIVE": _abi.UNTIL_NOT_ALIVE, "SWIM_UNTIL_GONE": _abi.UNTIL_GONE,
           "SWIM_UNTIL_INC_GE": _abi.UNTIL_INC_GE}


def code(header):
    return re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)


def declared_symbols(header):
    return sorted(set(re.findall(r"\b(swim_[a-z0-9_]+)\s*\(", code(header))))


def header_fields():
    """(name, size) of every member of struct swim_watch_sample, in declaration order, parsed from the header."""
    body = re.search(r"struct swim_watch_sample \{(.*?)\};", code(HEADER), re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(uint32_t\*|uint64_t|uint32_t) (.*)", decl)
        assert m, decl
        size = {"uint32_t*": 8, "uint64_t": 8, "uint32_t": 4}[m.group(1)]
        for name in m.group(2).split(","):
            name = name.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", name)
            out.append((arr.group(1), size * int(arr.group(2))) if arr else (name, size))
    return out


@pytest.fixture(scope="module")
def lib():
    if not LIB_PATH.exists():
        pytest.skip("libswimhip.so not built (run __graft_entry__.build())")
    return _abi.bind_watch(_abi.load(LIB_PATH))  # loading initialises no device


def test_header_and_ctypes_agree():
    assert set(declared_symbols(HEADER)) == set(_abi.WATCH_SIGNATURES) == {
        "swim_watch_create", "swim_watch_destroy", "swim_watch_sample", "swim_watch_stamps", "swim_watch_met",
        "swim_run_until"}
    text = HEADER.read_text()
    for name, v in DEFINES.items():
        m = re.search(rf"#define {name}\s+(0x[0-9A-Fa-f]+|\d+)u", text)
        assert m and int(m.group(1), 0) == v, name
    assert _abi.STAMP_NAMES == list(ref.STAMPS)
    assert (ref.CONVERGED, ref.NOT_ALIVE, ref.GONE, ref.INC_GE) == (
        _abi.UNTIL_CONVERGED, _abi.UNTIL_NOT_ALIVE, _abi.UNTIL_GONE, _abi.UNTIL_INC_GE)


def test_struct_layout_matches_the_header():
    assert header_fields() == [(n, s) for n, _, s in LAYOUT]
    assert C.sizeof(_abi.SwimWatchSample) == SIZE
    assert [f for f, _ in _abi.SwimWatchSample._fields_] == [n for n, _, _ in LAYOUT]
    for name, off, size in LAYOUT:
        fld = getattr(_abi.SwimWatchSample, name)
        assert (fld.offset, fld.size) == (off, size), name


def test_engine_library_exports_the_symbols(lib):
    w = C.c_void_p()
    subj = (C.c_uint32 * 1)(0)
    # a null handle is refused before any device call
    assert lib.swim_watch_create(None, subj, 1, None, None, 0, C.byref(w)) == _abi.SWIM_EINVAL
    assert not w.value
    assert lib.swim_watch_destroy(None) == _abi.SWIM_EINVAL
    assert lib.swim_watch_sample(None, C.byref(_abi.SwimWatchSample())) == _abi.SWIM_EINVAL
    assert lib.swim_watch_stamps(None, 0, subj, 1) == _abi.SWIM_EINVAL
    t, m = C.c_uint32(), C.c_uint32()
    assert lib.swim_run_until(None, None, 0, 1, 1, C.byref(t), C.byref(m), None) == _abi.SWIM_EINVAL


def test_main_header_declares_no_watch_symbol(oracle):
    names = declared_symbols(INCLUDE / "swimhip.h")
    assert not [s for s in names if "watch" in s or "run_until" in s]
    assert not set(_abi.WATCH_SIGNATURES) & set(_abi.SIGNATURES)
    for name in _abi.WATCH_SIGNATURES:  # _abi.load still binds the oracle, which lacks the symbols
        assert not hasattr(oracle, name), name


def c_met(lib, cond, counts, mn, mx, inc):
    a = [np.ascontiguousarray(x, dtype=np.uint32) if x is not None else None for x in (counts, mn, mx, inc)]
    return lib.swim_watch_met(cond, len(counts), *[x.ctypes.data_as(P) if x is not None else None for x in a])


def test_met_agrees_with_the_reference(lib):
    rng = np.random.default_rng(0x3E7)
    seen = set()
    for i in range(400):
        k = int(rng.integers(1, 5))
        # small numbers, so that zero counts, equal keys and targets on either side of the key all occur
        counts = rng.integers(0, 3, (k, 4)).astype(np.uint32) * rng.integers(0, 2, (k, 4)).astype(np.uint32)
        mn = rng.choice(np.array([1, 5, 9, 0xFE, 0xFF, 0x101, 0x40000001, 0xFFFFFFFF], np.uint32), k)
        mx = np.where(rng.random(k) < 0.6, mn, np.maximum(mn, rng.choice(np.array([2, 0x101, 0x40000002], np.uint32), k)))
        inc = rng.choice(np.array([0, 1, 2, 63, 64, 0x10000000, 0x3FFFFFFF], np.uint32), k)
        for cond in range(4):
            want = ref.met(cond, counts, mn, mx, inc)
            assert c_met(lib, cond, counts, mn, mx, inc) == int(want), (i, cond, counts, mn, mx, inc)
            assert met(cond, counts, mn, mx, inc) == want, (i, cond)
            seen.add((cond, want))
    assert seen == {(c, v) for c in range(4) for v in (False, True)}  # each condition was seen both ways


def test_met_arguments(lib):
    counts, one = np.zeros((1, 4), np.uint32), np.zeros(1, np.uint32)
    assert c_met(lib, 4, counts, one, one, one) == _abi.SWIM_EINVAL  # an unknown condition
    assert lib.swim_watch_met(_abi.UNTIL_GONE, 0, counts.ctypes.data_as(P), None, None, None) == _abi.SWIM_EINVAL
    assert lib.swim_watch_met(_abi.UNTIL_GONE, 257, counts.ctypes.data_as(P), None, None, None) == _abi.SWIM_EINVAL
    assert lib.swim_watch_met(_abi.UNTIL_GONE, 1, None, None, None, None) == _abi.SWIM_EINVAL
    assert c_met(lib, _abi.UNTIL_GONE, counts, None, None, None) == 1  # the counts alone decide GONE and NOT_ALIVE
    assert c_met(lib, _abi.UNTIL_CONVERGED, counts, one, None, None) == _abi.SWIM_EINVAL
    assert c_met(lib, _abi.UNTIL_INC_GE, counts, one, one, None) == _abi.SWIM_EINVAL


ROWS = {o: np.array(r, np.uint64) for o, r in {
    0: [1 << 32, (2 << 32) | 63, 0], 1: [1 << 32, (1 << 32) | 64, 0], 2: [(2 << 32) | 1, (1 << 32) | 64, 0],
    3: [(1 << 32) | 1, (3 << 32) | 63, (1 << 32) | 9]}.items()}


def part(ids, subjects, tick=7):
    t = ref.tally(ROWS, ids, subjects)
    return WatchSample(tick=tick, n_observers=t["n_observers"], counts=t["counts"], key_min=t["key_min"],
                       key_max=t["key_max"], path=_abi.CENSUS_PATH_KEY8)


@pytest.mark.parametrize("split", [[(0, 2), (2, 4)], [(0, 1), (1, 3), (3, 4)]], ids=["two", "three"])
def test_combine(split):
    subjects = [2, 0, 1]
    whole = part(range(4), subjects)
    parts = [part(range(lo, hi), subjects) for lo, hi in split]
    # subject 2 is held by observer 3 alone: the shards without it report "nobody holds it"
    assert parts[0].key_min[0] == 0xFFFFFFFF and parts[0].key_max[0] == 0
    got = combine(parts)
    assert (got.tick, got.n_observers, got.path) == (whole.tick, 4, whole.path)
    for f in ("counts", "key_min", "key_max"):
        assert np.array_equal(getattr(got, f), getattr(whole, f)), f
        assert getattr(got, f).dtype == np.uint32
    assert got.key_min.tolist() == [37, 1, 0xFE] and got.key_max.tolist() == [37, 6, 0x101]
    assert got.counts.sum(axis=1).tolist() == [4, 4, 4]
    with pytest.raises(AssertionError):
        combine([part([0], subjects), part([1], subjects, tick=8)])
    # stamps: disjoint rows, NEVER elsewhere
    stamps = []
    for lo, hi in split:
        s = ref.StampRef(4, subjects)
        s.feed(5, ROWS, range(lo, hi))
        assert all((p[:, :lo] == ref.NEVER).all() and (p[:, hi:] == ref.NEVER).all() for p in s.planes.values())
        stamps.append(s.planes)
    all_ = ref.StampRef(4, subjects)
    all_.feed(5, ROWS, range(4))
    got = combine_stamps(stamps)
    for name in ref.STAMPS:
        assert np.array_equal(got[name], all_.planes[name]), name
    assert (got["not_alive"] != ref.NEVER).any()
    with pytest.raises(AssertionError):
        combine_stamps([all_.planes, all_.planes])
