"""The view census at the C-ABI boundary (include/swimhip_census.h) and its host-side helpers: no GPU needed.

The header, the ctypes mirror and the built library must agree; the census stays out of include/swimhip.h (the oracle
exports every symbol of that header and has no census); swimhip.census.combine implements the shard combination the
header documents, and ViewCensus.converged the convergence rule."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from swimhip import LIB_PATH, _abi
from swimhip.census import ViewCensus, combine

INCLUDE = Path(__file__).resolve().parent.parent / "include"
HEADER = INCLUDE / "swimhip_census.h"

# swim_census as the header lays it out on LP64: (field, offset, size)
LAYOUT = [("observers", 0, 8), ("by_subject", 8, 8), ("by_observer", 16, 8), ("key_min", 24, 8), ("key_max", 32, 8),
          ("tick", 40, 8), ("n_observers", 48, 8), ("records", 56, 32), ("bytes_read", 88, 8), ("path", 96, 4),
          ("reserved", 100, 12)]
SIZE = 112


def declared_symbols(header):
    return sorted(set(re.findall(r"\b(swim_[a-z0-9_]+)\s*\(", header.read_text())))


def header_fields():
    """(name, size) of every member of struct swim_census, in declaration order, parsed from the header."""
    text = HEADER.read_text()
    body = re.search(r"typedef struct swim_census \{(.*?)\} swim_census;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const uint8_t\*|uint32_t\*|uint64_t|uint32_t) (.*)", decl)
        assert m, decl
        size = {"const uint8_t*": 8, "uint32_t*": 8, "uint64_t": 8, "uint32_t": 4}[m.group(1)]
        for name in m.group(2).split(","):
            name = name.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", name)
            out.append((arr.group(1), size * int(arr.group(2))) if arr else (name, size))
    return out


def test_header_and_ctypes_agree():
    assert set(declared_symbols(HEADER)) == set(_abi.CENSUS_SIGNATURES) == {"swim_view_census"}


def test_struct_layout_matches_the_header():
    assert header_fields() == [(n, s) for n, _, s in LAYOUT]
    assert C.sizeof(_abi.SwimCensus) == SIZE
    assert [f for f, _ in _abi.SwimCensus._fields_] == [n for n, _, _ in LAYOUT]
    for name, off, size in LAYOUT:
        fld = getattr(_abi.SwimCensus, name)
        assert (fld.offset, fld.size) == (off, size), name
    text = HEADER.read_text()
    for name, v in (("IMPLICIT", _abi.CENSUS_PATH_IMPLICIT), ("KEY8", _abi.CENSUS_PATH_KEY8),
                    ("KEY32", _abi.CENSUS_PATH_KEY32)):
        assert re.search(rf"#define SWIM_CENSUS_PATH_{name}\s+{v}u", text), name
    assert re.search(rf"#define SWIM_CENSUS_TILE_ROWS\s+{_abi.CENSUS_TILE_ROWS}u", text)
    assert re.search(rf"#define SWIM_CENSUS_TILE_COLS\s+{_abi.CENSUS_TILE_COLS}u", text)


def test_engine_library_exports_the_symbol():
    if not LIB_PATH.exists():
        pytest.skip("libswimhip.so not built (run __graft_entry__.build())")
    lib = _abi.bind_census(_abi.load(LIB_PATH))  # loading initialises no device
    assert lib.swim_view_census(None, None) == _abi.SWIM_EINVAL  # a null handle is refused before any device call


def test_main_header_declares_no_census_symbol(oracle):
    assert not [s for s in declared_symbols(INCLUDE / "swimhip.h") if "census" in s]
    assert not set(_abi.CENSUS_SIGNATURES) & set(_abi.SIGNATURES)
    assert not hasattr(oracle, "swim_view_census")  # _abi.load still binds the oracle, which lacks the symbol


def part(n, rows, key=None, path=_abi.CENSUS_PATH_KEY8, tick=7):
    """A hand-made partial census over observers `rows` of an n-member cluster: rows[o] = n statuses; every held record
    has key 4 * inc + status with inc = key[o][s] (default 0)."""
    bs, bo = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint32)
    mn, mx = np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32)
    for o, sts in rows.items():
        for s, st in enumerate(sts):
            bs[s, st] += 1
            bo[o, st] += 1
            if st:
                k = 4 * (key[o][s] if key else 0) + st
                mn[s], mx[s] = min(mn[s], k), max(mx[s], k)
    return ViewCensus(tick=tick, n_observers=len(rows), records=bo.sum(axis=0, dtype=np.uint64), by_subject=bs,
                      by_observer=bo, key_min=mn, key_max=mx, path=path, bytes_read=n * len(rows))


def same(a, b):
    assert (a.tick, a.n_observers, a.path, a.bytes_read) == (b.tick, b.n_observers, b.path, b.bytes_read)
    for f in ("records", "by_subject", "by_observer", "key_min", "key_max"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


ROWS = {0: [1, 1, 2, 0], 1: [1, 1, 1, 0], 2: [2, 1, 1, 0], 3: [1, 0, 3, 1]}
INCS = {0: [0, 5, 1, 0], 1: [0, 5, 2, 0], 2: [3, 5, 2, 0], 3: [3, 0, 2, 9]}


@pytest.mark.parametrize("split", [[(0, 2), (2, 4)], [(0, 1), (1, 3), (3, 4)]], ids=["two", "three"])
def test_combine(split):
    whole = part(4, ROWS, INCS)
    parts = [part(4, {o: ROWS[o] for o in range(lo, hi)}, INCS) for lo, hi in split]
    # subject 3 is held by observer 3 alone: the shards without it report "nobody holds it"
    assert parts[0].key_min[3] == 0xFFFFFFFF and parts[0].key_max[3] == 0
    assert whole.key_min[3] == whole.key_max[3] == 4 * 9 + 1
    for p, (lo, hi) in zip(parts, split):  # disjoint by_observer rows
        assert not p.by_observer[:lo].any() and not p.by_observer[hi:].any()
    got = combine(parts)
    same(got, whole)
    assert np.array_equal(got.records, got.by_observer.sum(axis=0))
    assert np.array_equal(got.by_subject.sum(axis=1), np.full(4, 4))


def test_combine_keeps_switched_off_outputs_off():
    a, b = part(4, {0: ROWS[0]}), part(4, {1: ROWS[1]})
    a.key_min = a.key_max = b.key_min = b.key_max = None
    got = combine([a, b])
    assert got.key_min is None and got.key_max is None and got.n_observers == 2
    assert np.array_equal(got.by_subject, part(4, {0: ROWS[0], 1: ROWS[1]}).by_subject)


def test_converged_and_helpers():
    c = part(4, ROWS, INCS)
    # subject 0: incarnations 0 and 3 and a SUSPECT; 1: absent at observer 3; 2: statuses differ; 3: absent at three
    assert c.converged().tolist() == [False, False, False, False]
    rows = {0: [1, 2, 1, 0], 1: [1, 2, 1, 1], 2: [1, 2, 1, 1]}
    incs = {0: [4, 1, 0, 0], 1: [4, 1, 0, 2], 2: [4, 1, 1, 2]}
    c = part(4, rows, incs)
    # subject 0: ALIVE inc 4 everywhere; 1: SUSPECT inc 1 everywhere; 2: incarnations differ; 3: absent at observer 0
    assert c.converged().tolist() == [True, True, False, False]
    assert c.trusted_by(0) == 3 and c.suspected_by(1) == 3 and c.trusted_by(3) == 2 and c.suspected_by(0) == 0
    assert c.view_sizes().tolist() == [3, 4, 4, 0]
