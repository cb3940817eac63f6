"""tests/watch_ref.py (the numpy restatement the GPU tests of the subject watch compare against) on hand-made rows: a
DEAD own record, an absent subject, and keys of 0xFF and above (what the 8-bit shadow plane escapes). No GPU needed."""
import numpy as np

import watch_ref as ref


def rec(st, inc=0, aux=0):
    """A row entry as swim_read_row returns it: inc | status << 32 | aux << 34; 0 = no record."""
    return 0 if st == ref.ABSENT else inc | (st << 32) | (aux << 34)


# 5 members; rows of observers 0..3 (observer 4 is never counted). Subject 3 is absent at observers 0 and 1; observer 2
# holds its own record DEAD (a leaver); subject 1 is at incarnation 63 SUSPECT (key 0xFE), 63 DEAD would be 0xFF,
# incarnation 64 ALIVE is key 0x101; subject 4 is absent everywhere.
ROWS = {
    0: np.array([rec(1), rec(2, 63, aux=5), rec(1, 2), rec(0), rec(0)], np.uint64),
    1: np.array([rec(1), rec(1, 64), rec(1, 2), rec(0), rec(0)], np.uint64),
    2: np.array([rec(1), rec(1, 64, aux=1), rec(3, 3), rec(1, 7), rec(0)], np.uint64),
    3: np.array([rec(2, 0), rec(3, 63), rec(1, 2), rec(1, 7), rec(0)], np.uint64),
}


def test_tally():
    t = ref.tally(ROWS, [0, 1, 2, 3], [0, 1, 2, 3, 4])
    assert t["n_observers"] == 4
    assert t["counts"].tolist() == [[0, 3, 1, 0], [0, 2, 1, 1], [0, 3, 0, 1], [2, 2, 0, 0], [4, 0, 0, 0]]
    assert t["key_min"].tolist() == [1, 0xFE, 9, 29, 0xFFFFFFFF]
    assert t["key_max"].tolist() == [2, 0x101, 15, 29, 0]
    # the caller's order is kept; a subset of observers
    t = ref.tally(ROWS, [3, 1], [4, 1])
    assert t["counts"].tolist() == [[2, 0, 0, 0], [0, 1, 0, 1]]
    assert t["key_min"].tolist() == [0xFFFFFFFF, 0xFF] and t["key_max"].tolist() == [0, 0x101]
    assert t["counts"].sum(axis=1).tolist() == [2, 2]
    # nobody counted
    t = ref.tally(ROWS, [], [0, 1])
    assert t["n_observers"] == 0 and not t["counts"].any()
    assert t["key_min"].tolist() == [0xFFFFFFFF] * 2 and t["key_max"].tolist() == [0, 0]


def test_met():
    t = ref.tally(ROWS, [0, 1, 2, 3], [0, 1, 2, 3, 4])
    one = lambda cond, j, inc=None: ref.met(cond, t["counts"][j:j + 1], t["key_min"][j:j + 1], t["key_max"][j:j + 1], inc)
    assert [one(ref.CONVERGED, j) for j in range(5)] == [False, False, False, False, False]
    assert [one(ref.NOT_ALIVE, j) for j in range(5)] == [False, False, False, False, True]
    assert [one(ref.GONE, j) for j in range(5)] == [False, False, False, False, True]
    assert one(ref.INC_GE, 1, [63]) and not one(ref.INC_GE, 1, [64])
    assert not one(ref.INC_GE, 3, [0])  # absent at two observers
    assert one(ref.INC_GE, 2, [2]) and not one(ref.INC_GE, 2, [3])
    # every subject must meet it
    assert not ref.met(ref.INC_GE, t["counts"][1:3], t["key_min"][1:3], t["key_max"][1:3], [63, 3])
    assert ref.met(ref.INC_GE, t["counts"][1:3], t["key_min"][1:3], t["key_max"][1:3], [63, 2])
    # observers 2 and 3 alone agree on subject 3 (ALIVE at incarnation 7): converged
    t = ref.tally(ROWS, [2, 3], [3])
    assert ref.met(ref.CONVERGED, t["counts"], t["key_min"], t["key_max"])
    # a subject that everyone holds SUSPECT or DEAD is NOT_ALIVE but not GONE
    rows = {0: np.array([rec(2, 1)], np.uint64), 1: np.array([rec(3, 1)], np.uint64)}
    t = ref.tally(rows, [0, 1], [0])
    assert ref.met(ref.NOT_ALIVE, t["counts"], t["key_min"], t["key_max"])
    assert not ref.met(ref.GONE, t["counts"], t["key_min"], t["key_max"])


def test_stamps():
    s = ref.StampRef(5, [1, 3, 2], inc_target=[64, 7, 3])
    s.feed(10, ROWS, [0, 1, 2])   # observer 3 is not counted yet
    s.feed(10, ROWS, [0, 1, 2])   # sampling twice at one tick changes nothing
    N = ref.NEVER
    assert s.planes["not_alive"].tolist() == [[10, N, N, N, N], [10, 10, N, N, N], [N, N, 10, N, N]]
    assert s.planes["gone"].tolist() == [[N, N, N, N, N], [10, 10, N, N, N], [N, N, 10, N, N]]
    assert s.planes["inc_ge"].tolist() == [[N, 10, 10, N, N], [N, N, 10, N, N], [N, N, 10, N, N]]
    rows = dict(ROWS)
    rows[0] = np.array([rec(1), rec(1, 64), rec(1, 2), rec(1, 7), rec(0)], np.uint64)  # refuted, and subject 3 learnt
    s.feed(12, rows, [0, 1, 2, 3])
    assert s.planes["not_alive"].tolist() == [[10, N, N, 12, N], [10, 10, N, N, N], [N, N, 10, N, N]]  # stamps stay
    assert s.planes["gone"].tolist() == [[N, N, N, 12, N], [10, 10, N, N, N], [N, N, 10, N, N]]
    assert s.planes["inc_ge"].tolist() == [[12, 10, 10, N, N], [12, N, 10, 12, N], [N, N, 10, N, N]]
    # no inc_target: the INC_GE stamps stay NEVER
    s = ref.StampRef(5, [1])
    s.feed(3, ROWS, [0, 1, 2, 3])
    assert (s.planes["inc_ge"] == N).all() and s.planes["not_alive"].tolist() == [[3, N, N, 3, N]]
