"""A plain numpy restatement of the subject watch (include/swimhip_watch.h) from rows as swim_read_row returns them:
row[s] = inc | status << 32 | ... (0 = no record). The GPU tests compare the engine's samples and stamps against it."""
import numpy as np

ABSENT, ALIVE, SUSPECT, DEAD = 0, 1, 2, 3
NEVER = 0xFFFFFFFF
CONVERGED, NOT_ALIVE, GONE, INC_GE = 0, 1, 2, 3  # SWIM_UNTIL_*
STAMPS = ("not_alive", "gone", "inc_ge")         # SWIM_STAMP_* in order


def columns(rows, observer_ids, subjects):
    """(status, key) of the watched subjects in the counted rows, each [len(observer_ids), K]. rows[o] is observer o's
    row; key = incarnation << 2 | status."""
    subjects = np.asarray(subjects, dtype=np.int64)
    if len(observer_ids) == 0:
        z = np.zeros((0, len(subjects)), np.uint64)
        return z.astype(np.int64), z
    sub = np.stack([np.asarray(rows[o], dtype=np.uint64)[subjects] for o in observer_ids])
    st = ((sub >> np.uint64(32)) & np.uint64(3)).astype(np.int64)
    key = ((sub & np.uint64(0xFFFFFFFF)) << np.uint64(2)) | st.astype(np.uint64)
    return st, key


def tally(rows, observer_ids, subjects):
    """What a sample reports: counts [K, 4], key_min / key_max [K] over the held records (nobody: 0xFFFFFFFF / 0)."""
    st, key = columns(rows, observer_ids, subjects)
    k = len(subjects)
    counts = np.zeros((k, 4), np.uint32)
    for s in range(4):
        counts[:, s] = np.count_nonzero(st == s, axis=0)
    held = st != ABSENT
    mn = np.where(held, key, np.uint64(NEVER)).min(axis=0, initial=np.uint64(NEVER))
    mx = np.where(held, key, np.uint64(0)).max(axis=0, initial=np.uint64(0))
    return dict(n_observers=len(observer_ids), counts=counts, key_min=mn.astype(np.uint32), key_max=mx.astype(np.uint32))


def met(cond, counts, key_min, key_max, inc_target=None):
    """SWIM_UNTIL_*: the condition must hold for every watched subject."""
    out = True
    for j in range(len(counts)):
        c = [int(x) for x in counts[j]]
        if cond == CONVERGED:
            ok = c[ABSENT] == 0 and int(key_min[j]) == int(key_max[j])
        elif cond == NOT_ALIVE:
            ok = c[ALIVE] == 0
        elif cond == GONE:
            ok = c[ALIVE] == 0 and c[SUSPECT] == 0
        elif cond == INC_GE:
            ok = c[ABSENT] == 0 and (int(key_min[j]) >> 2) >= int(inc_target[j])
        else:
            raise ValueError(cond)
        out = out and ok
    return out


class StampRef:
    """First-seen ticks: fed the counted rows once per sample, it keeps the tick of the first sample at which each
    predicate held for (subject j, observer o) while o was counted."""

    def __init__(self, n, subjects, inc_target=None):
        self.n, self.subjects = n, list(subjects)
        self.inc_target = None if inc_target is None else np.asarray(inc_target, dtype=np.uint64)
        self.planes = {name: np.full((len(self.subjects), n), NEVER, np.uint32) for name in STAMPS}

    def feed(self, tick, rows, observer_ids):
        st, key = columns(rows, observer_ids, self.subjects)
        pred = {"not_alive": st != ALIVE, "gone": (st == ABSENT) | (st == DEAD)}
        if self.inc_target is not None:
            pred["inc_ge"] = (st != ABSENT) & ((key >> np.uint64(2)) >= self.inc_target[None, :])
        ids = np.asarray(observer_ids, dtype=np.int64)
        for name, p in pred.items():
            plane = self.planes[name]
            for j in range(len(self.subjects)):
                hit = ids[p[:, j]]
                hit = hit[plane[j, hit] == NEVER]
                plane[j, hit] = tick
