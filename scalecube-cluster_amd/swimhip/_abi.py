"""ctypes mirror of include/swimhip.h (the C ABI of libswimhip).

The same ABI is exported by the product library (libswimhip.so, gfx950) and, for tests only, by the CPU oracle
(oracle/liboracle_swimref.so). This module only describes the ABI. Choosing a library is the caller's job.
"""
import ctypes as C

SWIM_OK = 0
SWIM_EINVAL = -1
SWIM_ENOMEM = -2
SWIM_EDEVICE = -3
SWIM_ECAPACITY = -4
SWIM_EUNSUPPORTED = -5

INIT_COLD_JOIN = 0
INIT_PRECONVERGED = 1
MODE_FULL, MODE_RUMOR = 0, 1
FLAG_RECORD_EVENTS = 1
FLAG_PROFILE = 2
FLAG_PROFILE_ALL = 4
FLAG_IMPLICIT_VIEWS = 8
FLAG_EMULATOR_COUNTERS = 16

EV_ADDED, EV_REMOVED, EV_UPDATED, EV_GOSSIP = 0, 1, 2, 3
META_NONE = 0xFFFFFFFF
ST_ABSENT, ST_ALIVE, ST_SUSPECT, ST_DEAD = 0, 1, 2, 3
HASH_WORDS = 6  # row, fd list, gossip list, events, gossips held, misc


class SwimConfig(C.Structure):
    _fields_ = [
        ("n_members", C.c_uint32),
        ("tick_ms", C.c_uint32),
        ("latency_ticks", C.c_uint32),
        ("init_mode", C.c_uint32),
        ("seed", C.c_uint64),
        ("sync_interval_ms", C.c_uint32),
        ("sync_timeout_ms", C.c_uint32),
        ("suspicion_mult", C.c_uint32),
        ("ping_interval_ms", C.c_uint32),
        ("ping_timeout_ms", C.c_uint32),
        ("ping_req_members", C.c_uint32),
        ("gossip_interval_ms", C.c_uint32),
        ("gossip_fanout", C.c_uint32),
        ("gossip_repeat_mult", C.c_uint32),
        ("metadata_timeout_ms", C.c_uint32),
        ("mode", C.c_uint32),
        ("flags", C.c_uint32),
        ("n_seeds", C.c_uint32),
        ("seeds", C.c_uint32 * 16),
        ("gossip_slot_cap", C.c_uint32),
        ("pending_fetch_cap", C.c_uint32),
        ("event_cap", C.c_uint32),
        ("n_gpus", C.c_uint32),
        ("device", C.c_uint32),
        ("list_slack", C.c_uint32),
        ("churn_per_period", C.c_uint32),
        ("n_dormant", C.c_uint32),
        ("gossip_ring_cap", C.c_uint32),
        ("delay_cap_ms", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class SwimMemberConfig(C.Structure):
    _fields_ = [
        ("ping_interval_ms", C.c_uint32),
        ("ping_timeout_ms", C.c_uint32),
        ("ping_req_members", C.c_uint32),
        ("sync_group", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class SwimEvent(C.Structure):
    _fields_ = [
        ("tick", C.c_uint32),
        ("observer", C.c_uint32),
        ("seq", C.c_uint32),
        ("type", C.c_uint32),
        ("subject", C.c_uint32),
        ("old_meta", C.c_uint32),
        ("new_meta", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class SwimCounters(C.Structure):
    _fields_ = [
        ("tick", C.c_uint64),
        ("record_compares", C.c_uint64),
        ("row_writes", C.c_uint64),
        ("messages", C.c_uint64),
        ("gossip_messages", C.c_uint64),
        ("events", C.c_uint64),
        ("messages_lost", C.c_uint64),
        ("gossips_created", C.c_uint64),
        ("sync_merges", C.c_uint64),
        ("device_bytes", C.c_uint64),
        ("diff_ns", C.c_uint64),
        ("member_ns", C.c_uint64),
        ("gossip_ns", C.c_uint64),
        ("diff_launches", C.c_uint64),
        ("exchange_ns", C.c_uint64),
        ("diff_msgs", C.c_uint64),
        ("ack_resolved", C.c_uint64),
        ("ack_resolved_total", C.c_uint64),
        ("diff_msgs_total", C.c_uint64),
        ("diff_key_bytes", C.c_uint64),
        ("diff_key_bytes_total", C.c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


# every entry point declared in include/swimhip.h: name -> (restype, argtypes)
_H = C.c_void_p
_U32P = C.POINTER(C.c_uint32)
SIGNATURES = {
    "swim_default_config": (None, [C.POINTER(SwimConfig)]),
    "swim_abi_version": (C.c_uint32, []),
    "swim_create": (C.c_int, [C.POINTER(SwimConfig), C.POINTER(_H)]),
    "swim_destroy": (C.c_int, [_H]),
    "swim_step": (C.c_int, [_H, C.c_uint32]),
    "swim_run_periods": (C.c_int, [_H, C.c_uint32]),
    "swim_sync": (C.c_int, [_H]),
    "swim_kill": (C.c_int, [_H, C.c_uint32]),
    "swim_set_default_loss": (C.c_int, [_H, C.c_uint32]),
    "swim_set_partition": (C.c_int, [_H, _U32P]),
    "swim_unblock_all": (C.c_int, [_H]),
    "swim_set_link_loss": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32]),
    "swim_set_default_link_settings": (C.c_int, [_H, C.c_uint32, C.c_uint32]),
    "swim_set_link_settings": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "swim_emulator_counters": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_unblock_link": (C.c_int, [_H, C.c_uint32, C.c_uint32]),
    "swim_update_incarnation": (C.c_int, [_H, C.c_uint32]),
    "swim_update_metadata": (C.c_int, [_H, C.c_uint32]),
    "swim_leave": (C.c_int, [_H, C.c_uint32]),
    "swim_spread_gossip": (C.c_int, [_H, C.c_uint32, C.c_uint64]),
    "swim_join": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    "swim_set_member_config": (C.c_int, [_H, C.c_uint32, C.POINTER(SwimMemberConfig)]),
    "swim_current_tick": (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    "swim_read_row": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_state_hash": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_read_lists": (C.c_int, [_H, C.c_uint32, _U32P, _U32P, _U32P, _U32P, C.c_size_t, C.POINTER(C.c_int32)]),
    "swim_read_gossips": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_uint64), _U32P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "swim_drain_events": (C.c_int, [_H, C.POINTER(SwimEvent), C.c_size_t, C.POINTER(C.c_size_t)]),
    "swim_counters_get": (C.c_int, [_H, C.POINTER(SwimCounters)]),
    "swim_last_error": (C.c_char_p, [_H]),
    "swim_is_overrides": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "swim_ceil_log2": (C.c_uint32, [C.c_uint32]),
}


# include/swimhip_shard.h (row-sharded multi-GPU handles; exported by libswimhip only, not by the oracle)
TRANSPORT_RCCL = 1
TRANSPORT_HOST = 2
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64,
                          C.POINTER(C.c_uint64))


class SwimShardSpec(C.Structure):
    _fields_ = [
        ("rank", C.c_uint32),
        ("world", C.c_uint32),
        ("transport", C.c_uint32),
        ("chunk_cap", C.c_uint32),
        ("rccl_id", C.c_uint8 * 128),
        ("exchange", EXCHANGE_FN),
        ("ctx", C.c_void_p),
        ("reserved", C.c_uint32 * 8),
    ]


SHARD_SIGNATURES = {
    "swim_rccl_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "swim_create_sharded": (C.c_int, [C.POINTER(SwimConfig), C.POINTER(SwimShardSpec), C.POINTER(_H)]),
    "swim_shard_range": (C.c_int, [_H, _U32P, _U32P]),
}


# include/swimhip_census.h (the cluster-wide view census; exported by libswimhip only, not by the oracle)
CENSUS_PATH_IMPLICIT, CENSUS_PATH_KEY8, CENSUS_PATH_KEY32 = 0, 1, 2
CENSUS_TILE_ROWS, CENSUS_TILE_COLS = 128, 4096  # the kernel's tile: observers x subjects (SWIM_CENSUS_TILE_*)


class SwimCensus(C.Structure):
    _fields_ = [
        ("observers", C.POINTER(C.c_uint8)),
        ("by_subject", _U32P),
        ("by_observer", _U32P),
        ("key_min", _U32P),
        ("key_max", _U32P),
        ("tick", C.c_uint64),
        ("n_observers", C.c_uint64),
        ("records", C.c_uint64 * 4),
        ("bytes_read", C.c_uint64),
        ("path", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


CENSUS_SIGNATURES = {
    "swim_view_census": (C.c_int, [_H, C.POINTER(SwimCensus)]),
}


def bind_census(lib):
    """Attach the census entry point (engine library only)."""
    for name, (res, args) in CENSUS_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


# include/swimhip_watch.h (the subject watch; exported by libswimhip only, not by the oracle)
WATCH_MAX_SUBJECTS, WATCH_NEVER, WATCH_STAMPS, WATCH_BLOCK_ROWS = 256, 0xFFFFFFFF, 1, 256
STAMP_NOT_ALIVE, STAMP_GONE, STAMP_INC_GE = 0, 1, 2
STAMP_NAMES = ["not_alive", "gone", "inc_ge"]
UNTIL_CONVERGED, UNTIL_NOT_ALIVE, UNTIL_GONE, UNTIL_INC_GE = 0, 1, 2, 3


class SwimWatchSample(C.Structure):
    _fields_ = [
        ("tick", C.c_uint64),
        ("n_observers", C.c_uint64),
        ("counts", _U32P),
        ("key_min", _U32P),
        ("key_max", _U32P),
        ("path", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


_W = C.c_void_p
WATCH_SIGNATURES = {
    "swim_watch_create": (C.c_int, [_H, _U32P, C.c_uint32, _U32P, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(_W)]),
    "swim_watch_destroy": (C.c_int, [_W]),
    "swim_watch_sample": (C.c_int, [_W, C.POINTER(SwimWatchSample)]),
    "swim_watch_stamps": (C.c_int, [_W, C.c_uint32, _U32P, C.c_size_t]),
    "swim_watch_met": (C.c_int, [C.c_uint32, C.c_uint32, _U32P, _U32P, _U32P, _U32P]),
    "swim_run_until": (C.c_int, [_H, _W, C.c_uint32, C.c_uint32, C.c_uint32, _U32P, _U32P,
                                 C.POINTER(SwimWatchSample)]),
}


# include/swimhip_watch_series.h (recording on a watch: a per-tick series taken inside swim_step)
WATCH_SERIES_MAX_WORDS = 1 << 26
_U64P = C.POINTER(C.c_uint64)
WATCH_SERIES_SIGNATURES = {
    "swim_watch_record": (C.c_int, [_W, C.c_uint32, C.c_uint32]),
    "swim_watch_record_stop": (C.c_int, [_W]),
    "swim_watch_series": (C.c_int, [_W, C.c_uint32, C.c_uint32, _U64P, _U64P, _U32P, _U32P, _U32P, _U32P]),
    "swim_run_until_recorded": (C.c_int, [_H, _W, C.c_uint32, C.c_uint32, C.c_uint32, _U64P, _U32P, _U32P]),
}


def bind_watch(lib):
    """Attach the watch entry points, the recording's included (engine library only)."""
    for name, (res, args) in {**WATCH_SIGNATURES, **WATCH_SERIES_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


# include/swimhip_selftest.h (known-answer surface; exported by libswimhip and by the oracle)
SELFTEST_OVERRIDES, SELFTEST_PHILOX, SELFTEST_CLUSTER_MATH, SELFTEST_LOSS_ROLL = 0, 1, 2, 3
SELFTEST_SIGNATURES = {
    "swim_selftest_eval": (C.c_int, [C.c_uint32, _U32P, _U32P, C.c_size_t, C.c_uint32]),
}


def selftest_eval(lib, op, rows, device=0):
    """Evaluate `op` on a list of input tuples through swim_selftest_eval; returns a list of output tuples."""
    fn = lib.swim_selftest_eval
    fn.restype, fn.argtypes = SELFTEST_SIGNATURES["swim_selftest_eval"]
    win, wout = {SELFTEST_OVERRIDES: (4, 1), SELFTEST_PHILOX: (6, 4), SELFTEST_CLUSTER_MATH: (4, 4),
                 SELFTEST_LOSS_ROLL: (8, 1)}[op]
    flat = [int(x) & 0xFFFFFFFF for r in rows for x in r]
    assert len(flat) == win * len(rows)
    cin = (C.c_uint32 * max(1, len(flat)))(*flat)
    cout = (C.c_uint32 * max(1, wout * len(rows)))()
    rc = fn(op, cin, cout, len(rows), device)
    if rc != 0:
        raise RuntimeError(f"swim_selftest_eval(op={op}) rc={rc}")
    return [tuple(cout[i * wout:(i + 1) * wout]) for i in range(len(rows))]


# include/swimhip_debug.h (capacity-fallback counters; libswimhip only, with SWIM_CAPS / SWIM_FALLBACKS at create)
FB_NAMES = ["trk_walk", "ulog", "creq", "cwmax", "cev_slow", "replay", "mq", "sort_merge", "rx_all"]
DEBUG_SIGNATURES = {
    "swim_debug_fallbacks": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_debug_caps": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_debug_holders": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "swim_debug_set_incarnation": (C.c_int, [_H, C.c_uint32, C.c_uint32]),
    "swim_debug_diff_dirty": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_debug_dirty_check": (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    "swim_debug_light": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_debug_light_sure": (C.c_int, [_H, C.POINTER(C.c_uint64), C.c_size_t]),
    "swim_debug_prim_eval": (C.c_int, [C.c_uint32, _U32P, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_uint32]),
    "swim_debug_receipts_set": (C.c_int, [_H, _U32P, C.c_size_t, _U32P, C.c_size_t, C.c_uint32]),
    "swim_debug_receipts_read": (C.c_int, [_H, C.c_uint32, C.c_uint32, C.c_uint32, _U32P, _U32P]),
}
# swim_debug_receipts_set / _read (include/swimhip_debug.h): record kinds, write-log entries, words per fetch record,
# fixed words per member of the read-back
DEBUG_REC_MEMBER, DEBUG_REC_USER, DEBUG_TL, DEBUG_FREC, DEBUG_RD_WORDS = 0, 1, 16, 8, 25
RD_NAMES = ["tsize", "cidCnt", "nfetch", "fnext", "timerMin", "held", "gCounter", "evSeq", "tl_n"]


def debug_receipts_set(lib, handle, recs, lists, split):
    """Install the next tick's routed receipts (include/swimhip_debug.h swim_debug_receipts_set); the return code.
    recs: 6-word tuples; lists: {member: (ndrop, [record indices])} or a flat word list."""
    fn = lib.swim_debug_receipts_set
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_receipts_set"]
    flat = [int(x) & 0xFFFFFFFF for r in recs for x in r]
    assert len(flat) == 6 * len(recs)
    if isinstance(lists, dict):
        words = []
        for m, (nd, idx) in lists.items():
            words += [m, nd, len(idx), *idx]
    else:
        words = list(lists)
    a = (C.c_uint32 * max(1, len(flat)))(*flat)
    b = (C.c_uint32 * max(1, len(words)))(*[int(x) & 0xFFFFFFFF for x in words])
    return fn(handle, a, len(recs), b, len(words), 1 if split else 0)


def debug_receipts_read(lib, handle, first, n, n_members, fetch_cap=0, messages=False):
    """(rc, out[n][DEBUG_RD_WORDS + DEBUG_FREC * fetch_cap], msg[2 + 3 * n_members] or None) after the injected tick."""
    import numpy as np
    fn = lib.swim_debug_receipts_read
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_receipts_read"]
    out = np.zeros((max(n, 1), DEBUG_RD_WORDS + DEBUG_FREC * fetch_cap), dtype=np.uint32)
    msg = np.zeros(2 + 3 * n_members, dtype=np.uint32) if messages else None
    rc = fn(handle, first, n, fetch_cap, out.ctypes.data_as(_U32P), msg.ctypes.data_as(_U32P) if messages else None)
    return rc, out[:n], msg
# swim_debug_prim_eval: ops, and the sub-ops of PRIM_WAVE and PRIM_ARITH (include/swimhip_debug.h has the layouts)
(PRIM_SCAN, PRIM_SEG_SORT, PRIM_ROUTING, PRIM_WAVE, PRIM_DIRTY, PRIM_ARITH, PRIM_FEISTEL, PRIM_RING_MOVE,
 PRIM_SYNC_DIFF, PRIM_XPACK, PRIM_PACK_B, PRIM_INLINE_IN, PRIM_XUNPACK, PRIM_GOSSIP) = range(14)
# PRIM_GOSSIP's flags (SWIM_PRIM_GS_*)
(GS_APPLY, GS_EM, GS_FB) = (1, 2, 4)
# PRIM_XPACK's flags (SWIM_PRIM_XP_*)
(XP_ACKRES, XP_INLINE, XP_SPEC, XP_HALTED, XP_TLOG, XP_INLINE_OUT) = (1, 2, 4, 8, 16, 32)
# PRIM_XUNPACK's flags (SWIM_PRIM_XU_*)
(XU_END, XU_SPEC, XU_HALTED, XU_ACKRES, XU_INLINE_IN, XU_GOSSIP) = (1, 2, 4, 8, 16, 32)
# PRIM_SYNC_DIFF's flags (SWIM_PRIM_SD_*)
(SD_K8, SD_LISTER, SD_LISTS, SD_SHARDED, SD_DIRTY) = (1, 2, 4, 8, 16)
(WAVE_APPEND, WAVE_RESERVE, WAVE_BLOCK_RESERVE, WAVE_SUM32, WAVE_MIN32, WAVE_SUM64) = range(6)
(ARITH_DIV_GT, ARITH_S16, ARITH_RG, ARITH_KEY8, ARITH_DELAY, ARITH_EPOCH, ARITH_PAYKEY) = range(7)


def prim_eval_rc(lib, op, params, inp, out, device=0):
    """swim_debug_prim_eval on numpy arrays: `inp` (C-contiguous, 8-byte aligned; None: no input) is read and `out`
    is read and written in place; returns the code (SWIM_EINVAL for anything the op's layout does not allow)."""
    fn = lib.swim_debug_prim_eval
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_prim_eval"]
    p = (C.c_uint32 * max(1, len(params)))(*[int(x) & 0xFFFFFFFF for x in params])
    assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and (inp is None or inp.flags["C_CONTIGUOUS"])
    return fn(op, p, len(params), inp.ctypes.data if inp is not None and inp.nbytes else None,
              inp.nbytes if inp is not None else 0, out.ctypes.data, out.nbytes, device)


def prim_eval(lib, op, params, inp, out, device=0):
    """The same, raising on any code but SWIM_OK; returns `out`."""
    rc = prim_eval_rc(lib, op, params, inp, out, device)
    if rc != 0:
        raise RuntimeError(f"swim_debug_prim_eval(op={op}, params={list(params)}) rc={rc}")
    return out
DD_NAMES = ["skipped", "streamed", "msg_skipped", "rebases", "dirty_rows", "pin_decided", "diff_elided", "diff_halts",
            "lister_free_ticks", "lister_free_stops"]
CAP_NAMES = ["slots", "ring", "receipts", "replay", "history", "growths"]


def debug_caps(lib, handle):
    """{name: size} of the structures that grow between ticks (include/swimhip_debug.h swim_debug_caps)."""
    fn = lib.swim_debug_caps
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_caps"]
    out = (C.c_uint64 * len(CAP_NAMES))()
    rc = fn(handle, out, len(CAP_NAMES))
    if rc != 0:
        raise RuntimeError(f"swim_debug_caps rc={rc}")
    return dict(zip(CAP_NAMES, (int(x) for x in out)))


def debug_holders(lib, handle, first, n):
    """[n][5] uint32 array: per member of [first, first + n) its gossip count, receipt-ring head and end positions,
    held-bit popcount and pending folded GOSSIP events (include/swimhip_debug.h swim_debug_holders)."""
    import numpy as np
    fn = lib.swim_debug_holders
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_holders"]
    out = np.zeros((n, 5), dtype=np.uint32)
    rc = fn(handle, first, n, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise RuntimeError(f"swim_debug_holders rc={rc}")
    return out


def debug_set_incarnation(lib, handle, m, inc):
    """Member m's own record at incarnation inc (include/swimhip_debug.h swim_debug_set_incarnation); the return code."""
    fn = lib.swim_debug_set_incarnation
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_set_incarnation"]
    return fn(handle, m, inc)


def debug_diff_dirty(lib, handle, n=len(DD_NAMES)):
    """{name: count} of the SYNC diff's dirty-chunk skipping since create (include/swimhip_debug.h
    swim_debug_diff_dirty); n = 4 leaves out dirty_rows, which costs a pass over the key plane (and what follows it:
    the pinned payloads decided from the masks, the ticks run without a diff launch, the diff-halts)."""
    fn = lib.swim_debug_diff_dirty
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_diff_dirty"]
    out = (C.c_uint64 * len(DD_NAMES))()
    rc = fn(handle, out, n)
    if rc != 0:
        raise RuntimeError(f"swim_debug_diff_dirty rc={rc}")
    return dict(zip(DD_NAMES[:n], (int(x) for x in out)))


# swim_debug_light's entries (include/swimhip_debug.h SWIM_LT_*)
LIGHT_NAMES = ["ticks", "fd", "p1", "sync", "general", "fb_reshuffle", "fb_send", "fb_payloads", "fb_candidates",
               "fb_busy", "fb_status", "fb_other", "on"]


def debug_light(lib, handle):
    """{name: count} of the member kernel's light path since create: member-ticks it finished (and those with an FD
    case, a SYNC receipt, the periodic SYNC send), member-ticks of the general body, fallbacks by reason, and whether
    the next launch takes the path (include/swimhip_debug.h swim_debug_light)."""
    fn = lib.swim_debug_light
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_light"]
    out = (C.c_uint64 * len(LIGHT_NAMES))()
    rc = fn(handle, out, len(LIGHT_NAMES))
    if rc != 0:
        raise RuntimeError(f"swim_debug_light rc={rc}")
    return dict(zip(LIGHT_NAMES, (int(x) for x in out)))


# swim_debug_light_sure's entries (include/swimhip_debug.h SWIM_LS_*)
LIGHT_SURE_NAMES = ["skipped", "first_dead", "min_dead"]


def debug_light_sure(lib, handle):
    """{name: value} of the light path while nobody is dead: member-ticks with the dead lookups skipped, the
    first_dead word and the minimum of the members' dead ticks
    (include/swimhip_debug.h swim_debug_light_sure)."""
    fn = lib.swim_debug_light_sure
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_light_sure"]
    out = (C.c_uint64 * len(LIGHT_SURE_NAMES))()
    rc = fn(handle, out, len(LIGHT_SURE_NAMES))
    if rc != 0:
        raise RuntimeError(f"swim_debug_light_sure rc={rc}")
    return dict(zip(LIGHT_SURE_NAMES, (int(x) for x in out)))


def debug_dirty_check(lib, handle):
    """Clean (row, chunk) pairs that differ from the baseline (the first clean row of the chunk): 0 in a correct engine
    (swim_debug_dirty_check)."""
    fn = lib.swim_debug_dirty_check
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_dirty_check"]
    v = C.c_uint64(0)
    rc = fn(handle, C.byref(v))
    if rc != 0:
        raise RuntimeError(f"swim_debug_dirty_check rc={rc}")
    return int(v.value)


def debug_fallbacks(lib, handle):
    """{name: count} of the capacity fallbacks the handle took (include/swimhip_debug.h)."""
    fn = lib.swim_debug_fallbacks
    fn.restype, fn.argtypes = DEBUG_SIGNATURES["swim_debug_fallbacks"]
    out = (C.c_uint64 * len(FB_NAMES))()
    rc = fn(handle, out, len(FB_NAMES))
    if rc != 0:
        raise RuntimeError(f"swim_debug_fallbacks rc={rc}")
    return dict(zip(FB_NAMES, (int(x) for x in out)))


# include/swimhip_wire.h (wire-format export; libswimhip only)
class SwimWireRecord(C.Structure):
    _fields_ = [("member", C.c_uint32), ("status", C.c_uint32), ("incarnation", C.c_uint32)]


WIRE_SYNC, WIRE_SYNC_ACK = 1, 2
_U8P = C.POINTER(C.c_uint8)
WIRE_SIGNATURES = {
    "swim_wire_sync_frame": (C.c_int, [C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(SwimWireRecord),
                                       C.c_size_t, _U8P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "swim_wire_gossip_frame": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(SwimWireRecord), _U8P,
                                         C.c_size_t, C.POINTER(C.c_size_t)]),
    "swim_export_sync_frame": (C.c_int, [_H, C.c_uint32, C.c_uint32, _U8P, C.c_size_t, C.POINTER(C.c_size_t)]),
}


def bind_wire(lib):
    for name, (res, args) in WIRE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def _frame_call(fn, *args):
    """Call an encoder twice: once for the size, once into a buffer of that size; returns the frame bytes."""
    n = C.c_size_t()
    fn(*args, None, 0, C.byref(n))
    buf = (C.c_uint8 * n.value)()
    rc = fn(*args, buf, n.value, C.byref(n))
    if rc != 0:
        raise RuntimeError(f"{fn.__name__} rc={rc}")
    return bytes(buf)


def wire_sync_frame(lib, kind, sender, records, cid=None, sync_group="default"):
    bind_wire(lib)
    arr = (SwimWireRecord * max(1, len(records)))(*[SwimWireRecord(*r) for r in records])
    return _frame_call(lib.swim_wire_sync_frame, kind, sender, cid.encode() if cid else None, sync_group.encode(),
                       arr, len(records))


def wire_gossip_frame(lib, sender, origin, counter, record):
    bind_wire(lib)
    return _frame_call(lib.swim_wire_gossip_frame, sender, origin, counter, C.byref(SwimWireRecord(*record)))


def export_sync_frame(lib, handle, observer, kind=WIRE_SYNC):
    bind_wire(lib)
    return _frame_call(lib.swim_export_sync_frame, handle, observer, kind)


def bind_shard(lib):
    """Attach the sharding entry points (engine library only)."""
    for name, (res, args) in SHARD_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def bind(lib):
    """Attach restype/argtypes for every ABI symbol; raises AttributeError if one is missing."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load(path):
    # RTLD_LOCAL keeps the oracle's and the engine's identically named swim_* symbols apart in one process
    return bind(C.CDLL(str(path), mode=C.RTLD_LOCAL))
