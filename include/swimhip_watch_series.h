/*
 * swimhip_watch_series.h — recording on a subject watch (swimhip_watch.h): a per-tick series of its tallies, taken by
 * the engine itself inside swim_step, speculative batches included (engine only).
 *
 * swim_watch_sample is a host call: it can only look between two swim_step calls, so a dissemination curve at tick
 * resolution costs a host wait per tick and gives up the batches. An armed recording queues the same kernel on the
 * engine stream behind every tick that comes to rest, with no host wait of its own, and writes each sample into its
 * own entry of a device series. Inside a speculative batch the launch reads the halt words like every other launch of
 * the batch (csrc/spec.h, halted_sample) and returns at once when the state it was queued to describe does not exist
 * yet; the host queues that sample again where it resumes. Each sample that ran leaves its tick in its entry, and
 * swim_watch_series refuses an entry without it: a missed sample is an error, never a row of zeros.
 *
 * The samples read what swim_watch_sample reads and write only the watch's own memory: a run with a recording armed
 * is bit-identical to a run without one, and cuts its batches at the same ticks (SEMANTICS.md §8).
 *
 * Kept apart from swimhip_watch.h, whose declarations, struct layouts and constants do not change.
 */
#ifndef SWIMHIP_WATCH_SERIES_H
#define SWIMHIP_WATCH_SERIES_H

#include <stdint.h>

#include "swimhip_watch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest series: cap * (5 K + 4) words may not exceed this many (256 MiB; K = 256 subjects: 52 000 entries,
 * K = 1: 7.4 million) */
#define SWIM_WATCH_SERIES_MAX_WORDS (1u << 26)

/* Arm recording on a watch. From the handle's current tick t0 on, the engine itself takes a sample of the state at
 * rest at every tick t0, t0 + every, t0 + 2 every, ... that swim_step passes (the one at t0 is taken by this call,
 * which waits for it), queued on the engine stream behind that tick's last kernel with no host wait of its own, into
 * entry (t - t0) / every of a device series of `cap` entries allocated here (the watch's own memory, like the rest of
 * it). After `cap` entries recording stops by itself. Stamps (SWIM_WATCH_STAMPS) are stamped by these samples with
 * their own ticks: resolution `every`, not the step size. A call while a recording is armed and not yet full:
 * SWIM_EINVAL; otherwise the previous series is dropped. every >= 1, cap >= 1,
 * cap * (5 K + 4) <= SWIM_WATCH_SERIES_MAX_WORDS (SWIM_EINVAL above it). A host call that changes the cluster between
 * two steps (swim_kill, ...) comes after the sample of that tick, as it comes after a swim_watch_sample made before it. */
int swim_watch_record(swim_watch* w, uint32_t every, uint32_t cap);
/* keeps the series readable; a later swim_watch_record starts a new one. Without a recording: SWIM_EINVAL */
int swim_watch_record_stop(swim_watch* w);
/* entries [first, first + n) of the series, each output optional (NULL): ticks [n] (u64), n_observers [n] (u64),
 * counts [n][4 K], key_min [n][K], key_max [n][K], in the caller's subject order, the same numbers swim_watch_sample
 * would have returned at that tick. *n_recorded (optional) = entries complete so far (ticks <= swim_current_tick).
 * first + n > *n_recorded: SWIM_EINVAL (n = 0 only asks for *n_recorded). Waits for the stream; reports a pending
 * device error like the other readbacks, and an entry whose sample did not run as SWIM_EDEVICE (its tick is in
 * swim_last_error). An n_gpus handle combines its shards' entries as samples are combined; one shard of
 * swim_create_sharded returns its partial series. */
int swim_watch_series(swim_watch* w, uint32_t first, uint32_t n, uint64_t* ticks, uint64_t* n_observers,
                      uint32_t* counts, uint32_t* key_min, uint32_t* key_max, uint32_t* n_recorded);
/* Looks at the entries from the handle's current tick on, then steps in calls of `chunk` ticks (so the batches stay
 * speculative), looking at the new entries after each, until an entry meets cond (swim_watch_met; *met = 1) or
 * max_ticks ran or the series is full (*met = 0). *met_tick = tick of the first entry that met it (exact to `every`);
 * *ticks_run >= met_tick - start tick, overshooting by less than chunk. Needs an armed recording (SWIM_EINVAL);
 * chunk >= 1. One shard of swim_create_sharded: SWIM_EUNSUPPORTED, as swim_run_until. */
int swim_run_until_recorded(swim_handle* h, swim_watch* w, uint32_t cond, uint32_t max_ticks, uint32_t chunk,
                            uint64_t* met_tick, uint32_t* met, uint32_t* ticks_run);

#ifdef __cplusplus
}
#endif
#endif
