/*
 * swimhip_watch.h — the subject watch of libswimhip (engine only; the CPU oracle has no such call).
 *
 * Every experiment ends in a question about a few subjects: how long until everyone has suspected or removed the member
 * that was killed, has the joiner's record or the new incarnation reached everybody, and when did each observer get it
 * (the reference's tests: awaitUntil / awaitSeconds followed by assertTrusted / assertSuspected / assertNoSuspected).
 * swim_view_census answers it by streaming the whole N x N key plane. A question about K subjects is a question about K
 * columns of the table: N bytes per subject. A watch is a persistent object on a handle for up to 256 subjects; one
 * read-only kernel samples it: it tallies those columns over the counted observers and stamps each
 * observer's first-seen ticks. swim_run_until steps the handle until a stated condition on the tallies holds.
 *
 * A sample describes the state at rest between ticks: exactly what swim_view_census with the same mask returns for
 * those subjects at the same moment, and what swim_read_row of every counted observer returns. It reads the key plane
 * (its 8-bit shadow where the handle keeps one) and the members' stop ticks, and writes nothing the simulation reads:
 * a run with samples interleaved is bit-identical to a run without them (SEMANTICS.md §8).
 *
 * Counted observers are the census's: with observers == NULL every member running at the sample's tick, evaluated at
 * each sample; an explicit mask (copied at create) is taken literally, a killed member's frozen row included.
 *
 * Stamps (SWIM_WATCH_STAMPS): the tick of the first sample at which the predicate held for (subject j, observer o)
 * while o was counted. Literal: whatever is true at the first sample is stamped with that sample's tick.
 * SWIM_WATCH_NEVER until then, and for observers never counted. Sampling twice at one tick changes nothing. Without
 * inc_target the INC_GE stamps stay NEVER.
 *
 * Handles: a handle with n_gpus > 1 keeps one watch per shard and combines them as the census does (counts and
 * n_observers add, key ranges widen, stamp rows are disjoint). One shard of swim_create_sharded samples its own
 * observers only (every other stamp word stays NEVER); its partial results combine the same way, and swim_run_until on
 * it is SWIM_EUNSUPPORTED because the verdict needs every shard's tallies. SWIM_MODE_RUMOR handles (implicit views
 * included) are SWIM_EUNSUPPORTED: their views never change.
 *
 * The watch's device memory is its own allocation, made once at create and reused by every sample; it is not part of
 * swim_counters.device_bytes. swim_destroy frees the handle's remaining watches.
 *
 * A sample is a host call between two steps. swimhip_watch_series.h arms a recording instead: the engine takes the
 * samples itself behind the ticks inside swim_step and keeps them as a series.
 */
#ifndef SWIMHIP_WATCH_H
#define SWIMHIP_WATCH_H

#include <stddef.h>
#include <stdint.h>

#include "swimhip.h"
#include "swimhip_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWIM_WATCH_MAX_SUBJECTS 256u
#define SWIM_WATCH_NEVER 0xFFFFFFFFu
#define SWIM_WATCH_STAMPS 1u /* flag: keep the per-observer first-seen ticks */
/* the kernel's block (one workgroup): this many consecutive observers, one per lane */
#define SWIM_WATCH_BLOCK_ROWS 256u
/* stamps */
#define SWIM_STAMP_NOT_ALIVE 0u /* status != ALIVE (SUSPECT, ABSENT or DEAD) */
#define SWIM_STAMP_GONE 1u      /* status ABSENT or DEAD */
#define SWIM_STAMP_INC_GE 2u    /* held (status != ABSENT) and incarnation >= inc_target[j] */
/* conditions of swim_run_until / swim_watch_met: they must hold for EVERY watched subject */
#define SWIM_UNTIL_CONVERGED 0u /* counts[ABSENT] == 0 && key_min == key_max  (the census's convergence) */
#define SWIM_UNTIL_NOT_ALIVE 1u /* counts[ALIVE] == 0 */
#define SWIM_UNTIL_GONE 2u      /* counts[ALIVE] == 0 && counts[SUSPECT] == 0 */
#define SWIM_UNTIL_INC_GE 3u    /* counts[ABSENT] == 0 && key_min >> 2 >= inc_target[j] */

typedef struct swim_watch swim_watch;
/* (a struct tag only, no typedef: the tag shares its name with the function below, which C and C++ both allow) */
struct swim_watch_sample {
  uint64_t tick, n_observers;
  uint32_t* counts;  /* [4*K] counts[4*j+st], may be NULL */
  uint32_t* key_min; /* [K], may be NULL; nobody holds it: 0xFFFFFFFF / 0, as the census */
  uint32_t* key_max;
  uint32_t path; /* SWIM_CENSUS_PATH_KEY8 / KEY32 */
  uint32_t reserved[3];
};

/* subjects: k distinct member ids, 1 <= k <= SWIM_WATCH_MAX_SUBJECTS; outputs keep the caller's order.
 * inc_target: [k] or NULL. observers: n_members bytes, copied; NULL = every running member at each sample. */
int swim_watch_create(swim_handle* h, const uint32_t* subjects, uint32_t k, const uint32_t* inc_target,
                      const uint8_t* observers, uint32_t flags, swim_watch** out);
int swim_watch_destroy(swim_watch* w);
/* one memset, one kernel and one copy back, queued on the handle's stream behind the ticks already queued and waited
 * for; reports a pending device error like the other readbacks */
int swim_watch_sample(swim_watch* w, struct swim_watch_sample* out);
/* out[j * n_members + o], cap >= k * n_members words; which = SWIM_STAMP_*; needs SWIM_WATCH_STAMPS */
int swim_watch_stamps(swim_watch* w, uint32_t which, uint32_t* out, size_t cap);
/* 1 / 0, pure host arithmetic; negative: bad arguments (inc_target is needed by SWIM_UNTIL_INC_GE only) */
int swim_watch_met(uint32_t cond, uint32_t k, const uint32_t* counts, const uint32_t* key_min, const uint32_t* key_max,
                   const uint32_t* inc_target);
/* Samples first: if cond already holds, *ticks_run = 0 and the handle's tick is unchanged. Otherwise repeats
 * swim_step(min(check_every, ticks left)) followed by a sample, and stops at the first sample that meets cond
 * (*met = 1) or after max_ticks ticks (*met = 0). A host loop over swim_step: the answer's resolution is check_every
 * ticks. last, if not NULL, receives the final sample (its array pointers are the caller's, as in swim_watch_sample). */
int swim_run_until(swim_handle* h, swim_watch* w, uint32_t cond, uint32_t max_ticks, uint32_t check_every,
                   uint32_t* ticks_run, uint32_t* met, struct swim_watch_sample* last);

#ifdef __cplusplus
}
#endif
#endif
