/*
 * swimhip_census.h — the cluster-wide view census of libswimhip (engine only; the CPU oracle has no such call).
 *
 * Membership tests ask one question over every member's view: who sees whom as ALIVE, SUSPECT or gone, and has a
 * change reached everyone (MembershipProtocolTest.java assertTrusted / assertSuspected / assertNoSuspected, :625-670).
 * swim_read_row answers it one observer per call; the census answers it for all counted observers in one read-only
 * pass over the membership table on the device and copies back only the counts.
 *
 * The census describes the state at rest between ticks: exactly what swim_read_row of every counted observer returns
 * at the same moment. It writes nothing the simulation reads: a run with census calls interleaved is bit-identical to
 * a run without them (SEMANTICS.md §8).
 *
 * Counted observers: with observers == NULL every running member, that is every member started and not stopped at the
 * current tick (a dormant member is not running until its swim_join, a killed member not from the swim_kill call on, a
 * leaver not once it has stopped). An explicit mask is taken literally: a crashed member's frozen row is counted if the
 * caller asks for it.
 *
 * Convergence on subject s among the counted observers is  by_subject[4*s] == 0 && key_min[s] == key_max[s] :
 * every counted observer holds a record of s, and they all hold the same (incarnation, status).
 *
 * Handles: a shard from swim_create_sharded counts only the observers it owns (of the mask or of the running members),
 * and the shards' results combine to the cluster's: by_subject, records, n_observers and bytes_read add, key_min and
 * key_max combine by min and max, by_observer rows are disjoint (the contract of swim_emulator_counters). A handle
 * with n_gpus > 1 does that combination itself. A slot-sharded RUMOR group holds the views replicated and reports one
 * shard's. With implicit views (SWIM_FLAG_IMPLICIT_VIEWS) every row is the PRECONVERGED row: the answer is filled in
 * closed form, path SWIM_CENSUS_PATH_IMPLICIT, bytes_read 0, no kernel launch.
 */
#ifndef SWIMHIP_CENSUS_H
#define SWIMHIP_CENSUS_H

#include <stddef.h>
#include <stdint.h>

#include "swimhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWIM_CENSUS_PATH_IMPLICIT 0u /* implicit views: closed form, nothing read */
#define SWIM_CENSUS_PATH_KEY8     1u /* streamed the 8-bit shadow plane, u32 keys only where a byte is the escape 0xFF */
#define SWIM_CENSUS_PATH_KEY32    2u /* streamed the u32 key plane (no shadow plane on this handle) */

/* the kernel's tile (one workgroup): SWIM_CENSUS_TILE_ROWS observers x SWIM_CENSUS_TILE_COLS subjects; per-subject
 * partial counts are summed over a tile in registers and added to the output once per tile */
#define SWIM_CENSUS_TILE_ROWS 128u
#define SWIM_CENSUS_TILE_COLS 4096u

typedef struct swim_census {
  /* in */
  const uint8_t* observers; /* n_members bytes, non-zero = count this observer's row; NULL = every running member */
  /* out, each may be NULL (not computed, not copied back) */
  uint32_t* by_subject;  /* [4 * n_members]: by_subject[4*s + st] = counted observers whose row holds subject s with
                            status st (SWIM_ST_ABSENT / ALIVE / SUSPECT, 3 = DEAD: only a leaver's own record) */
  uint32_t* by_observer; /* [4 * n_members]: by_observer[4*o + st] = subjects with status st in o's row; zeros for an
                            observer that was not counted */
  uint32_t* key_min;     /* [n_members]: smallest and largest key (incarnation << 2 | status) among the counted      */
  uint32_t* key_max;     /*   observers that hold subject s; nobody holds it: key_min = 0xFFFFFFFF, key_max = 0      */
  /* out, always */
  uint64_t tick;         /* the tick the census describes (swim_current_tick) */
  uint64_t n_observers;  /* rows counted */
  uint64_t records[4];   /* records[st] = sum of by_observer[4*o + st] over the counted observers */
  uint64_t bytes_read;   /* key bytes the kernel was asked to load: rows counted x row bytes of the plane used (n_members
                            bytes on KEY8, 4 n_members on KEY32) plus 4 B per escaped subject; the algorithmic figure, as
                            swim_counters.diff_key_bytes is for the SYNC diff */
  uint32_t path;         /* SWIM_CENSUS_PATH_*: also tells whether this handle keeps the 8-bit shadow plane */
  uint32_t reserved[3];
} swim_census;

/* SWIM_EINVAL: null handle or null struct. All four output pointers NULL is valid: the totals only. Synchronises the
 * handle's stream before and after; reports a pending device error like the other readbacks. */
int swim_view_census(swim_handle* h, swim_census* c);

#ifdef __cplusplus
}
#endif
#endif
