/*
 * swimhip_debug.h — test surface of libswimhip (not part of the simulation API; the CPU oracle has no such paths).
 *
 * The engine keeps its hot per-tick state in fixed-capacity fast structures and falls back to an exact slow path
 * when one is full. Those fallbacks must give the same bits as the fast path, so tests force them:
 * the environment variable SWIM_CAPS, read by swim_create, lowers the capacities, e.g.
 *   SWIM_CAPS="trk=1,ulog=2,creq=1,cwmax=1,cev=1,mq=1,sort=2"
 *   trk    subjects tracked per receiver and tick in a sorted list for later SYNC payloads (more: the written-subject
 *          bitmap is walked in subject order),
 *          MembershipProtocolImpl.syncMembership (:456-467) with several payloads in one tick
 *   ulog   row writes logged after a SYNC send of the same tick (more: the lane copies its open snapshots),
 *          prepareSyncDataMsg (:446-454) snapshot semantics
 *   creq   copy-on-write snapshots open per member and tick (more: the lane copies them)
 *   cwmax  deferred snapshots per k_member_tick block (more: the lane copies the row)
 *   cev    cached contact events per (sender, target) pair (more: k_gossip_send_slow scans both round logs),
 *          GossipProtocolImpl.selectGossipsToSend isInfected (:239-250)
 *   mq     inbound SYNC messages of one tick sorted in registers (more: selection by list walks), onMessage (:320-331)
 *   sort   first receipts of one member and tick sorted in LDS at once (more: sorted runs merged), P4 order
 *   rx     contact pairs per tick whose replay is limited to the gossips received before the contact (more: the
 *          whole window is replayed), GossipProtocolImpl isInfected (:247)
 *   xinl   bytes per peer of the RCCL inline all-to-all of a sharded tick (more: a send/recv group; speculative
 *          sharded batches halt on the overflow flag), every rank the same value
 *   rp     replay / slow-path gossip sends per tick (grow_caps enlarges the lists; SWIM_DELIV_CAP sets the routed
 *          receipts per tick the same way)
 * With SWIM_CAPS (or SWIM_FALLBACKS=1) set, the handle counts how often each fallback fired.
 */
#ifndef SWIMHIP_DEBUG_H
#define SWIMHIP_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#include "swimhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* indices into swim_debug_fallbacks' output */
#define SWIM_FB_TRK_WALK 0u    /* later SYNC payloads merged with the written-subject bitmap (trk) */
#define SWIM_FB_ULOG 1u        /* snapshot copies forced by a full undo log (ulog) */
#define SWIM_FB_CREQ 2u        /* snapshot copies forced by too many open snapshots (creq) */
#define SWIM_FB_CWMAX 3u       /* lane row copies, block list full (cwmax) */
#define SWIM_FB_CEV_SLOW 4u    /* gossip sends replayed from a full log scan (cev) */
#define SWIM_FB_REPLAY 5u      /* gossip sends replayed from the contact cache (pairs with a logged contact) */
#define SWIM_FB_MQ 6u          /* receivers with more than mq inbound SYNC messages in one tick */
#define SWIM_FB_SORT_MERGE 7u  /* receipt segments sorted as runs and merged (sort) */
#define SWIM_FB_RX_ALL 8u      /* contact pairs that replayed their whole window (rx: rows of window gossips received
                                  before the contact, per tick) */
#define SWIM_FB_COUNT 9u

/* counts of the fallbacks fired since create, n <= 16 entries (summed over shards); SWIM_EUNSUPPORTED when the
 * handle was created without SWIM_CAPS / SWIM_FALLBACKS */
int swim_debug_fallbacks(swim_handle* h, uint64_t* out, size_t n);

/* the current sizes of the structures that grow between ticks (api.hip grow_caps), n <= 8 entries:
 * gossip slots per shard, receipt-ring entries per member, routed receipts per tick, replay / slow-path sends per
 * tick, incarnation-history entries, and how many growth steps ran. One GPU (a sharded handle: SWIM_EUNSUPPORTED). */
#define SWIM_CAP_SLOTS 0u
#define SWIM_CAP_RING 1u
#define SWIM_CAP_RECEIPTS 2u
#define SWIM_CAP_REPLAY 3u
#define SWIM_CAP_HISTORY 4u
#define SWIM_CAP_GROWTHS 5u
int swim_debug_caps(swim_handle* h, uint64_t* out, size_t n);

/* the holder bookkeeping of members [first, first + n), out[5 * i + j] for member first + i: j = 0 its gossip count
 * (GossipProtocolImpl.gossips.size(), what doSpreadGossip's early return reads, :141-146), 1 / 2 the receipt-ring
 * positions of its first held entry and of the ring end (absolute: every creation and first receipt appends one entry,
 * every sweep advances the first), 3 the popcount of its held-bit row, 4 first receipts of the last tick whose GOSSIP
 * events the next P4 folds (RUMOR mode without recorded events; 0 otherwise). One GPU or one shard of a slot-sharded
 * RUMOR cluster (a row-sharded or multi-device handle: SWIM_EUNSUPPORTED). */
int swim_debug_holders(swim_handle* h, uint32_t first, uint32_t n, uint32_t* out);

/* sets member m's own record in its own table to incarnation inc, status unchanged, between steps (one GPU): the
 * boundary test of the 30-bit incarnation field of the key plane (SEMANTICS.md §8). inc >= 2^30: SWIM_ECAPACITY.
 * The write bypasses the row's copy-on-write and write-log bookkeeping, so it is refused (SWIM_EINVAL) while a SYNC /
 * SYNC_ACK that m sent in the last tick still carries m's live row as its payload. */
int swim_debug_set_incarnation(swim_handle* h, uint32_t m, uint32_t inc);

/* One GPU, stored tables: the SYNC diff skips the 2048-subject chunks of a live-row payload that neither the sender's
 * nor the receiver's row ever changed against the baseline row. SWIM_NO_DIRTY=1, read by swim_create,
 * keeps the rows' dirty-chunk masks up to date but never consults them: every chunk is streamed (the reference path
 * of the equality tests, and A/B timing on one build).
 * With the masks consulted and the 8-bit key plane, the lister also decides a pinned live-row payload (one of several
 * payloads of its receiver in a tick) when every row involved is clean, and speculative batches queue no k_sync_diff
 * on untimed ticks. SWIM_NO_ELIDE=1, read by swim_create, keeps a diff launch on every tick.
 * Once a whole such batch has listed nothing and written nothing, no delay is set and every row is clean, the untimed
 * ticks queue no lister either and the receivers count their messages in its place ("Round 10").
 * SWIM_NO_LISTERFREE=1, read by swim_create, keeps the lister on every tick.
 * swim_debug_diff_dirty: n <= 10 entries since create; entry 4 (n > 4) costs a pass over the key plane. */
#define SWIM_DD_SKIPPED 0u      /* narrow chunks decided from the masks, not streamed */
#define SWIM_DD_STREAMED 1u     /* narrow chunks streamed */
#define SWIM_DD_MSG_SKIPPED 2u  /* payloads decided without streaming any chunk */
#define SWIM_DD_REBASES 3u      /* baseline chunks replaced (k_rebase) */
#define SWIM_DD_DIRTY_ROWS 4u   /* (row, chunk) pairs marked dirty now */
#define SWIM_DD_PIN_DECIDED 5u  /* pinned live-row payloads decided from the masks (among MSG_SKIPPED) */
#define SWIM_DD_DIFF_ELIDED 6u  /* ticks run without a k_sync_diff launch (speculative batches, SWIM_NO_ELIDE: 0) */
#define SWIM_DD_DIFF_HALTS 7u   /* batches stopped because a lister listed work for a diff that was not queued */
#define SWIM_DD_LF_TICKS 8u     /* ticks run without a lister launch (lister-free batches, SWIM_NO_LISTERFREE: 0) */
#define SWIM_DD_LF_STOPS 9u     /* lister-free batches stopped because a member kernel wrote */
int swim_debug_diff_dirty(swim_handle* h, uint64_t* out, size_t n);

/* One GPU, FULL mode, stored tables: the member kernel runs the steady state's member-ticks (a ping, its hop, its ack,
 * one or two SYNC / SYNC_ACK receipts with nothing to merge, the periodic SYNC send) on a light path that loads what it
 * needs in rounds of independent loads, decides in registers, and commits only then; anything else falls back, before
 * any store, to the general body, which is also its reference ("Round 12"). SWIM_NO_LIGHT=1 (any value
 * but 0), read by swim_create, runs every member-tick through the general body. That is the tests' reference path, not
 * the kernel as it was before the path existed: the launch keeps the path's LDS lists, so timing against that kernel
 * needs both builds. The path is also off while link delays or per-link settings exist.
 * swim_debug_light: n <= 13 entries since create. SWIM_LT_GENERAL is counted while the path is on, and with it off
 * only on a handle that counts its fallbacks (SWIM_CAPS / SWIM_FALLBACKS at create), so that a handle without the path
 * pays nothing for it. A multi-device or sharded handle: SWIM_EUNSUPPORTED. */
#define SWIM_LT_TICKS 0u          /* member-ticks finished by the light path */
#define SWIM_LT_FD 1u             /* of them with a ping, a ping hop or an ack arrival */
#define SWIM_LT_P1 2u             /* of them with a SYNC / SYNC_ACK receipt */
#define SWIM_LT_SYNC 3u           /* of them with the periodic SYNC send */
#define SWIM_LT_GENERAL 4u        /* member-ticks run by the general body (the fallbacks among them) */
#define SWIM_LT_FB_RESHUFFLE 5u   /* fallbacks by reason: the ping cursor reached the end of the list */
#define SWIM_LT_FB_SEND 6u        /* the ping's send failed (a ping-req follows) */
#define SWIM_LT_FB_PAYLOADS 7u    /* three inbound SYNC / SYNC_ACK payloads or more (two under SWIM_CAPS mq=1) */
#define SWIM_LT_FB_CAND 8u        /* a payload with records to merge */
#define SWIM_LT_FB_BUSY 9u        /* pending fetches, several paths or subscriptions, a ping-req's */
#define SWIM_LT_FB_STATUS 10u     /* an ack for a target the row holds as neither ALIVE nor ABSENT (a SYNC follows) */
#define SWIM_LT_FB_OTHER 11u
#define SWIM_LT_ON 12u            /* 1: the next member kernel takes the light path, 0: it does not */
int swim_debug_light(swim_handle* h, uint64_t* out, size_t n);

/* The light path while nobody is dead ("Round 13"). The engine keeps one device word, first_dead, that
 * is at most every member's dead tick (a kill, a completed leave and dormant members lower it; nothing raises it). A
 * member kernel launched for a tick below it skips the light path's dead-member lookups (the ping target's, a hop
 * target's, the SYNC and SYNC_ACK destinations'): every one of them would answer "alive".
 * swim_debug_light_sure: n <= 3 entries; the counter since create, counted under swim_debug_light's conditions;
 * entry 2 (n > 2) costs a readback of every member's dead tick. A multi-device or sharded handle: SWIM_EUNSUPPORTED. */
#define SWIM_LS_SKIPPED 0u     /* member-ticks finished by the light path with the dead lookups skipped */
#define SWIM_LS_FIRST_DEAD 1u  /* the word now (0xFFFFFFFF: nobody ever died, left or was dormant) */
#define SWIM_LS_MIN_DEAD 2u    /* the minimum over the members' dead ticks now: never below the word */
int swim_debug_light_sure(swim_handle* h, uint64_t* out, size_t n);

/* the masks' invariant, tested directly: the number of (row, chunk) pairs marked clean whose keys differ from the
 * baseline's chunk, which on one GPU is what the first row marked clean in that chunk holds: all clean rows must agree
 * (0 in a correct engine). One pass over the key plane. */
int swim_debug_dirty_check(swim_handle* h, uint64_t* violations);

/* Known-answer surface of the device primitives the per-tick kernels are made of (no handle): the engine's own scan,
 * segmented sort, receipt routing, ring move and inline device helpers run on caller data, in the block shape the
 * engine launches them in (256 threads), so a test can compare each with a plain reference at the sizes and lane masks
 * where such code goes wrong. Every buffer is allocated by the call and freed before it returns. Sizes, offsets and
 * indices are checked on the host first: anything the layouts below do not allow is SWIM_EINVAL before any launch.
 * `in` and `out` are 8-byte aligned arrays of 32-bit words (u64 = two words, low first) in the order listed; `out` is
 * also read where marked in/out (the caller's sentinels or preset bits). T = 256 * blocks threads.
 *
 * SCAN       params n (1..2^20)                        in  v[n]
 *            launch_scan                               out x[n + 64] in/out (words at and past n are not written)
 * SEG_SORT   params total, nmem, nlist, run, fb        in  key u64[total], val[total], off[nmem], cnt[nmem], sg[nlist]
 *            k_seg_sort, 1024 blocks; run a power of   out merges u64 (FB_SORT_MERGE; fb = 0: a null counter), key
 *            two in 2..4096; off + cnt <= total            u64[total], val[total]
 * ROUTING    params N, RCAP, rc_n, SLOTS, sort_cap, fb in  rc_raw u64[min(rc_n, RCAP)] (member << 32 | slot), slot_gid
 *            launch_receipt_routing on a zeroed Dev        u64[SLOTS]
 *                                                      out rc_key u64[RCAP] in/out, merges u64, rc_slot[RCAP] in/out,
 *                                                          rc_off[N], rc_cnt[N], sg_list[N] in/out, nsg, 0
 * WAVE       params sub, blocks (1..64)                in  a[3][T]
 *            sub APPEND: lanes with a[0] != 0 call     out r[3][T] in/out, ctr[4] in/out (ctr[0] is the counter)
 *            wave_append; WAVE_RESERVE / BLOCK_RESERVE: every thread reserves a[0] (block: a[0], a[1], a[2] in three
 *            calls on one LDS scratch); SUM32 / MIN32: wave_sum / wave_min of a[0]; SUM64: of a[0] | a[1] << 32 into
 *            r[0], r[1]
 * DIRTY      params wave, blocks (1..64), MW (1..3)    in  a[3][T]
 *            wave = 0: thread t owns mask row t and    out mask u64[rows][MW] in/out (rows = T, or T / 64)
 *            calls dirty_mark for each a[j][t] != 0xFFFFFFFF; wave = 1: wave w owns row w and every lane calls
 *            dirty_mark_wave(wr = a[1] != 0, subject a[0]); subjects < MW * 64 * 2048
 * ARITH      params sub, n (1..2^20), ...              one thread per case
 *            DIV_GT  params gossip_t (>= 1)            in  x[n]                        out q[n], gt_mul
 *            S16     s16_tick                          in  (entry, ref)[n]             out tick[n]
 *            RG      rg_entry then rg_period           in  (slot, infp, P)[n]          out (period lo, hi, slot bits)[n]
 *            KEY8                                      in  key[n]                      out shadow[n]
 *            DELAY   params di (< 16), len (<= 256)    in  thr[len], x[n]              out ticks[n]
 *            EPOCH   epoch_at                          in  ep_from[8], k[n]            out epoch[n] (0xFFFFFFFF: none)
 *            PAYKEY  params MW, NS, ri, RXCAP, off     in  mask u64[MW], base_row[NS], shipped[popcount(mask)][2048],
 *                    payload_key_at of payload             s[n] (each < NS <= MW * 64 * 2048)
 *                    PAY_RX | ri, shipped chunks at    out key[n]
 *                    byte offset off (a multiple of 4) of the receive buffer
 * FEISTEL    params n (1..2^20), k0, k1, k2, k3        in  -
 *            make_perm, feistel over [0, n)            out device[n], host[n] (the same functions compiled for the host)
 * RING_MOVE  params N, B, B2 (powers of two, B <= B2)  in  rg[N][B], rhead[N], rtail[N] (rtail - rhead <= B)
 *            launch_ring_move                          out rg2[N][B2] in/out
 *
 * SYNC_DIFF  k_sync_diff and its lister k_ack_resolve (sync_diff.hip) on a Dev that holds only what the two kernels read,
 *            queued through launch_diff_listed (the diff alone) or launch_diff (the lister, then the diff) as a step
 *            queues them, on the messages of one buffer (that of tick k - 1). The sizes follow from N by the expressions
 *            swim_create uses: NS = N rounded up to 8, NS8 to 16, NCHUNK = NS / 2048 and NMETA = NS / 1024 rounded up,
 *            MW = NCHUNK / 64 rounded up, nit = NCHUNK / 4 rounded up (narrow items per payload).
 *            params (15): N subjects (1 .. 3 * 64 * 2048); R rows (1..64: members lo .. lo + R - 1); flags (SWIM_PRIM_SD_*);
 *              nmsg; MSGCAP (nmsg <= MSGCAP <= 4096); ARENA_ROWS A (<= 64); POOLCAP (<= 2^22); k (>= 1: the tick, buffer
 *              (k - 1) & 1); grid (k_sync_diff's blocks, <= 4096; 0: the engine's own); sentinel; nnar, nwide (the lists'
 *              lengths, with SD_LISTS); lo, nrx (received payloads <= 64; with SD_SHARDED); ls (launch_diff's: 1 = LS_SPEC,
 *              2 = LS_NODIFF; with SD_LISTER)
 *            flags: SD_K8 the rows have the 8-bit plane (derived here with key8; narrow entries need it);
 *              SD_LISTS (mode A) ackres is on and k_sync_diff streams the caller's two lists, else every message wide;
 *              SD_SHARDED (mode A) W = 2: k_sync_diff<true>, a narrow entry per message, payloads PAY_RX | ri;
 *              SD_LISTER (mode B, one GPU) launch_diff(k, ls): k_ack_resolve builds the lists; SD_DIRTY with it: the
 *              lister consults the rows' dirty masks (with SD_K8 too: diff_elidable, the inbound lists are walked)
 *            in  dirty u64[R][3] (MS::dirty); SD_SHARDED: rx_mask u64[nrx][MW], rx_off u64[nrx] (byte offsets into the
 *                receive buffer, multiples of 16); rowk[R][NS]; arena[A][NS]; msgs[nmsg][6] = src, dst, kind, payload,
 *                pin, tln (ncand = 0); SD_LISTS: narrow[nnar][4], wide[nwide][4] (message, sender, receiver, place:
 *                desc_pay; one GPU narrow: item << 4 | chunk bits); SD_LISTER: tl_tick[2][R], tl_n[2][R], tlog[2][R][16],
 *                m_head[R], m_next[nmsg]; SD_SHARDED: base_row[NS], receive buffer [chunks][2048]
 *            out pool u64[POOLCAP + 64] (every word preset to sentinel | sentinel << 32; the last 64 are guard words);
 *                u64[12] = C_DIFFMSG, C_DIFFMSG_ALL, C_DIFFWIDE, C_DIFFWIDE_ALL, C_ACKRES, C_ACKRES_ALL, C_DSTREAM,
 *                C_DSUBJ, C_DSUBJ_ALL, C_DMSGSKIP, pin-decided, 0; cstat u64[NCHUNK][3] (0 when SD_SHARDED);
 *                chunk_meta[nmsg][NMETA][2] (preset to sentinel); (kind, ncand, pin)[nmsg]; arena[A][NS];
 *                narrow list [ncap][4] (ncap = MSGCAP * nit, SD_SHARDED: MSGCAP) and wide list [MSGCAP][4] (preset to
 *                sentinel); pool_used, err, narrow length, wide length, halt[3], hflag[HF_STREAMED]
 *            EINVAL before any launch: a src / dst outside the rows (a PAY_RX payload's src: outside N), a payload or pin
 *            that is no arena row (or PAY_RX | ri with ri >= nrx), a list entry whose message, rows, place, item or chunk
 *            bits do not exist, a log subject >= N, an m_head / m_next link >= nmsg or a list that does not end, chunk-mask
 *            bits past NCHUNK, an rx_off that is no multiple of 16 or whose popcount(mask) chunks pass the receive buffer,
 *            non-zero padding keys between N and NS, k = 0, flags that do not go together
 *
 * The row-shard exchange codec (shard.hip), each kernel in the grid the engine launches it in, on a Dev that
 * holds only what it reads. The in/out buffers are preset by the caller (a sentinel), so a test also sees what was not
 * written. Capacity overflows (E_XCAP, E_MSGS) are the kernels' own error paths and reach them; everything else the
 * layouts do not allow is SWIM_EINVAL before any launch. At most 32 params.
 *
 * XPACK      k_pack_all at (16, W) on one rank's tick output; NS, NCHUNK, MW follow from N as for SYNC_DIFF.
 *            params (22): N; W (2..8); rank; R local rows (1..64: members shard_lo(N, W, rank) .. + R - 1, inside the
 *              shard); b (tick parity); flags (SWIM_PRIM_XP_*); nmsg; MSGCAP (nmsg <= MSGCAP <= 4096); ARENA_ROWS A (<= 64);
 *              NSCAP, RRCAP (1..1024); RQCAP, CHCAP (<= 2^20); XA_PEER (a multiple of 16, 32 .. 2^26: chunks are stored
 *              16 B at a time); XI (a multiple of 8, 64 .. 2^20); gossip slots in use (> 0: XFLAG_GOSSIP); xn[0], xn[1] (the
 *              tick's slot and round record counts, which may pass NSCAP / RRCAP); nsr, nrr (records supplied:
 *              min(xn[0], NSCAP) <= nsr <= NSCAP, the same for rounds); xn[4] (messages already queued in mtmp); sentinel
 *              (the value of the xn words the kernel does not use)
 *            flags: XP_ACKRES the log prefixes are copied; XP_INLINE the inline blocks are written (Dev::inl); XP_SPEC a
 *              speculative launch, XP_HALTED with it: the halt word is already raised; XP_TLOG the input has the log;
 *              XP_INLINE_OUT k_inline_out at (W) then writes its blocks of the same regions and count words into xi_out
 *              (XA_PEER >= XI - 8)
 *            in  rdirty u64[R][MW]; arena_dirty u64[A][MW]; rowk[R][NS]; arena[A][NS]; msgs[nmsg][13] (whole SyncMsg
 *                records); XP_TLOG: tlog[R][16] of parity b; ns_rec[nsr][8]; rr_rec[nrr][12]
 *            out (bytes, all in/out but the last three) xa_send[W][XA_PEER]; xa_scnt u64[W]; xi_send[W][XI]; xi_out[W][XI];
 *                mtmp[MSGCAP][13]; mlog[MSGCAP][16]; xn[8]; err; halt[0]
 *            EINVAL: a src outside the R rows, a dst >= N, a payload that is neither 0xFFFFFFFF nor an arena row, mask
 *            bits past NCHUNK, a KF_RES message with 1 <= tln <= 16 under XP_ACKRES without XP_TLOG, counts or sizes out
 *            of the ranges above, XP_HALTED without XP_SPEC
 * PACK_B     k_pack_b at (64, W). params (5): W, rank, DCAP (1..2^20), *xd_n, XB_PEER (a multiple of 8, 16 .. 2^24)
 *            in  xd u64[min(*xd_n, DCAP)]
 *            out xb_send[W][XB_PEER] in/out; xb_scnt u64[W] in/out; err; 0
 * INLINE_IN  k_inline_in at (W). params (4): W, XI, cap (a multiple of 8, XI - 8 .. 2^24: bytes per receive region), flags
 *              (1: a speculative launch, which reads the halt word; 3: that word is raised)
 *            in  irecv[W][XI] (count word, then the block); scnt u64[W]
 *            out recv[W][cap] in/out; rcnt u64[W] in/out; host u64[2 W] in/out
 * XUNPACK    k_unpack_a at (32, W), with msgs_commit and (XU_END) tick_end, on caller-built receive regions; with
 *            XU_INLINE_IN k_inline_in at (W) first expands inline blocks into regions preset to the sentinel's low byte.
 *            params (18): N; W (2..8); rank; k (the tick, < 2^31: the inbound list of buffer k & 1); flags (SWIM_PRIM_XU_*);
 *              MSGCAP (1..4096); RXCAP (<= 4096); ARENA_ROWS (<= 64); XA_PEER (a multiple of 16, max(32, XI - 8) .. 2^26); XI;
 *              nloc (local messages already in mtmp: xn[4]); SLOTS (a multiple of 64, 64..4096), BCAP (a power of two <= 64),
 *              LOGW (1..8), F (1..8), EXPB, gossip_t (>= 1) (all six with XU_GOSSIP only, N <= 65536 then); sentinel
 *            flags: XU_END the launch closes the tick; XU_SPEC a speculative launch (the gate is evaluated), XU_HALTED with
 *              it: the halt word is already raised; XU_ACKRES log prefixes are copied; XU_GOSSIP the gossip plane's arrays
 *              exist (without it no region may hold a slot or round record)
 *            in  regions [W][XA_PEER], or with XU_INLINE_IN blocks [W][XI] (count word first); rcnt u64[W] (ignored with
 *                XU_INLINE_IN); scnt u64[W] (this rank's sent count words); mtmp[nloc][13]; XU_GOSSIP: firstGossip[N],
 *                rhead[N], rtail[N], log_pos[N], log_spread[N][LOGW]
 *            out (bytes; in/out unless said) msgs[MSGCAP][13] of buffer k & 1; m_head[N] of that buffer (starts empty: every
 *                word 0xFFFFFFFF); m_next[MSGCAP]; rx_mask u64[RXCAP][MW]; rx_off u64[RXCAP]; mlog[MSGCAP][16]; u32[18] =
 *                nmsg[2], arena_used[2], xn[8], err, halt[0], pool_used, rc_n, ndl, ndlw (start: nmsg, the other buffer's
 *                arena_used, xn[0..3], xn[7] and the last four at the sentinel; this buffer's arena_used, xn[5], xn[6], err 0;
 *                xn[4] = nloc); xa_scnt u64[W] (starts as scnt); xb_scnt u64[W]; xdone[2 W]; xa_rcnt u64[W]; host u64[2 W];
 *                XU_GOSSIP: slot_gid u64[SLOTS]; slot_key u64[SLOTS]; slot_subj, slot_ctick, slot_exp, slot_used [SLOTS] each;
 *                GU, DM u64[SLOTS / 64] each (start 0); S u16[N][SLOTS]; HB u64[N][SLOTS / 64] (starts 0); rg[N][BCAP];
 *                [8][N] = rtail (starts as given), held (starts 0), tround, tcnt, tspread, tperiod, spchg, log_pos (starts as
 *                given); T[N][F]; [3][N][LOGW] = log_tick, log_spread (starts as given), log_cnt; log_tg[N][LOGW][F]
 *            EINVAL: unless a speculative launch is certain to stop at its halt word or gate, every region of a peer with a
 *            count >= 32 is checked against its byte count and XA_PEER: records, entries and data_off (a multiple of 16)
 *            inside it, base + popcount(mask) <= nchunk chunks inside it, mask bits past NCHUNK, src / dst / origins / round
 *            members / targets < N, slot ids < SLOTS, cnt <= F; an inline block whose region is longer than it (the engine
 *            fetches the rest first) unless the gate stops the launch; an mtmp entry with src or dst >= N; rtail - rhead >
 *            BCAP; sizes out of the ranges above
 *
 * The gossip data plane's per-tick kernels (gossip_*.hip): the engine's own launchers, unchanged and in their
 * own grids, for one tick k on a caller-built holder state, on a zeroed Dev that holds only what their kernels read and a
 * device copy of it (Dev::self). Scope: one GPU (W = XW = 1, lo = 0, hi = N); no link delays (dly_on = 0: the k_gossip_due*
 * kernels are not launched); exp = 0, dbg_send = null, fastp4 = 0; one settings epoch (ep_from[0] = 0, the others NEVER) and
 * no per-link setting (link_n = 0). Every array of `in` and `out` starts 8-byte aligned (its bytes are rounded up to a
 * multiple of 8); `out` is in/out throughout: the caller presets every word, so what a kernel did not write is seen.
 *
 * GOSSIP     launch_gossip_send, then with GS_APPLY launch_gossip_apply. QW = SLOTS / 64, NS = N rounded up to 8.
 *            params (27): N (1..4096); F (1..8); SLOTS (a multiple of 64, 64..2^18, N * SLOTS <= 2^21); BCAP (a power of two
 *              <= 16384, N * BCAP <= 2^22); LOGW (a power of two <= 256); lat (<= 2^16); gossip_t (1..2^16); EXPB (<= 2^20); k
 *              (the tick, 1 .. 2^30 - 1); seed_lo, seed_hi; rr_atomic; cev_cap (<= 6, the cache's CEV); CRCAP (1..4096, CRCAP *
 *              QW <= 2^22); RPCAP, SLOWCAP (1..2^20); RCAP (1..2^22); HCAP (a power of two <= 2^16); sort_cap (a power of two in
 *              2..4096); rank (< 64) and SPR (>= 1: k_gossip_free returns the slots g with g / SPR == rank); flags (SWIM_PRIM_GS_*);
 *              cw, cb, cx (the LDS row chunks in 8-byte words of k_round_apply_w (its row limit), k_round_apply_b and k_rx_build;
 *              0: the engine's own min(1024 | 4096 | 8192, QW); at most those, the 64 KB of LDS a workgroup has); ep_loss
 *              (<= 100), ep_part (0 / 1) of the one epoch
 *            flags: GS_APPLY also launch_gossip_apply (rowk is read); GS_EM the emulator counters exist (Dev::em: the exact
 *              per-send path of k_gossip_send and deliver_one); GS_FB the fallback counters exist (Dev::fb)
 *            in  slot_gid u64[SLOTS]; slot_key u64[SLOTS]; slot_subj, slot_ctick [SLOTS] each; firstGossip, tround, tcnt,
 *                tspread, tperiod, spchg, log_pos [N] each; T[N][F]; log_tick, log_spread, log_cnt [N][LOGW] each;
 *                log_tg[N][LOGW][F]; ep_group[N]; leaving[N]; with GS_APPLY rowk[N][NS]
 *            out u64: GU, DM [QW] each; HB, WB [N][QW] each; RX[CRCAP][QW]; rp[RPCAP]; slow[SLOWCAP]; hist[HCAP][11];
 *                rc_raw[RCAP]; rc_key[RCAP]; ctr[C_G] (out only); em[2 N]; fb[16] (both unchanged without their flag);
 *                then S u16[N][SLOTS]; then u32: rg[N][BCAP]; [N] each: dead_tick, rhead, rtail, rwin, rseen, held, rsend,
 *                rwnew, rt0, tin_cnt as launch_gossip_send left it (out only: k_gossip_apply clears it), tin_cnt, tin_fill (out
 *                only: both start a tick at 0), tin_off, dead_rx, rc_ndrop, rwl, tlist, ap_list, rc_off, rc_cnt (out only),
 *                sg_list; [SLOTS] each: slot_exp, slot_used, fexp, free_list; agroup[QW]; [N][F] each: tin, tcontact, cin,
 *                crow; cev[N][F][22]; rxl[CRCAP][3]; rc_slot[RCAP]; u32[16] = nagroup[2], nrwl, ntl, nrx, rp_n, slow_n, rc_n (must
 *                start at 0), nap, nsg, nfexp, free_top, hist_n, ncfl, xd_n, 0; err[8] (out only)
 *            The kernels' own capacity paths are no validation and reach the kernels: E_RING (ring writes are masked),
 *            E_CONTACTS (rp / slow writes are guarded by RPCAP / SLOWCAP), E_RECEIPTS (rc_raw writes by RCAP), E_SLIFE.
 *            EINVAL before any launch: a T entry below tcnt or a log target below log_cnt that is >= N; tcnt or log_cnt > F; a
 *            ring entry of [rhead, rtail) whose slot is >= SLOTS; rtail - rhead > BCAP; rwin or rseen outside [rhead, rtail]
 *            (positions are absolute and wrap: compared by differences); a slot_subj that is neither USER_SUBJ nor < N;
 *            free_top < 0 or free_top + popcount(GU) > SLOTS (the free list holds SLOTS entries); rc_n != 0; in / out of the
 *            wrong length (an ep_group of the wrong length is one); sizes, capacities or chunk overrides out of the ranges
 *            above; k = 0. (SLOTS is a multiple of 64, so GU / DM / HB / WB have no bit past SLOTS.) */
#define SWIM_PRIM_SCAN 0u
#define SWIM_PRIM_SEG_SORT 1u
#define SWIM_PRIM_ROUTING 2u
#define SWIM_PRIM_WAVE 3u
#define SWIM_PRIM_DIRTY 4u
#define SWIM_PRIM_ARITH 5u
#define SWIM_PRIM_FEISTEL 6u
#define SWIM_PRIM_RING_MOVE 7u
#define SWIM_PRIM_SYNC_DIFF 8u
#define SWIM_PRIM_XPACK 9u
#define SWIM_PRIM_PACK_B 10u
#define SWIM_PRIM_INLINE_IN 11u
#define SWIM_PRIM_XUNPACK 12u
#define SWIM_PRIM_GOSSIP 13u
#define SWIM_PRIM_GS_APPLY 1u
#define SWIM_PRIM_GS_EM 2u
#define SWIM_PRIM_GS_FB 4u
#define SWIM_PRIM_XP_ACKRES 1u
#define SWIM_PRIM_XP_INLINE 2u
#define SWIM_PRIM_XP_SPEC 4u
#define SWIM_PRIM_XP_HALTED 8u
#define SWIM_PRIM_XP_TLOG 16u
#define SWIM_PRIM_XP_INLINE_OUT 32u
#define SWIM_PRIM_XU_END 1u
#define SWIM_PRIM_XU_SPEC 2u
#define SWIM_PRIM_XU_HALTED 4u
#define SWIM_PRIM_XU_ACKRES 8u
#define SWIM_PRIM_XU_INLINE_IN 16u
#define SWIM_PRIM_XU_GOSSIP 32u
#define SWIM_PRIM_SD_K8 1u
#define SWIM_PRIM_SD_LISTER 2u
#define SWIM_PRIM_SD_LISTS 4u
#define SWIM_PRIM_SD_SHARDED 8u
#define SWIM_PRIM_SD_DIRTY 16u
#define SWIM_PRIM_WAVE_APPEND 0u
#define SWIM_PRIM_WAVE_RESERVE 1u
#define SWIM_PRIM_WAVE_BLOCK_RESERVE 2u
#define SWIM_PRIM_WAVE_SUM32 3u
#define SWIM_PRIM_WAVE_MIN32 4u
#define SWIM_PRIM_WAVE_SUM64 5u
#define SWIM_PRIM_ARITH_DIV_GT 0u
#define SWIM_PRIM_ARITH_S16 1u
#define SWIM_PRIM_ARITH_RG 2u
#define SWIM_PRIM_ARITH_KEY8 3u
#define SWIM_PRIM_ARITH_DELAY 4u
#define SWIM_PRIM_ARITH_EPOCH 5u
#define SWIM_PRIM_ARITH_PAYKEY 6u
int swim_debug_prim_eval(uint32_t op, const uint32_t* params, size_t n_params, const void* in, size_t in_bytes,
                         void* out, size_t out_bytes, uint32_t device);

/* Injected gossip receipts: the receipts of the next tick's P4 (onMembershipGossip -> updateMembership,
 * MembershipProtocolImpl.java:401-408,475-541) set by the caller on a live handle, so that a test chooses the batch
 * sizes, subjects, orders and pre-states that the lane-serial fold (member.hip p4_receipts) and the wave version
 * (inbox.hip k_inbox_apply) must agree on. One GPU, FULL mode, stored tables; a multi-device, row- or slot-sharded or RUMOR
 * handle is SWIM_EINVAL. Host copies only: the kernels that run the receipts are the ones a step launches.
 *
 * swim_debug_receipts_set, between steps, installs for the handle's next tick k:
 *   recs   [n_recs][6] words, one gossip each. SWIM_DEBUG_REC_MEMBER: subject, status (1 ALIVE, 2 SUSPECT, 3 DEAD),
 *          incarnation, then the gossip id (origin member, counter). SWIM_DEBUG_REC_USER: origin, payload low word,
 *          payload high word, 0, the gossip's counter (GossipProtocolImpl user gossips: the GOSSIP event's fields).
 *   lists  groups of words: member, dropped receipts (Dev::rc_ndrop: receipts the routing found unable to change the
 *          row, counted as record compares), count, then `count` indices into recs in the order P4 takes them. Each
 *          member at most once; the same record may be listed for many members and several times for one.
 *   split  1: the member launch of tick k is the split triple (k_member_tick BODY_SPLIT, k_inbox_apply, BODY_RESUME: the
 *          launch that follows a gossip plane), 0: the single BODY_FULL launch.
 * Each record takes one gossip slot off the top of the free stack (slot_subj, slot_key, slot_gid written, slot_used left
 * 0: neither the gossip plane nor the state hash sees it; a gossip the tick creates cannot take the slot). The next
 * step of one tick runs tick k on the one-tick path (no speculative or lister-free batch); everything after the member
 * launch runs as on any tick. SWIM_EINVAL before anything is written: a subject, origin or member >= N; a status
 * outside 1..3; an unknown record kind; an index >= n_recs; a member listed twice; more receipts in all than the routed-
 * receipt capacity (swim_debug_caps SWIM_CAP_RECEIPTS); more records than free slots; a handle with a gossip slot in use,
 * a routed receipt pending, queued user gossips or an injection not yet read back. An incarnation >= 2^30 is not
 * refused: it reaches the kernels' own E_INC path (the step returns SWIM_ECAPACITY).
 *
 * swim_debug_receipts_read, after that step: out[n][SWIM_DEBUG_RD_WORDS + SWIM_DEBUG_FREC * fetch_cap] for members
 * [first, first + n): tsize, cidCnt, nfetch, fnext, timerMin, held (the member's gossip count), gCounter, evSeq, the
 * length of the member's write log of tick k (0 when it logged nothing in k; SWIM_DEBUG_TL + 1: overflowed), its
 * SWIM_DEBUG_TL entries (0 past the length), then the first min(nfetch, fetch_cap) pending metadata fetches, 8 words each:
 * correlation id, subject, incarnation, status | reason << 8 | added << 16 | stage << 24, group, deadline tick, next hop
 * tick, metadata version (0 past nfetch). fetch_cap <= swim_config.pending_fetch_cap (256 when that is 0).
 * msg_out (may be null): [2 + 3 N] = arena rows taken in tick k's message buffer, its messages, then per sender the
 * messages of that buffer whose payload is an arena row (a snapshot of the row as it was sent), then every member's
 * routed-receipt count and fill as the tick left them (Dev::rc_cnt, rc_fill: 0 once P4 or the triage took the list).
 * The first read after a set also puts the injected slots back on top of the free stack, so stepping goes on as on any
 * handle; n = 0 with msg_out null does only that. SWIM_EINVAL: no injection since create, a range past N, fetch_cap
 * past the handle's. */
#define SWIM_DEBUG_REC_MEMBER 0u
#define SWIM_DEBUG_REC_USER 1u
#define SWIM_DEBUG_TL 16u
#define SWIM_DEBUG_FREC 8u
#define SWIM_DEBUG_RD_WORDS 25u
int swim_debug_receipts_set(swim_handle* h, const uint32_t* recs, size_t n_recs, const uint32_t* lists, size_t n_words,
                            uint32_t split);
int swim_debug_receipts_read(swim_handle* h, uint32_t first, uint32_t n, uint32_t fetch_cap, uint32_t* out,
                             uint32_t* msg_out);

#ifdef __cplusplus
}
#endif
#endif
