// spec.h — the halt protocol of the speculative batches, the launch flags that carry it, the host-mapped flag block
// and the SWIM_EXP bits: everything a kernel or a host path must agree on to take part in a batch (step.hip).
//
// A speculative batch is a run of ticks queued with no host wait (one GPU: spec_batch; row shards over RCCL:
// shard_spec_batch). Device words, Dev::halt, decide which of the queued launches still do anything. A launch of
// tick k reads them at its start (all at once, system scope: halt_load; hg = halt[HALT_GOSSIP], hd = halt[HALT_DIFF],
// hw = halt[HALT_WROTE]) and returns at once by the rule of its kernel; nothing waits on the device, and the host reads the words back after
// the batch. hw takes part only in the launches of a lister-free batch (LS_LF, MT_LF; below): the other one-GPU
// batches write it (the host looks at it before it enters the mode) but never read it on the device.
//
//   kernel (launch of tick k)         predicate             returns at once when
//   k_ack_resolve (the lister)        halted_lister         hg != 0, or hd != 0 && hd != k + 1; LS_LF: or hw != 0 && hw <= k
//   k_sync_diff                       halted_diff           hg != 0 or hd != 0; LS_LF: or hw != 0 (the same thing: it is
//                                                           queued before member(k), so any hw it reads is <= k)
//   k_member_tick_t                   halted_member         hg != 0 && hg <= k, or hd != 0; MT_LF: or hw != 0 && hw <= k
//   k_sync_redeliver<false>           halted_member         (the same, without the MT_LF clause: no delay in that mode)
//   k_sync_defer<false>               halted_member         (the same)
//   k_sync_redeliver<true>            halted_before         hg != 0 && hg <= k
//   k_sync_defer<true>                halted_uncommitted    hg != 0 && hg <= k + 1
//   k_pack_all, k_unpack_a,           halted                hg != 0
//   k_inline_in
//   k_watch (a recorded sample of     halted_sample         hg != 0 && hg <= t, or hd != 0; lister-free: or hw != 0 &&
//   tick t, behind member(t - 1))                           hw <= t - 1
//
// Why the rules differ:
// * the lister and the diff of tick k are queued before member(k - 1)'s successors know whether that member kernel
//   took a gossip slot, so any gossip halt (hg = k at the latest) stops them: the host queues them again after the
//   gossip plane. The lister ignores the diff-halt of its own tick, hd == k + 1, which another block of the same
//   launch raised: its list must be complete for the diff the host then runs. The diff is only queued when its lister
//   raises no diff-halt, so either word stops it.
// * member(k) raises hg = k + 1 itself while it runs (a member that takes a slot, or tick_reset): its own blocks and
//   the one-GPU delayed-SYNC kernels of tick k, which move that tick's messages, go on; only a halt of an earlier tick
//   (hg <= k) stops them. A diff-halt of tick k or earlier means member(k) must not run before the host has run that
//   diff: returning before tick_reset keeps the lists and the pool as the lister left them.
// * a row shard never raises a diff-halt (its batches always queue the diff), and its gossip halt is raised by the
//   gate in k_unpack_a(k), after exchange A: k_sync_redeliver<true>(k) runs before the gate and stops on an earlier
//   tick's halt only; k_sync_defer<true>(k) runs after it and skips tick k itself too, because its inbound list was
//   not committed (the host's path stores that tick's delayed messages); k_pack_all, k_unpack_a and k_inline_in carry
//   no tick of their own and stop on any halt (the kernels after the gate: on this tick's, too).
//
// * a lister-free batch (one GPU, step.hip spec_batch) queues no lister on its untimed ticks: in a
//   cluster whose rows all equal the baseline and whose write logs are empty the lister's verdict is a constant
//   (ncand = 0 for every message), and the receivers count the messages as it would have (MT_NOLIST: P1 and the
//   triage's dead branch). A member kernel that does anything that verdict depends on (note_wrote: a key change or a
//   merged candidate, a copy-on-write snapshot, a delayed send, a redelivery) stores hw = its tick + 1. member(kw) itself
//   is complete and right (its own lister, had it run, ran before it); lister(kw + 1) would not be a constant any more,
//   so every launch of a later tick returns at once, member(k) before its resets, and the host goes on from
//   lister(kw + 1) with the mode off. A member that writes usually takes a gossip slot in the same launch: then
//   hg == hw and the gossip halt's path is taken (the host queues the front of kw + 1 again after the gossip plane).
//
// * a recorded watch sample of tick t (watch.hip, swimhip_watch_series.h) is a reader only: it is queued directly
//   behind member(t - 1) (row shards: behind k_unpack_a(t - 1)) and in front of the front of t, and describes the state
//   at rest at tick t, which exists once member(t - 1) and, where one is needed, the gossip plane of t - 1 have run.
//   hg <= t: member(t - 1) took a slot (hg = t; the gossip plane of t - 1 has not run) or an earlier halt kept it from
//   running; hd != 0: a lister of tick <= t - 1 stopped the batch in front of member(t - 1) (hd <= t: no lister of a later
//   tick has run yet); lister-free, hw <= t - 1: an earlier member kernel wrote and member(t - 1) returned at once, while
//   hw == t is member(t - 1) itself, which is complete. The engine has one stream: nothing runs beside the sample, so
//   the words it reads were stored by earlier launches only. The host queues a void sample again where it resumes.
//
// The raises: raise_gossip_halt (a member taking a slot, tick_reset), raise_gate_halt (k_unpack_a's gate),
// raise_diff_halt and count_listed (the lister), note_wrote (member control). The host clears a word after it has
// acted on it.
#pragma once
#include <stdint.h>

namespace swim {

// ---- Dev::halt ----
enum HaltWord : uint32_t {
  // tick + 1 of the member kernel after which the gossip plane is needed (0: none); row shards: of the tick whose
  // exchange A needs the host (k_unpack_a's gate)
  HALT_GOSSIP = 0,
  // one GPU, batches that queue no k_sync_diff on untimed ticks (step.hip): the diff-halt, tick + 1 of the lister that
  // listed work for a diff nobody queued (k_ack_resolve); every later launch of the batch returns at once, member(tick)
  // included, and the host runs that diff. A word of its own: HALT_GOSSIP = k may also be member(k - 1)'s.
  HALT_DIFF = 1,
  // entries the lister has listed since create (the host's re-enable rule)
  HALT_LISTED = 2,
  // tick + 1 of the latest member-kernel launch of a one-GPU speculative batch that did something the lister's verdict
  // depends on (note_wrote); the host clears it when it reads it non-zero. Stops the launches of a lister-free batch only.
  HALT_WROTE = 3,
  // k_masks_any (the host's look before it enters the lister-free mode): some row has a dirty chunk
  HALT_MASKS = 4,
  HALT_WORDS = 5  // adjacent: one copy reads them back
};

// The words a launch decides on, HALT_GOSSIP .. HALT_WROTE, read once, the four adjacent words as one 16-byte line
// segment (Dev::halt is 16-byte aligned: word SH_HALT of the counter rows' allocation, or an allocation of its own), so
// no predicate waits for one word after the other. Every predicate of the table above decides on a HaltWords; the
// overloads that take the pointer load and decide.
// The loads are system-scope like the volatile loads they replace (the same cache-bypass bits), but relaxed atomics, two
// of 8 bytes issued back to back: the compiler completes every volatile load with a full vector-memory wait directly
// behind it (which is what made three words three serial round trips), and it has no 16-byte atomic. A caller may so
// issue further loads behind these and wait once for all of them (member.hip).
struct HaltWords {
  uint32_t hg, hd, listed, hw;
};
static_assert(HALT_GOSSIP == 0 && HALT_DIFF == 1 && HALT_LISTED == 2 && HALT_WROTE == 3, "HaltWords is the first four halt words");
__device__ __forceinline__ HaltWords halt_load(const uint32_t* halt) {
  // (global loads: the words are device memory, and a FLAT load would count on the scalar loads' wait counter too)
  typedef const __attribute__((address_space(1))) unsigned long long* G;
  const unsigned long long a = __hip_atomic_load((G)halt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM),
                           b = __hip_atomic_load((G)halt + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return HaltWords{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
}

__device__ __forceinline__ bool halted(const HaltWords& h) { return h.hg != 0u; }
// lf: a launch of a lister-free batch (LS_LF, MT_LF): a member kernel of an earlier tick wrote
__device__ __forceinline__ bool halted_wrote(const HaltWords& h, uint32_t k, bool lf) { return lf && h.hw != 0u && h.hw <= k; }
__device__ __forceinline__ bool halted_diff(const HaltWords& h, bool lf) { return (h.hg | h.hd) != 0u || (lf && h.hw != 0u); }
__device__ __forceinline__ bool halted_lister(const HaltWords& h, uint32_t k, bool lf) {
  return h.hg || (h.hd && h.hd != k + 1u) || halted_wrote(h, k, lf);
}
__device__ __forceinline__ bool halted_before(const HaltWords& h, uint32_t k) { return h.hg != 0u && h.hg - 1u < k; }
__device__ __forceinline__ bool halted_uncommitted(const HaltWords& h, uint32_t k) { return halted_before(h, k + 1u); }
__device__ __forceinline__ bool halted_member(const HaltWords& h, uint32_t k, bool lf = false) {
  return halted_before(h, k) || h.hd != 0u || halted_wrote(h, k, lf);
}
// a recorded watch sample of tick t >= 1, queued behind member(t - 1): the state at rest at tick t does not exist (yet)
__device__ __forceinline__ bool halted_sample(const HaltWords& h, uint32_t t, bool lf) {
  return halted_uncommitted(h, t - 1u) || h.hd != 0u || halted_wrote(h, t - 1u, lf);
}

__device__ __forceinline__ bool halted(const uint32_t* halt) { return halted(halt_load(halt)); }
__device__ __forceinline__ bool halted_diff(const uint32_t* halt, bool lf) { return halted_diff(halt_load(halt), lf); }
__device__ __forceinline__ bool halted_lister(const uint32_t* halt, uint32_t k, bool lf) {
  return halted_lister(halt_load(halt), k, lf);
}
__device__ __forceinline__ bool halted_before(const uint32_t* halt, uint32_t k) { return halted_before(halt_load(halt), k); }
__device__ __forceinline__ bool halted_uncommitted(const uint32_t* halt, uint32_t k) {
  return halted_uncommitted(halt_load(halt), k);
}
__device__ __forceinline__ bool halted_member(const uint32_t* halt, uint32_t k, bool lf = false) {
  return halted_member(halt_load(halt), k, lf);
}
__device__ __forceinline__ bool halted_sample(const uint32_t* halt, uint32_t t, bool lf) {
  return halted_sample(halt_load(halt), t, lf);
}

__device__ __forceinline__ void raise_gossip_halt(uint32_t* halt, uint32_t k) {
  *(volatile uint32_t*)(halt + HALT_GOSSIP) = k + 1u;
}
// (a plain store: one thread of the grid, read by later launches only)
__device__ __forceinline__ void raise_gate_halt(uint32_t* halt, uint32_t k) { halt[HALT_GOSSIP] = k + 1u; }
__device__ __forceinline__ void raise_diff_halt(uint32_t* halt, uint32_t k) {
  *(volatile uint32_t*)(halt + HALT_DIFF) = k + 1u;
}
__device__ __forceinline__ void count_listed(uint32_t* halt, uint32_t n) { atomicAdd(halt + HALT_LISTED, n); }
// member control of tick k did something the lister's verdict depends on (a plain store of the launch's own tick, as
// raise_gossip_halt: every writer of one launch stores the same value, later launches read it)
__device__ __forceinline__ void note_wrote(uint32_t* halt, uint32_t k) { *(volatile uint32_t*)(halt + HALT_WROTE) = k + 1u; }

// ---- launch flags ----
// k_member_tick_t's flag
enum : uint32_t {
  MT_END = 1u,   // one GPU: the launch does the end-of-tick work (the last block: tick_flag)
  MT_SPEC = 2u,  // a launch of a speculative batch
  MT_LF = 4u,    // ... of a lister-free one: it returns at once when an earlier tick's member kernel wrote (HALT_WROTE)
  // no lister ran for this tick (an untimed tick of a lister-free batch): the receivers count their inbound messages
  // as the lister would have in a clean cluster (P1, the triage's dead branch)
  MT_NOLIST = 8u,
};
constexpr bool mt_spec(uint32_t flag) { return (flag & MT_SPEC) != 0u; }
constexpr bool mt_lf(uint32_t flag) { return (flag & MT_LF) != 0u; }
constexpr bool mt_nolist(uint32_t flag) { return (flag & MT_NOLIST) != 0u; }
// a one-GPU speculative launch: the resets at its start (tick_reset), the member taking a slot raises the halt
constexpr bool mt_spec_one_gpu(uint32_t flag) { return (flag & (MT_END | MT_SPEC)) == (MT_END | MT_SPEC); }
// the last block to finish closes the tick (tick_flag): one GPU, not speculative
constexpr bool mt_closes_tick(uint32_t flag) { return (flag & (MT_END | MT_SPEC)) == MT_END; }

// the lister's spec (k_ack_resolve), and what launch_diff takes
enum : uint32_t {
  LS_SPEC = 1u,    // a launch of a speculative batch
  LS_NODIFF = 2u,  // no k_sync_diff follows this launch: a block that lists an entry raises the diff-halt of its tick
  LS_LF = 4u,      // a (timed) launch of a lister-free batch: the lister and the diff also stop on HALT_WROTE
};

// ---- the host-mapped flag block (Dev::hflag, swim_handle::hflag) ----
enum HFlag : uint32_t {
  HF_USED = 0,        // gossip slots in use after this tick's member control (W == 1)
  HF_SHARD_HALT = 1,  // HALT_GOSSIP read back after a speculative sharded batch
  // with Dev::rfill, the previous gossip plane's peaks (grow.hip): the largest receipt-ring fill, routed receipts,
  // replay sends, slow-path sends, history entries in use
  HF_PEAK0 = 2,
  HF_FILL = HF_PEAK0,
  HF_NRC,
  HF_NRP,
  HF_NSL,
  HF_NHIST,
  HF_STREAMED = 7,  // a narrow chunk was streamed since the host's last look at the rebase counters (k_ack_resolve)
  HF_HALT = 8,      // Dev::halt's words read back after a one-GPU speculative batch
  HF_WORDS = HF_HALT + HALT_WORDS
};
constexpr uint32_t HF_NPEAK = 5, HF_BYTES = 64;
static_assert(HF_NHIST + 1 == HF_PEAK0 + HF_NPEAK && HF_NHIST < HF_STREAMED, "the peak words are adjacent");
static_assert(HALT_GOSSIP == 0 && HALT_DIFF == 1 && HALT_LISTED == 2 && HALT_WROTE == 3 && HALT_MASKS == 4 && HALT_WORDS == 5,
              "the halt words are adjacent: one copy reads them back, word w into hflag[HF_HALT + w]");
static_assert(HF_WORDS * 4 <= HF_BYTES, "the flag block fits its allocation");
// Dev::hsh, the device copy of what tick_flag publishes (it writes host memory only on a change): the slots in use, then
// the peaks in HFlag's order
enum : uint32_t { HSH_USED = 0, HSH_PEAK0 = 1, HSH_WORDS = HSH_PEAK0 + HF_NPEAK };
constexpr uint32_t hsh_of(HFlag w) { return w == HF_USED ? HSH_USED : HSH_PEAK0 + (w - HF_PEAK0); }  // hflag word w's copy
constexpr uint32_t hflag_of(uint32_t i) { return i == HSH_USED ? HF_USED : HF_PEAK0 + (i - HSH_PEAK0); }  // and back

// ---- SWIM_EXP bits (Dev::exp): timing experiments and debugging aids; most give wrong results ----
enum : uint32_t {
  EXP_NO_REPLAY = 1,      // no infectedFrom replay (no longer read)
  EXP_NO_TARGETS = 2,     // no per-target work (no longer read)
  EXP_GOSSIP_WORK = 4,    // gossip-send work units counted (ctr[8..12], ctr[16..19]) and dumped after each step
  EXP_ROUTE_ALL = 8,      // route every receipt to P4 (debugging aid)
  EXP_CYCLES_SUM = 16,    // member-kernel shader cycles per phase, summed over members (ctr[8..12])
  EXP_SKIP_CLASS0 = 32,   // skip the member bodies of class 0
  EXP_SKIP_CLASS123 = 64, // skip the member bodies of classes 1-3
  EXP_CYCLES_MAX = 128,   // the largest per-member cycles of each phase instead; full walks, largest candidate count
  EXP_NO_EVENT = 256,     // no per-tick event or host wait (the gossip plane is never launched)
  EXP_WAVE_CLOCK = 512,   // per-wave wall-clock stamps of the latest member kernel (Dev::wt)
  EXP_CYCLES = EXP_CYCLES_SUM | EXP_CYCLES_MAX,
};
// Dev::wt, words per wave: 0-3 the kernel's own stamps (entry, after the triage, after the bodies, exit), 4-15 the
// general body's laps (member.hip Lap), then the light path's send_sync's: just before and just after the wave's latest message-slot
// reservation, and after the list-link exchange that followed it returned (stamped by the first lane active there)
// Word 19: the wave's clock at the kernel's true entry, in front of the halt check and every load (word 0 is stamped behind
// the halt decision).
constexpr uint32_t WT_WORDS = 20, WT_SLOT0 = 16, WT_SLOT1 = 17, WT_LINK = 18, WT_ENTRY = 19;

}  // namespace swim
