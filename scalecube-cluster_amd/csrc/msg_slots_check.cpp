// msg_slots_check.cpp — the message-slot scheme of msg_slots.h on the CPU (tests/test_msg_slots_host.py builds this with
// the host compiler under ASan + UBSan and runs it): senders of every shard take slots one at a time and a wave at a
// time, in random order, and the readers' enumeration must visit exactly what was taken.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "msg_slots.h"

using namespace swim;

static int fails = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (fails++ < 20) {                         \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                      \
        printf("\n");                             \
      }                                           \
    }                                             \
  } while (0)

// what the device does for the n lanes of a wave of shard s that send together (dev_util.h msg_take): one add on the
// shard's counter, then one on the overflow counter for the lanes whose index reached Q
static void take_wave(const MsgLayout& L, std::vector<uint32_t>& cnt, uint32_t& nover, uint32_t s, uint32_t n,
                      std::vector<uint32_t>& got) {
  if (L.S == 1) {
    const uint32_t base = nover;
    nover += n;
    for (uint32_t r = 0; r < n; ++r) got.push_back(msg_over_slot(L, base + r));
    return;
  }
  const uint32_t base = cnt[s];
  cnt[s] += n;
  uint32_t nov = 0;
  for (uint32_t r = 0; r < n; ++r) nov += base + r >= L.Q;
  const uint32_t obase = nover;
  nover += nov;
  uint32_t o = 0;
  for (uint32_t r = 0; r < n; ++r)
    got.push_back(base + r < L.Q ? msg_fast_slot(L, s, base + r) : msg_over_slot(L, obase + o++));
}

// demand[s] sends per shard, in random order, singly (waves == false) or in random groups of up to 64
static void run(uint32_t S, uint32_t cap, const std::vector<uint32_t>& demand, bool waves, std::mt19937& rng, const char* what) {
  const MsgLayout L = msg_layout(cap, S);
  CHECK(L.S == S && (1u << L.sh) == S && L.R == L.S * L.Q && L.R <= cap, "%s: layout S %u cap %u", what, S, cap);
  CHECK(S == 1 ? L.Q == 0 && L.R == 0 : L.Q == cap / (4 * S), "%s: Q %u at S %u cap %u", what, L.Q, S, cap);
  std::vector<uint32_t> order;
  for (uint32_t s = 0; s < S; ++s) order.insert(order.end(), demand[s], s);
  std::shuffle(order.begin(), order.end(), rng);
  std::vector<uint32_t> cnt(S, 0), got;
  uint32_t nover = 0;
  if (!waves) {
    for (uint32_t s : order) got.push_back(msg_take_serial(L, cnt.data(), &nover, s));
  } else {
    std::vector<uint32_t> left = demand;
    for (size_t i = 0; i < order.size(); ++i) {  // (a shard drawn from the shuffled order, a group of what it has left)
      const uint32_t s = order[i];
      if (!left[s]) continue;
      const uint32_t n = 1 + rng() % std::min<uint32_t>(64, left[s]);
      take_wave(L, cnt, nover, s, n, got);
      left[s] -= n;
    }
    for (uint32_t s = 0; s < S; ++s)
      if (left[s]) take_wave(L, cnt, nover, s, left[s], got);
  }
  // E_MSGS exactly for the overflow demand beyond the overflow region
  uint64_t want_over = 0, total = 0;
  for (uint32_t s = 0; s < S; ++s) total += demand[s], want_over += S == 1 ? demand[s] : demand[s] > L.Q ? demand[s] - L.Q : 0;
  const uint64_t room = cap - L.R, want_err = want_over > room ? want_over - room : 0;
  std::vector<uint32_t> taken;
  uint64_t err = 0;
  for (uint32_t i : got) {
    if (i >= cap) ++err;
    else taken.push_back(i);
  }
  CHECK(got.size() == total, "%s: %zu takes for %llu sends", what, got.size(), (unsigned long long)total);
  CHECK(nover == want_over, "%s: overflow demand %u, expected %llu", what, nover, (unsigned long long)want_over);
  CHECK(err == want_err, "%s: S %u cap %u: %llu takes without a slot, expected %llu", what, S, cap, (unsigned long long)err,
        (unsigned long long)want_err);
  if (S == 1)  // as before the shards: 0, 1, 2, ... in the order of the takes
    for (size_t i = 0; i < taken.size(); ++i) CHECK(taken[i] == i, "%s: S 1 slot %zu is %u", what, i, taken[i]);
  std::sort(taken.begin(), taken.end());
  for (size_t i = 0; i < taken.size(); ++i) {
    CHECK(taken[i] < cap, "%s: slot %u at cap %u", what, taken[i], cap);
    CHECK(i == 0 || taken[i] != taken[i - 1], "%s: slot %u taken twice (S %u cap %u)", what, taken[i], S, cap);
  }
  // the readers' enumeration: exactly the taken set, ascending
  std::vector<uint32_t> seen;
  const uint32_t n = msg_for_each(L, cnt.data(), nover, [&](uint32_t i) { seen.push_back(i); });
  CHECK(n == seen.size() && seen == taken, "%s: S %u cap %u: the enumeration visits %zu slots, %zu were taken", what, S, cap,
        seen.size(), taken.size());
  // and position by position, as the device walks it
  uint32_t c_max = 0;
  for (uint32_t s = 0; S > 1 && s < S; ++s) c_max = std::max(c_max, msg_fill(L, cnt[s]));
  const MsgEnum E = msg_enum(L, c_max, nover);
  CHECK(E.total <= cap && E.nfast <= L.R, "%s: %u positions, %u fast at cap %u R %u", what, E.total, E.nfast, cap, L.R);
  std::vector<uint32_t> walk;
  for (uint32_t j = 0; j < E.total; ++j) {
    const uint32_t fill = j < E.nfast ? msg_fill(L, cnt[msg_pos_shard(L, j)]) : 0u;
    if (msg_pos_used(L, E, j, fill)) walk.push_back(msg_pos_slot(L, E, j));
  }
  CHECK(walk == taken, "%s: S %u cap %u: the position walk differs from the taken set", what, S, cap);
  // the dense walk: the same set, without holes
  std::vector<uint32_t> dense;
  for (uint32_t q = 0; q < taken.size(); ++q) dense.push_back(msg_dense_slot(L, cnt.data(), q));
  std::sort(dense.begin(), dense.end());
  CHECK(dense == taken, "%s: S %u cap %u: the dense walk differs from the taken set", what, S, cap);
}

int main() {
  std::mt19937 rng(20240614u);
  const uint32_t shards[] = {1, 2, 8, 32}, caps[] = {4, 33, 1030, 12357};
  for (uint32_t s = 0; s <= 40; ++s) CHECK(msg_shards_ok(s) == (s == 1 || s == 2 || s == 4 || s == 8 || s == 16 || s == 32), "msg_shards_ok(%u)", s);
  for (uint32_t S : shards)
    for (uint32_t cap : caps)
      for (int waves = 0; waves < 2; ++waves) {
        const MsgLayout L = msg_layout(cap, S);
        std::vector<uint32_t> d(S, 0);
        run(S, cap, d, waves, rng, "nothing sent");
        for (uint32_t s = 0; s < S; ++s) d[s] = cap / S;  // evenly spread, the whole buffer but the remainder
        run(S, cap, d, waves, rng, "even");
        for (int rep = 0; rep < 6; ++rep) {  // random demands: below capacity, around it, beyond it
          const uint32_t scale = rep < 2 ? cap / (2 * S) + 1 : rep < 4 ? cap / S + 2 : 2 * cap / S + 3;
          for (uint32_t s = 0; s < S; ++s) d[s] = rng() % (scale + 1);
          run(S, cap, d, waves, rng, "random");
        }
        // one shard takes everything: served up to Q + (cap - R), then E_MSGS
        for (uint32_t extra : {0u, 1u, 7u}) {
          std::fill(d.begin(), d.end(), 0u);
          d[S - 1] = L.Q + (cap - L.R) + extra;
          run(S, cap, d, waves, rng, "one shard takes everything");
        }
        // every shard exactly full, then one more sender anywhere
        for (uint32_t s = 0; s < S; ++s) d[s] = L.Q;
        d[0] += cap - L.R;
        run(S, cap, d, waves, rng, "exactly full");
        d[S / 2] += 1;
        run(S, cap, d, waves, rng, "one past full");
      }
  if (fails) {
    printf("msg_slots_check: %d failures\n", fails);
    return 1;
  }
  printf("msg_slots_check ok\n");
  return 0;
}
