// step_rounds_host.cpp -- raftsql_amd/csrc/raftq_step_rounds.hpp against a naive model (tests/test_step_rounds_host.py builds this
// with g++ -fsanitize=address,undefined and runs it: no GPU, no HIP).  The model: a std::map from group to the records seen so far
// gives each record's round; the staged order is the records of round 0 in caller order, then those of round 1, and so on.
#include "raftq_step_rounds.hpp"

#include <cstdio>
#include <map>
#include <random>
#include <vector>

namespace {

int failures = 0;
#define CHECK(c, ...)                                         \
  do {                                                        \
    if (!(c)) {                                               \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                      \
      std::fprintf(stderr, "\n");                             \
      ++failures;                                             \
    }                                                         \
  } while (0)

// the state a handle keeps across calls
struct State {
  std::vector<uint64_t> mark, start;
  std::vector<uint32_t> round, pos;
  uint32_t epoch = 0;
};

const uint32_t kUntouched = 0xabababab;

// one call of the planner on `groups`, compared with the model; returns the round count
uint32_t check(State& st, uint64_t G, const std::vector<uint64_t>& groups, const char* what) {
  const uint64_t n = groups.size();
  std::map<uint64_t, uint32_t> seen;
  std::vector<uint32_t> want_round(n);
  uint32_t want_rounds = 1;
  for (uint64_t i = 0; i < n; ++i) {
    want_round[i] = seen[groups[i]]++;
    want_rounds = std::max(want_rounds, want_round[i] + 1);
  }
  std::vector<uint32_t> want_pos;
  std::vector<uint64_t> want_start;
  for (uint32_t r = 0; r < want_rounds; ++r) {
    want_start.push_back(want_pos.size());
    for (uint64_t i = 0; i < n; ++i)
      if (want_round[i] == r) want_pos.push_back((uint32_t)i);
  }
  want_start.push_back(n);

  // with one round the reorder arrays are not needed and must not be touched
  st.pos.assign(3, kUntouched);
  st.start.assign(2, 0xabababababababab);
  const uint32_t epoch_before = st.epoch;
  const uint32_t got = raftq_rounds::plan(G, n, [&](uint64_t i) { return groups[i]; }, st.mark, st.epoch, st.round, st.start, st.pos);
  CHECK(got == want_rounds, "%s: %u rounds, the model has %u", what, got, want_rounds);
  CHECK(st.epoch != 0 && st.epoch == (epoch_before == 0xffffffffu ? 1u : epoch_before + 1), "%s: epoch %u after %u", what, st.epoch, epoch_before);
  CHECK(st.mark.size() == G, "%s: %zu marks for %llu groups", what, st.mark.size(), (unsigned long long)G);
  CHECK(st.round == want_round, "%s: the records' rounds differ from the model's", what);
  if (want_rounds == 1) {
    CHECK(st.pos == std::vector<uint32_t>(3, kUntouched) && st.start == std::vector<uint64_t>(2, 0xabababababababab),
          "%s: one round, yet the reorder arrays were written", what);
  } else {
    CHECK(st.start == want_start, "%s: round_start differs from the model's", what);
    CHECK(st.pos == want_pos, "%s: the staged order differs from the model's (stable within a round)", what);
  }
  return got;
}

}  // namespace

int main() {
  unsigned cases = 0;
  {  // every group distinct: one round, no reorder arrays (in caller order, reversed, and the empty batch)
    State st;
    std::vector<uint64_t> g;
    for (uint64_t i = 0; i < 50; ++i) g.push_back(i);
    CHECK(check(st, 50, g, "distinct") == 1, "distinct: more than one round");
    CHECK(check(st, 50, std::vector<uint64_t>(g.rbegin(), g.rend()), "distinct, reversed") == 1, "reversed: more than one round");
    CHECK(check(st, 50, {}, "empty") == 1, "empty: more than one round");
    cases += 3;
  }
  for (uint32_t k : {2u, 3u, 17u, 64u}) {  // one group named k times: k rounds of one
    State st;
    CHECK(check(st, 7, std::vector<uint64_t>(k, 5), "one hot group") == k, "one hot group: not %u rounds", k);
    for (uint32_t r = 0; r <= k; ++r) CHECK(st.start[r] == r, "one hot group: round %u starts at %llu", r, (unsigned long long)st.start[r]);
    ++cases;
  }
  {  // seeded random batches, G = 7 and n <= 64, all on one state: every call follows another's marks
    State st;
    std::mt19937_64 rng(20251019);
    for (int t = 0; t < 4000; ++t, ++cases) {
      std::vector<uint64_t> g(rng() % 65);
      const uint64_t span = 1 + rng() % 7;  // (a narrow span gives long runs)
      for (auto& x : g) x = rng() % span;
      check(st, 7, g, "random");
    }
  }
  {  // two consecutive calls on the same state: the first call's marks must not leak into the second
    State st;
    CHECK(check(st, 7, {3, 3, 3, 1}, "first call") == 3, "first call: not 3 rounds");
    CHECK(check(st, 7, {3, 1, 0}, "second call") == 1, "second call: the first call's marks leaked");
    CHECK(check(st, 7, {1, 3, 1, 3, 0}, "third call") == 2, "third call: not 2 rounds");
    CHECK(check(st, 9, {8, 3, 8}, "a state sized for another G") == 2, "resized: not 2 rounds");  // (marks are re-made)
    cases += 4;
  }
  {  // the epoch wraps from 0xffffffff to 1 with stale marks present: marks of the old epoch 1 must not count
    State st;
    CHECK(check(st, 7, {2, 2, 4}, "epoch 1") == 2 && st.epoch == 1, "epoch 1");
    const std::vector<uint64_t> stale = st.mark;  // group 2 -> (1 << 32 | 2), group 4 -> (1 << 32 | 1)
    st.epoch = 0xfffffffe;
    CHECK(check(st, 7, {6, 6, 6}, "epoch 0xffffffff") == 3 && st.epoch == 0xffffffffu, "epoch 0xffffffff");
    st.mark = stale;
    st.mark[6] = (uint64_t)0xffffffffu << 32 | 3;
    CHECK(check(st, 7, {2, 4, 6, 0}, "wrapped epoch") == 1 && st.epoch == 1, "wrapped: stale marks of epoch 1 counted");
    CHECK(check(st, 7, {2, 4, 2}, "after the wrap") == 2 && st.epoch == 2, "after the wrap");
    cases += 4;
  }
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok: %u batches planned as the model plans them\n", cases);
  return 0;
}
