// raftq_step_rounds.hpp -- raftq_apply_log_deltas' round planner.  Host code only: the standard library, no HIP, no raftq_t
// (tests/c/step_rounds_host.cpp runs it against a naive model).
//
// Records of one group apply in order: the k-th record that names a group goes into launch ("round") k.  The common batch names
// every group once: one round, caller order, no bookkeeping.  Whether it does is found with a per-group mark (epoch << 32 |
// records seen this call) -- an array lookup per record, not a hash map: the map this replaces was most of the call's host time
// at 10^4 records (raftq_node's "deltas" phase).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace raftq_rounds {

// The vectors are the caller's, kept across calls so that a call allocates nothing once they have grown: `mark` [G] and `epoch`
// carry over (a mark of an earlier epoch counts as zero; when the epoch wraps the marks are cleared), the rest is output.
//   round[i]        the round of record i (group_of(i) < G is the caller's to check)
//   round_start[r]  with more than one round: the staged position where round r begins, [n_rounds] = n
//   pos_of[k]       with more than one round: the caller's index of the record staged at k -- a stable counting sort on the round
//                   number, O(n) whatever the skew, caller order within a round
// Returns the round count (1 for n == 0); with one round the staged order is the caller's and round_start / pos_of are not
// touched.  May throw std::bad_alloc; `mark` and `epoch` may have moved on by then, which only costs the next call its marks.
template <class GroupOf>
uint32_t plan(uint64_t G, uint64_t n, GroupOf group_of, std::vector<uint64_t>& mark, uint32_t& epoch, std::vector<uint32_t>& round,
              std::vector<uint64_t>& round_start, std::vector<uint32_t>& pos_of) {
  if (mark.size() != G) mark.assign(G, 0);
  if (++epoch == 0) {
    std::fill(mark.begin(), mark.end(), 0ull);
    epoch = 1;
  }
  const uint64_t ep = (uint64_t)epoch << 32;
  uint32_t n_rounds = 1;
  round.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t& mk = mark[group_of(i)];
    const uint32_t r = (mk >> 32) == epoch ? (uint32_t)mk : 0;
    mk = ep | (r + 1);
    round[i] = r;
    n_rounds = std::max(n_rounds, r + 1);
  }
  if (n_rounds == 1) return 1;
  round_start.assign((size_t)n_rounds + 1, 0);
  for (uint64_t i = 0; i < n; ++i) round_start[round[i] + 1]++;
  for (uint32_t r = 0; r < n_rounds; ++r) round_start[r + 1] += round_start[r];
  std::vector<uint64_t> fill(round_start.begin(), round_start.end() - 1);
  pos_of.resize(n);
  for (uint64_t i = 0; i < n; ++i) pos_of[fill[round[i]]++] = (uint32_t)i;
  return n_rounds;
}

}  // namespace raftq_rounds
