// raftq_step_walk_kernels.inc -- the three kernels that run Step's maybeCommit / poll: the sorted walk, the list walk and the log
// owner's tail reports.  Included FOUR times by raftq_step_kernels.hpp (inside namespace raftqk): over every slot and over each
// group's own voters, and both once more, without the tail reports, for raftq_respond_set_lead / raftq_respond_set_props.  Each time it sets
//   RAFTQ_WALK_KERNEL(stem)  the kernel's name: stem_kernel over every slot, stem_voters_kernel over each group's own voters,
//                            stem_lead_kernel / stem_lead_voters_kernel for the forms that answer broadcasts with entries too (a won
//                            election's, a forwarded proposal's: NodeArrays::ans_lead / ans_props)
//   RAFTQ_WALK_MASKED        NodeT's argument list: MASKED, or "MASKED, true" for the LEAD forms
//   RAFTQ_WALK_PARAM         the masked form's extra, LAST parameter (", const uint16_t* __restrict__ voters"): NodeArrays is a
//                            by-value argument of every Step-family kernel and stays as it is
//   RAFTQ_WALK_VOTERS        the same, handed to NodeT's constructor (", voters")
//   RAFTQ_WALK_NO_DELTAS     (optional) the two walks only: leave the tail reports out
//   RAFTQ_WALK_CQ            true in the *_cq_* expansions (NodeT's CQ form, raftq_set_check_quorum): type 12 is a known kind there, and
//                            under NodeArrays::pv (raftq_set_pre_vote) so are types 17 and 18 and RAFTQ_OUT_PRE_CAMPAIGN's packing; under
//                            NodeArrays::lt (raftq_set_lead_transfer) so are types 13 and 14, under NodeArrays::ri (raftq_set_read_index)
//                            types 15 and 16
//   RAFTQ_WALK_READS_PARAM   the *_cq_* walks' extra, very last parameter (", ReadRec* __restrict__ reads": raftq_set_read_index's
//                            records, nullptr unless the mode is RAFTQ_READ_SAFE); empty in every other expansion
//   RAFTQ_WALK_READS         the same, handed to NodeT's constructor behind the voters (", reads", or ", nullptr, reads" where there
//                            are none)
// One text, four walks of each kind and two tail-report kernels.  Why an include and not a template <bool MASKED> body the kernels call: the inliner simplifies such
// a body BEFORE it meets the kernel (no launch bounds, no noalias arguments, NodeArrays behind a generic reference), and all three
// unmasked kernels came out different from their parent's -- step_lists_kernel with other loads and another register count
// (tools/isa_unchanged.py; profiles/r12/README.md).  As an include the unmasked expansion is token for token what it was.

// ---- (3) the sorted walk: one lane per run of equal keys
static __global__ __launch_bounds__(kBlock) void RAFTQ_WALK_KERNEL(step)(NodeArrays a, const MsgRec* __restrict__ msgs,
                                                      const uint64_t* __restrict__ keys_sorted,
                                                      const uint32_t* __restrict__ order, void* __restrict__ out,
                                                      uint8_t compact, uint64_t n, unsigned long long* n_heads,
                                                      const unsigned int* bad RAFTQ_WALK_PARAM RAFTQ_WALK_READS_PARAM) {
  if (*bad) return;  // a malformed record somewhere in the batch: nothing is applied
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool head = false;
  uint64_t g = 0;
  if (k < n) {
    g = keys_sorted[k];
    head = (k == 0 || keys_sorted[k - 1] != g) && g < a.n_groups;  // (key n_groups: the RAFTQ_MSGF_SKIP records, answered by step_keys_kernel)
  }
  const uint64_t hb = __ballot(head);
  if ((threadIdx.x & 63) == 0 && hb) atomicAdd(n_heads, (unsigned long long)__popcll(hb));
  if (!head) return;
  NodeT<RAFTQ_WALK_MASKED> node(a, g RAFTQ_WALK_VOTERS RAFTQ_WALK_READS);
  for (uint64_t j = k; j < n && keys_sorted[j] == g; ++j) {
    const uint32_t i = order[j];
    const MsgRec m = msgs[i];
    StepOutRec o;
    node.step(m, o);
    node.respond(m, o, i);
    put_result<RAFTQ_WALK_CQ, RAFTQ_WALK_CQ>(out, i, o, compact);
  }
  node.store();
}

// ---- (3b) the list walk (raftq_step_kernels.hpp "(2b, 3b)"): the lane of a group's first message walks its list
static __global__ __launch_bounds__(kBlock) void RAFTQ_WALK_KERNEL(step_lists)(NodeArrays a, const MsgRec* __restrict__ msgs,
                                                                   void* __restrict__ out, uint8_t compact, uint64_t n,
                                                                   uint64_t n_groups,
                                                                   const uint32_t* __restrict__ next,
                                                                   unsigned long long* n_heads, unsigned int* tail_skipped,
                                                                   const unsigned int* bad, const unsigned int* stall, CopyRide ride RAFTQ_WALK_PARAM RAFTQ_WALK_READS_PARAM) {
  if (blockIdx.x < ride.blocks) {  // the rest of the previous batch's results (see CopyRide)
    copy_ride(ride);
    return;
  }
  const uint64_t i = (uint64_t)(blockIdx.x - ride.blocks) * kBlock + threadIdx.x;
  const bool stalled = *stall != 0;  // this batch, or one before it that has not been replayed yet, needs the sorted path
  if (stalled || *bad) {             // (*bad: a malformed record somewhere in the batch) -- nothing is applied;
    if (stalled && i == 0) *tail_skipped = 1u;
    if (i < n && classify(msgs[i], n_groups, a.n_peers, a.msg_flags, a.recs, a.props, RAFTQ_WALK_CQ, RAFTQ_WALK_CQ && a.pv, RAFTQ_WALK_CQ && a.lt, RAFTQ_WALK_CQ && a.ri != 0) == kTake) {  // every message empties its group's list words (idempotent)
      NodeRec* r = a.rec + msgs[i].group;
      r->lst_head = kNil;
      r->lst_cnt = 0;
      r->lst_min = kNil;
    }
    return;
  }
  uint64_t g = 0;
  bool owner = false;
  if (i < n) {
    g = msgs[i].group;
    // (a RAFTQ_MSGF_SKIP record belongs to no group -- its group field may hold anything -- and was answered by the link kernel)
    owner = !(a.msg_flags && (msgs[i].pad[1] & kMsgfSkip)) && a.rec[g].lst_min == (uint32_t)i;
  }
  const uint64_t ob = __ballot(owner);
  if ((threadIdx.x & 63) == 0 && ob) atomicAdd(n_heads, (unsigned long long)__popcll(ob));
  if (!owner) return;
  NodeT<RAFTQ_WALK_MASKED> node(a, g RAFTQ_WALK_VOTERS RAFTQ_WALK_READS);  // (the record's line is in the L1 already: the owner test read it)
  const uint32_t c = node.lst_cnt;
  if (c == 1) {
    StepOutRec o;
    const MsgRec m = msgs[i];
    node.step(m, o);
    node.respond(m, o, i);
    put_result<RAFTQ_WALK_CQ, RAFTQ_WALK_CQ>(out, i, o, compact);
  } else {
    uint32_t pos[kMaxRun];
    uint32_t p = node.lst_head;
    for (uint32_t k = 0; k < c; ++k) {  // gather, inserting in ascending order of batch position
      uint32_t j = k;
      while (j > 0 && pos[j - 1] > p) {
        pos[j] = pos[j - 1];
        --j;
      }
      pos[j] = p;
      p = next[p];
    }
    for (uint32_t k = 0; k < c; ++k) {
      const MsgRec m = msgs[pos[k]];
      StepOutRec o;
      node.step(m, o);
      node.respond(m, o, pos[k]);
      put_result<RAFTQ_WALK_CQ, RAFTQ_WALK_CQ>(out, pos[k], o, compact);
    }
  }
  // the record goes back with the group's list empty for the next batch.  Other lanes of this group only compare lst_min
  // with their own position to learn that they are not the owner: kNil tells them the same.
  node.store();
}

#ifndef RAFTQ_WALK_NO_DELTAS
// the log owner's tail reports; records are unique per group within a launch (the host splits
// repeated groups into successive launches)
static __global__ __launch_bounds__(kBlock) void RAFTQ_WALK_KERNEL(log_deltas)(NodeArrays a, const LogDeltaRec* __restrict__ d,
                                                                   uint64_t n, uint64_t* __restrict__ committed_out RAFTQ_WALK_PARAM) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const LogDeltaRec r = d[i];
  NodeT<RAFTQ_WALK_MASKED> node(a, r.group RAFTQ_WALK_VOTERS);
  node.last_index = r.last_index;
  node.last_term = r.last_term;
  if (node.role == kLeader) {
    if (node.match(a.self) < node.last_index) node.set_match(a.self, node.last_index);
    (void)node.maybe_commit();
  } else if (r.commit_to != 0) {
    node.commit_to(r.commit_to);
  }
  node.store(false);
  if (committed_out) committed_out[i] = node.committed;
}
#endif
