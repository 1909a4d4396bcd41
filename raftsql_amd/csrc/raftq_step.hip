// raftq_step.hip -- implementation of include/raftq_step.h: the batched raft Step over
// the device-resident group state.  Host side: validate + stage the batch in pinned
// memory, key/sort/walk it on the handle's stream (raftq_step_kernels.hpp), copy the
// result records back.  No CPU path: the state machine itself runs only on the GPU.
#include "raftq_step.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "raftq_internal.hpp"
#include "raftq_step_kernels.hpp"
#include "raftq_step_rounds.hpp"
#include "raftq_wire.h"
#include "raftq_sort_kernels.hpp"
#include "raftq_wire_kernels.hpp"

using namespace raftqk;
using raftq_detail::ensure_staging;
using raftq_detail::ensure_tick_state;
using raftq_detail::fail;
using raftq_detail::use_device;

static_assert(sizeof(raftq_msg_t) == sizeof(MsgRec) && sizeof(raftq_step_out_t) == sizeof(StepOutRec) &&
                  sizeof(raftq_log_delta_t) == sizeof(LogDeltaRec) && sizeof(raftq_step_out_c_t) == sizeof(StepOutC) &&
                  sizeof(raftq_step_out_s_t) == sizeof(raftqk::StepOutS),
              "ABI struct mismatch");

namespace {

// bytes of one result record in the handle's format
uint32_t result_rec_bytes(const raftq_t* h) {
  return h->step_compact == raftqk::kFmtS32 ? (uint32_t)sizeof(raftqk::StepOutS) : h->step_compact ? (uint32_t)sizeof(StepOutC) : (uint32_t)sizeof(StepOutRec);
}

int ensure_node_state(raftq_t* h) {
  if (h->node_rec) return RAFTQ_OK;
  if (int rc = ensure_tick_state(h)) return rc;  // role, elapsed
  if (const char* w = std::getenv("RAFTQ_STEP_WALK")) h->step_walk_mode = std::strcmp(w, "sort") == 0 ? 0 : 1;
  // h->node_rec marks the state complete: it is assigned only once the records have been allocated AND their initialisation has
  // been launched (a failed launch used to leave the pointer set, and the next call stepped uninitialised records).
  // The stall word and the records come as a pair or not at all (256 bytes leaked per failed attempt).
  void* rec = nullptr;
  void* stall = nullptr;
  HIPCHK(h, raftq_buf::alloc_group({{&stall, 256}, {&rec, h->ld * sizeof(NodeRec), raftq_buf::Kind::device, nullptr, /*zero=*/false}}, h->stream));
  hipLaunchKernelGGL(node_init_kernel, dim3((unsigned)((h->ld + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, (NodeRec*)rec, h->ld);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    raftq_buf::free_device(rec, stall);
    HIPCHK(h, e);
  }
  h->step_stall = (unsigned int*)stall;
  h->node_rec = rec;
  h->have_terms = true;  // Step maintains the current-term gate itself (closed = 0 until a group leads)
  return RAFTQ_OK;
}

NodeArrays node_arrays(raftq_t* h, uint8_t recs = raftqk::kRecsCaller) {
  NodeArrays a;
  a.rec = (NodeRec*)h->node_rec;
  a.role = h->role;
  a.elapsed = h->elapsed;
  a.committed = h->committed[h->cur];
  a.first_idx = h->first_idx;
  a.match = h->match;
  a.votes = h->votes;
  a.ld = h->ld;
  a.n_peers = h->N;
  a.self = h->self_peer;
  a.msg_flags = h->step_msg_flags;
  a.recs = recs;
  a.props = h->step_props;
  a.n_groups = h->G;
  a.self_max = h->self_max;
  a.cq = h->cq;  // raftq_set_check_quorum: nullptr unless the switch is on
  a.election_tick = h->election_tick;
  a.pv = h->pre_vote;  // raftq_set_pre_vote: only ever on beside cq
  a.lt = h->lead_transfer;  // raftq_set_lead_transfer: likewise
  a.ri = h->read_index;     // raftq_set_read_index: likewise (its records go to the *_cq_* walks as a parameter: launch_walk_cq)
  if (h->resp_on) {  // raftq_step_frames_respond: the walks (the list walk, the sorted one, a stalled batch's replay) answer too
    a.resp = (raftqk::RespRec*)h->resp_dev.d;
    a.at_tail = h->resp_at_tail_d;
    a.resp_stamp = h->resp_stamp;
    a.ans_lead = h->resp_lead;
    a.ans_props = h->resp_props;
    a.resp_ent_base = h->resp_ent_base;
  }
  return a;
}

// The records' copies of role / committed / first_idx / match (raftq_step_kernels.hpp NodeRec) are re-read from the dense arrays
// when something other than Step has changed those since (raftq_capi.hip marks it): enqueued in front of whatever reads a record.
int ensure_mirror(raftq_t* h) {
  if (h->node_mirror_fresh) return RAFTQ_OK;
  hipLaunchKernelGGL(node_mirror_kernel, dim3((unsigned)((h->G + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, node_arrays(h), h->G);
  HIPCHK(h, hipGetLastError());
  h->node_mirror_fresh = true;
  h->node_mirror_refreshes++;
  return RAFTQ_OK;
}

}  // namespace
int raftq_detail::node_records_of(raftq_t* h, const char* who, raftqk::NodeArrays* out, bool tick_rounds, bool bcast) {
  if (int rc = raftq_detail::refuse_voters(h, who, false, tick_rounds, bcast)) return rc;
  if (int rc = ensure_node_state(h)) return rc;
  if (int rc = ensure_mirror(h)) return rc;
  *out = node_arrays(h);
  return RAFTQ_OK;
}
int raftq_detail::node_arrays_of(raftq_t* h, raftqk::NodeArrays* out) {
  if (int rc = node_records_of(h, "raftq_propose_frames", out, false, true)) return rc;
  h->last_flags &= ~RAFTQ_SWEEP_NO_ADOPT;  // as in raftq_step_submit: the live state moves
  return RAFTQ_OK;
}
namespace {

// device scratch of one batch, carved from a single allocation
struct Scratch {
  MsgRec* msgs;
  void* msgs40;  // packed inbound records as they arrived (raftq_step_submit_packed), widened into msgs on the device
  void* outs;  // StepOutRec[n] or StepOutC[n], then the 16-byte tail at tail_off(n, rec)
  uint64_t *keys_in, *keys_out;
  uint32_t *order_in, *order_out;
  uint32_t* next;  // sort-free walk: list links
  unsigned long long* n_heads;
  void* sort_scratch;
  size_t sort_bytes;
  // raftq_step_submit_wire only: the staged frames and what the decoder needs
  uint64_t* w_off;       // [n + 1] frame offsets, the stream bytes right behind them
  uint8_t* w_stream;
  uint64_t *w_cnt, *w_base;  // [n + 1] entries per message, their exclusive scan
  unsigned long long* w_bad;
  WireEnt* w_ents;
  uint64_t w_ents_cap;
  void* w_scan;
  size_t w_scan_bytes;
};

// the results of the last collected batch are no longer to be read (raftq_step_results*)
void forget_results(raftq_t* h) {
  h->step_last_out = nullptr;
  h->step_last_n = 0;
}

// raftq_step_set_voters on a handle with masks loaded: the walks and the tail reports launch the *_voters_kernel twins.  So do the
// walks of a raftq_step_frames_respond call (resp_on: the first pass and a stalled batch's replay) on a handle that opted in to
// raftq_bcast_set_voters -- on its own authority, as raftq_tick_elect_frames uses the masked Step
bool masked_step(const raftq_t* h) { return h->voters != nullptr && (h->step_voters || (h->resp_on && h->bcast_voters)); }
// raftq_respond_set_lead: the walks of a raftq_step_frames_respond call (the first pass and a stalled batch's replay) are the
// *_lead_kernel forms, whose respond() answers RAFTQ_OUT_BECAME_LEADER too; every other caller of the walks launches what it always did
// raftq_respond_set_props: the same forms -- "the walks that answer broadcasts with entries" -- launched when either switch is on
// (NodeArrays::ans_lead / ans_props say which of the two they answer)
bool lead_step(const raftq_t* h) { return h->resp_on && (h->resp_lead || h->resp_props); }

// One walk, launched in the form the handle's switches ask for.  raftq_step_walk_kernels.inc is expanded once per form, so a walk
// comes as four entry points over one parameter list: plain, *_voters (masked_step: h->voters is appended), *_lead (lead_step) and
// *_lead_voters.  The tail reports are never launched in a lead form and pass nullptr for those two.  The caller reads the launch's
// error (hipGetLastError).
template <class T>
struct as_is {
  using type = T;  // (keeps a parameter out of template argument deduction: A is what `plain` takes)
};
template <class... A>
void launch_walk(const raftq_t* h, dim3 grid, void (*plain)(A...), typename as_is<void (*)(A..., const uint16_t*)>::type voters,
                 typename as_is<void (*)(A...)>::type lead, typename as_is<void (*)(A..., const uint16_t*)>::type lead_voters,
                 typename as_is<A>::type... args) {
  const bool lead_form = lead != nullptr && lead_step(h);
  if (masked_step(h))
    hipLaunchKernelGGL((lead_form ? lead_voters : voters), grid, dim3(kBlock), 0, h->stream, args..., (const uint16_t*)h->voters);
  else
    hipLaunchKernelGGL((lead_form ? lead : plain), grid, dim3(kBlock), 0, h->stream, args...);
}

// ... and the *_cq_* forms (raftq_set_check_quorum), whose parameter lists end with raftq_set_read_index's records (nullptr unless
// the mode is RAFTQ_READ_SAFE)
template <class... A>
void launch_walk_cq(const raftq_t* h, dim3 grid, typename as_is<void (*)(A..., raftqk::ReadRec*)>::type plain,
                    typename as_is<void (*)(A..., const uint16_t*, raftqk::ReadRec*)>::type voters,
                    typename as_is<void (*)(A..., raftqk::ReadRec*)>::type lead,
                    typename as_is<void (*)(A..., const uint16_t*, raftqk::ReadRec*)>::type lead_voters,
                    typename as_is<A>::type... args) {  // (A is given by the caller: a pack in front of other parameters is not deduced)
  const bool lead_form = lead_step(h);
  raftqk::ReadRec* reads = (raftqk::ReadRec*)h->reads;
  if (masked_step(h))
    hipLaunchKernelGGL((lead_form ? lead_voters : voters), grid, dim3(kBlock), 0, h->stream, args..., (const uint16_t*)h->voters, reads);
  else
    hipLaunchKernelGGL((lead_form ? lead : plain), grid, dim3(kBlock), 0, h->stream, args..., reads);
}

// The opening of the one-call entry points (raftq_step_batch, raftq_step_frames*): the device, the caller's counts zeroed, no
// submitted batch in flight, the last results forgotten.
template <class ZeroCounts>
int one_call_open(raftq_t* h, const char* who, ZeroCounts zero_counts) {
  if (int rc = use_device(h)) return rc;
  zero_counts();
  if (h->step_collected != h->step_submitted)
    return fail(h, RAFTQ_ESTATE, std::string(who) + ": submitted batches are still in flight; collect them first");
  forget_results(h);
  return RAFTQ_OK;
}

// The closing of the frames calls, behind their collect: the decoder's verdict and counts.  A look-back that gave up overrides
// Step's result: the records Step read are not to be trusted, nor is what it made of them
int frames_close(raftq_t* h, const uint64_t* frame_off, uint64_t n, bool want_ents, uint64_t ents_cap, raftq_wire_counts_t* counts) {
  const int rc_dec = raftq_detail::wire_frames_finish(h, frame_off, n, want_ents, ents_cap, counts);
  if (rc_dec != RAFTQ_OK) forget_results(h);
  return rc_dec;
}

size_t align256(size_t x) { return (x + 255) / 256 * 256; }
// result area: n records of `rec` bytes, then (16-byte aligned) the {touched count, bad, skipped} tail
size_t tail_off(uint64_t n, uint32_t rec) { return ((size_t)n * rec + 15) / 16 * 16; }

int ensure_slot(raftq_t* h, raftq::StepSlot& sl, uint64_t n, Scratch* s, bool wire = false,
                uint64_t wire_nbytes = 0) {
  if (!h->step_s_in) {
    HIPCHK(h, hipStreamCreateWithFlags(&h->step_s_in, hipStreamNonBlocking));
    HIPCHK(h, hipStreamCreateWithFlags(&h->step_s_out, hipStreamNonBlocking));
    // Stream topology: the H2D DMA on its own stream (overlaps the previous batch's kernels), the result copy on the
    // handle's stream.  Measured on MI355X (profiles/r01/step_pipeline_trace.txt): a kernel that writes to host memory over
    // PCIe keeps every other queue's NEXT kernel from starting until it retires (a kernel that merely spins does not), so a
    // third stream for the D2H buys nothing (176 us per 64K batch; a third stream 186 us, everything on one stream 426 us,
    // copies sharing a stream 459 us).  Round 2 of that A/B (profiles/r01/step_result_copy_ab.txt): the runtime's own D2H
    // memcpy instead of our kernel (382-394 us), the copy split into 2-32 short kernels (177-185 us), the walk writing
    // straight into mapped host memory (186 us) -- none beat this form; those variants are no longer in the code.
    if (const char* m = std::getenv("RAFTQ_STEP_DEFER_COPY")) h->step_defer_copy = std::atoi(m) != 0;
  }
  if (!sl.ev_in) {
    HIPCHK(h, hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&sl.ev_out, hipEventDisableTiming));
  }
  const size_t sort_bytes = raftqk::radix_plan(n).bytes;  // digit counts of the hand-written radix sort (raftq_sort_kernels.hpp)
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
  // the 16-byte {touched count, bad flag} tail sits right behind the result records: one copy moves both
  const size_t o_msgs = carve(n * sizeof(MsgRec)), o_outs = carve(n * sizeof(StepOutRec) + 16), o_ki = carve(n * 8),
               o_ko = carve(n * 8), o_oi = carve(n * 4), o_oo = carve(n * 4), o_sort = carve(sort_bytes), o_next = carve(n * 4),
               o_m40 = carve(n * sizeof(raftqk::Msg40Rec));
  const size_t o_nh = o_outs + tail_off(n, result_rec_bytes(h));
  // decoded entry headers: an entry costs its message two bytes at least, so nbytes / 2 + 1 always suffice
  const uint64_t w_ents_cap = wire ? wire_nbytes / 2 + 1 : 0;
  size_t w_scan_bytes = 0, o_wfr = 0, o_wcnt = 0, o_wbase = 0, o_wbad = 0, o_wents = 0, o_wscan = 0;
  if (wire) {
    w_scan_bytes = scan_sum_scratch_bytes(n + 1);  // tile totals of the hand-written scan (raftq_wire_kernels.hpp)
    o_wfr = carve((n + 1) * 8 + wire_nbytes + 16);
    o_wcnt = carve((n + 1) * 8);
    o_wbase = carve((n + 1) * 8);
    o_wbad = carve(8);
    o_wents = carve(w_ents_cap * sizeof(WireEnt));
    o_wscan = carve(w_scan_bytes);
  }
  // the slot is idle (its previous batch was collected): safe to regrow
  HIPCHK(h, sl.dev.grow(off, std::max(off, (size_t)1 << 20) * 2, &h->stream));
  const size_t out_bytes = (size_t)n * sizeof(StepOutRec) + 16;
  if (out_bytes > sl.out.cap && sl.out.h && h->step_last_out == sl.out.h) forget_results(h);
  HIPCHK(h, sl.out.grow(out_bytes, std::max(out_bytes * 2, (size_t)1 << 20), nullptr));
  uint8_t* base = (uint8_t*)sl.dev.d;
  s->msgs = (MsgRec*)(base + o_msgs);
  s->msgs40 = base + o_m40;
  s->outs = base + o_outs;
  s->keys_in = (uint64_t*)(base + o_ki);
  s->keys_out = (uint64_t*)(base + o_ko);
  s->order_in = (uint32_t*)(base + o_oi);
  s->order_out = (uint32_t*)(base + o_oo);
  s->next = (uint32_t*)(base + o_next);
  s->n_heads = (unsigned long long*)(base + o_nh);
  s->sort_scratch = base + o_sort;
  s->sort_bytes = sort_bytes;
  s->w_off = (uint64_t*)(base + o_wfr);
  s->w_stream = base + o_wfr + (n + 1) * 8;
  s->w_cnt = (uint64_t*)(base + o_wcnt);
  s->w_base = (uint64_t*)(base + o_wbase);
  s->w_bad = (unsigned long long*)(base + o_wbad);
  s->w_ents = (WireEnt*)(base + o_wents);
  s->w_ents_cap = w_ents_cap;
  s->w_scan = base + o_wscan;
  s->w_scan_bytes = w_scan_bytes;
  return RAFTQ_OK;
}

int ensure_slot_staging(raftq_t* h, raftq::StepSlot& sl, uint64_t n, size_t raw_bytes = 0) {
  const size_t bytes = raw_bytes ? raw_bytes : (size_t)std::max<uint64_t>(n, 1) * sizeof(raftq_msg_t);
  HIPCHK(h, sl.in_h.grow(bytes, std::max(bytes * 2, (size_t)1 << 20), nullptr));
  return RAFTQ_OK;
}

// the in-place staging of raftq_step_stage: device memory the host can write (large BAR), else the pinned buffer
int ensure_slot_bar(raftq_t* h, raftq::StepSlot& sl, uint64_t n, void** out, size_t raw_bytes = 0) {
  const size_t bytes = raw_bytes ? raw_bytes : (size_t)std::max<uint64_t>(n, 1) * sizeof(raftq_msg_t);
  if (h->bar.staging) {
    HIPCHK(h, sl.in_bar.grow_bar(bytes, std::max(bytes * 2, (size_t)1 << 20), nullptr, h->bar));
    if (sl.in_bar.h) {
      *out = sl.in_bar.h;
      return RAFTQ_OK;
    }
  }
  if (int rc = ensure_slot_staging(h, sl, n, raw_bytes)) return rc;
  *out = sl.in_h.h;
  return RAFTQ_OK;
}

// raftq_load_node / raftq_read_node: the ABI speaks one flat array per field, the device keeps one record per group.  A
// slab of groups at a time goes through a device temporary and a kernel that writes / reads the field of every record.
int node_fields(raftq_t* h, bool put, uint64_t* term, uint32_t* vote, uint32_t* lead, uint64_t* last_index, uint64_t* last_term) {
  void* host[5] = {term, vote, lead, last_index, last_term};
  const size_t width[5] = {8, 4, 4, 8, 8};
  if (!term && !vote && !lead && !last_index && !last_term) return RAFTQ_OK;
  const uint64_t slab = std::min<uint64_t>(h->G, 1ull << 24);
  void* tmp = nullptr;
  HIPCHK(h, hipMalloc(&tmp, slab * 8));
  int rc = RAFTQ_OK;
  for (int f = 0; f < 5 && rc == RAFTQ_OK; ++f) {
    if (!host[f]) continue;
    for (uint64_t g0 = 0; g0 < h->G && rc == RAFTQ_OK; g0 += slab) {
      const uint64_t cnt = std::min(slab, h->G - g0);
      uint8_t* hp = (uint8_t*)host[f] + g0 * width[f];
      hipError_t e = hipSuccess;
      if (put) e = hipMemcpyAsync(tmp, hp, cnt * width[f], hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) {
        if (put) hipLaunchKernelGGL(node_field_kernel<true>, dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, (NodeRec*)h->node_rec, g0, cnt, f, tmp);
        else hipLaunchKernelGGL(node_field_kernel<false>, dim3((unsigned)((cnt + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, (NodeRec*)h->node_rec, g0, cnt, f, tmp);
        e = hipGetLastError();
      }
      if (e == hipSuccess && !put) e = hipMemcpyAsync(hp, tmp, cnt * width[f], hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // the temporary is reused by the next slab / field
      if (e != hipSuccess) rc = fail(h, RAFTQ_EHIP, std::string("raftq node fields: ") + hipGetErrorString(e));
    }
  }
  (void)hipFree(tmp);
  return rc;
}

}  // namespace

void raftq_detail::free_node_state(raftq_t* h) {
  for (auto& sl : h->step_slot) {
    if (sl.busy && sl.copy_pending && h->stream) (void)hipStreamSynchronize(h->stream);  // its kernels; the copy never ran
    else if (sl.ev_out && sl.busy) (void)hipEventSynchronize(sl.ev_out);
    if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
    if (sl.ev_out) (void)hipEventDestroy(sl.ev_out);
  }
  for (auto& q : h->ld_nowait)
    if (q.ev) (void)hipEventDestroy(q.ev);
  raftq_buf::free_device(h->node_rec, h->step_stall);
}

extern "C" {

int raftq_set_self(raftq_t* h, uint32_t self_peer) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (self_peer >= h->N) return fail(h, RAFTQ_EINVAL, "raftq_set_self: self_peer out of range");
  h->self_peer = self_peer;
  h->self_set = true;
  return raftq_detail::self_max_check(h);  // the sweep's skipped row follows the handle's own slot
}

int raftq_load_node(raftq_t* h, const uint64_t* term, const uint32_t* vote, const uint32_t* lead,
                    const uint64_t* last_index, const uint64_t* last_term) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_load_node")) return rc;
  if (int rc = ensure_node_state(h)) return rc;
  for (uint64_t g = 0; g < h->G; ++g)
    if ((vote && vote[g] > h->N) || (lead && lead[g] > h->N))
      return fail(h, RAFTQ_EINVAL, "raftq_load_node: vote / lead must be 0 (None) or a peer slot + 1");
  if (int rc = node_fields(h, true, const_cast<uint64_t*>(term), const_cast<uint32_t*>(vote), const_cast<uint32_t*>(lead),
                           const_cast<uint64_t*>(last_index), const_cast<uint64_t*>(last_term)))
    return rc;
  return RAFTQ_OK;
}

int raftq_read_node(raftq_t* h, uint64_t* term, uint32_t* vote, uint32_t* lead, uint64_t* last_index,
                    uint64_t* last_term, uint64_t* first_idx_cur_term) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_read_node")) return rc;
  if (int rc = ensure_node_state(h)) return rc;
  if (int rc = node_fields(h, false, term, vote, lead, last_index, last_term)) return rc;
  if (first_idx_cur_term)
    HIPCHK(h, hipMemcpyAsync(first_idx_cur_term, h->first_idx, h->G * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return RAFTQ_OK;
}

int raftq_step_stage(raftq_t* h, uint64_t n, raftq_msg_t** msgs) {
  if (int rc = use_device(h)) return rc;
  if (!msgs) return fail(h, RAFTQ_EINVAL, "raftq_step_stage: null argument");
  const int slot_no = (int)(h->step_submitted % raftq::kStepSlots);
  raftq::StepSlot& sl = h->step_slot[slot_no];  // the slot the next submit will use
  if (sl.busy) return fail(h, RAFTQ_ESTATE, "raftq_step_stage: three batches already in flight; collect one first");
  // a wire batch decoded in place in this slot has its stream in the buffer the producer is about to overwrite
  if (h->step_last_slot == slot_no && sl.w_off_in_place) h->step_last_slot = -1;
  void* p = nullptr;
  if (int rc = ensure_slot_bar(h, sl, n, &p)) return rc;
  *msgs = (raftq_msg_t*)p;
  return RAFTQ_OK;
}

int raftq_step_results(raftq_t* h, const raftq_step_out_t** out, uint64_t* n) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (!out || !n) return fail(h, RAFTQ_EINVAL, "raftq_step_results: null argument");
  if (h->step_last_out && h->step_last_rec != sizeof(StepOutRec))
    return fail(h, RAFTQ_ESTATE, "raftq_step_results: the last batch has compact records (raftq_step_results_c)");
  *out = (const raftq_step_out_t*)h->step_last_out;
  *n = h->step_last_n;
  return RAFTQ_OK;
}

int raftq_step_results_c(raftq_t* h, const raftq_step_out_c_t** out, uint64_t* n) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (!out || !n) return fail(h, RAFTQ_EINVAL, "raftq_step_results_c: null argument");
  if (h->step_last_out && h->step_last_rec != sizeof(StepOutC))
    return fail(h, RAFTQ_ESTATE, "raftq_step_results_c: the last batch has full records (raftq_step_results)");
  *out = (const raftq_step_out_c_t*)h->step_last_out;
  *n = h->step_last_n;
  return RAFTQ_OK;
}

int raftq_step_results_s(raftq_t* h, const raftq_step_out_s_t** out, uint64_t* n) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (!out || !n) return fail(h, RAFTQ_EINVAL, "raftq_step_results_s: null argument");
  if (h->step_last_out && h->step_last_rec != sizeof(raftqk::StepOutS))
    return fail(h, RAFTQ_ESTATE, "raftq_step_results_s: the last batch has records of another format (raftq_step_set_compact)");
  *out = (const raftq_step_out_s_t*)h->step_last_out;
  *n = h->step_last_n;
  return RAFTQ_OK;
}

int raftq_step_set_msg_flags(raftq_t* h, int on) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_step_set_msg_flags")) return rc;
  h->step_msg_flags = on != 0;
  return RAFTQ_OK;
}

int raftq_step_set_voters(raftq_t* h, int on) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_step_set_voters")) return rc;
  if (on != 0 && on != 1) return fail(h, RAFTQ_EINVAL, "raftq_step_set_voters: 0 (a masked handle is refused) or 1 (Step over each group's own voters)");
  h->step_voters = on == 1;
  return RAFTQ_OK;
}

int raftq_step_set_props(raftq_t* h, int on) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_step_set_props")) return rc;
  if (on != 0 && on != 1) return fail(h, RAFTQ_EINVAL, "raftq_step_set_props: 0 (MsgProp is an unknown kind; the frames calls hold it) or 1 (Step takes a forwarded proposal)");
  h->step_props = on == 1;
  return RAFTQ_OK;
}

int raftq_step_set_compact(raftq_t* h, int on) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_step_set_compact")) return rc;
  if (on < 0 || on > 2) return fail(h, RAFTQ_EINVAL, "raftq_step_set_compact: 0 (64-byte records), 1 (40-byte) or 2 (32-byte)");
  h->step_compact = (uint8_t)on;
  forget_results(h);
  return RAFTQ_OK;
}

// One batch into the pipeline.  wire == nullptr: n raftq_msg_t records at msgs.  Otherwise the
// records are decoded on the device from n rafthttp stream frames (raftq_wire.h).
struct WireSrc {
  const void* stream;
  uint64_t nbytes;
  const uint64_t* frame_off;
  // raftq_step_frames: the arrays stay where they are (page-locked), the streaming decoder reads them there, hands the
  // decoded records and entry headers to the caller and keeps a copy of the records in the slot's scratch for Step
  bool frames = false;
  void* msgs_h = nullptr;
  void* ents_h = nullptr;
  uint64_t ents_cap = 0;
  int tail_appends = 0;
  const raftq_detail::PackedDst* packed = nullptr;  // raftq_step_frames_packed: msgs_h is the narrow array
};

// key -> stable radix sort -> walk, on the handle's stream (the path that takes runs of any length)
static int enqueue_sorted_walk(raftq_t* h, const Scratch& s, uint64_t n, int end_bit, uint8_t recs) {
  if (int rc = ensure_mirror(h)) return rc;
  unsigned int* bad = (unsigned int*)(s.n_heads + 1);
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(step_keys_kernel, grid, dim3(kBlock), 0, h->stream, (const MsgRec*)s.msgs, s.keys_in, s.order_in, n,
                     h->G, h->N, bad, h->step_msg_flags, recs, s.outs, h->step_compact, h->step_props, h->cq != nullptr, h->pre_vote, h->lead_transfer, h->read_index != 0);
  HIPCHK(h, hipGetLastError());
  int in_b = 0;  // which pair of buffers the sorted (group, batch position) pairs end up in
  HIPCHK(h, raftqk::radix_sort_pairs(h->stream, s.sort_scratch, s.keys_in, s.order_in, s.keys_out, s.order_out, n, end_bit, &in_b));
  if (h->cq)  // raftq_set_check_quorum: NodeT's CQ form
    launch_walk_cq<NodeArrays, const MsgRec*, const uint64_t*, const uint32_t*, void*, uint8_t, uint64_t, unsigned long long*, const unsigned int*>(
        h, grid, step_cq_kernel, step_cq_voters_kernel, step_cq_lead_kernel, step_cq_lead_voters_kernel, node_arrays(h, recs), s.msgs,
        in_b ? s.keys_out : s.keys_in, in_b ? s.order_out : s.order_in, s.outs, h->step_compact, n, s.n_heads, bad);
  else
    launch_walk(h, grid, step_kernel, step_voters_kernel, step_lead_kernel, step_lead_voters_kernel, node_arrays(h, recs), s.msgs,
                in_b ? s.keys_out : s.keys_in, in_b ? s.order_out : s.order_in, s.outs, h->step_compact, n, s.n_heads, bad);
  HIPCHK(h, hipGetLastError());
  return RAFTQ_OK;
}

// link -> walk (and empty) the per-group lists: two launches, no sort (raftq_step_kernels.hpp 2b / 3b)
static unsigned d2h_blocks(uint64_t quads) { return (unsigned)std::min<uint64_t>(64, (quads + kBlock - 1) / kBlock); }

// `carry`: a slot whose result copy is still pending rides in this batch's walk kernel (nullptr: nothing to carry)
static int enqueue_list_walk(raftq_t* h, const Scratch& s, uint64_t n, uint8_t recs, raftq::StepSlot* carry) {
  if (int rc = ensure_mirror(h)) return rc;
  unsigned int* bad = (unsigned int*)(s.n_heads + 1);
  unsigned int* skipped = bad + 1;  // the last word of the 16-byte tail behind the result records
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  // the carried copy is split over this batch's two kernels roughly as their own durations are (link ~ 1/5 of the chain):
  // 25 per cent of it rides in the link kernel, the rest in the walk kernel
  raftqk::CopyRide in_link{nullptr, nullptr, 0, 0, 0, 0}, in_walk = in_link;
  if (carry) {
    const uint64_t quads = carry->out_quads, cut = quads * 25 / 100;
    in_link = {(const u64x2*)carry->outs_d, (u64x2*)carry->out.d, 0, cut, quads - 1, cut ? d2h_blocks(cut) : 0u};
    in_walk = {(const u64x2*)carry->outs_d, (u64x2*)carry->out.d, cut, quads, quads - 1, d2h_blocks(quads - cut)};
  }
  hipLaunchKernelGGL(step_link_kernel, dim3(blocks + in_link.blocks), dim3(kBlock), 0, h->stream, (const MsgRec*)s.msgs, n, h->G,
                     h->N, h->step_msg_flags, recs, (NodeRec*)h->node_rec, s.next, bad, h->step_stall, s.outs, h->step_compact, in_link, h->step_props, h->cq != nullptr, h->pre_vote, h->lead_transfer, h->read_index != 0);
  HIPCHK(h, hipGetLastError());  // (the link kernel's, before the walk's launch can hide it)
  if (h->cq)  // raftq_set_check_quorum: NodeT's CQ form
    launch_walk_cq<NodeArrays, const MsgRec*, void*, uint8_t, uint64_t, uint64_t, const uint32_t*, unsigned long long*, unsigned int*, const unsigned int*,
                   const unsigned int*, raftqk::CopyRide>(h, dim3(blocks + in_walk.blocks), step_lists_cq_kernel, step_lists_cq_voters_kernel,
                                                          step_lists_cq_lead_kernel, step_lists_cq_lead_voters_kernel, node_arrays(h, recs), s.msgs, s.outs,
                                                          h->step_compact, n, h->G, s.next, s.n_heads, skipped, bad, h->step_stall, in_walk);
  else
    launch_walk(h, dim3(blocks + in_walk.blocks), step_lists_kernel, step_lists_voters_kernel, step_lists_lead_kernel,
                step_lists_lead_voters_kernel, node_arrays(h, recs), s.msgs, s.outs, h->step_compact, n, h->G, s.next, s.n_heads, skipped,
                bad, h->step_stall, in_walk);
  HIPCHK(h, hipGetLastError());
  if (carry) {
    HIPCHK(h, hipEventRecord(carry->ev_out, h->stream));
    carry->copy_pending = false;
  }
  return RAFTQ_OK;
}

// the slot's result records (and tail) -> its pinned host buffer, as a kernel of its own on the handle's stream.  zero_tail: the
// device copy of the tail is left zeroed behind the copy (step_d2h_kernel); whether the slot may count on that (tail_zeroed) is the
// caller's to note
static int enqueue_result_copy(raftq_t* h, raftq::StepSlot& sl, bool zero_tail) {
  hipLaunchKernelGGL(step_d2h_kernel, dim3(d2h_blocks(sl.out_quads)), dim3(kBlock), 0, h->stream, (const u64x2*)sl.outs_d,
                     (u64x2*)sl.out.d, sl.out_quads, zero_tail);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(sl.ev_out, h->stream));
  sl.copy_pending = false;
  return RAFTQ_OK;
}

// Where a batch's input lies when it is submitted.  Everything that differs between the forms follows from this one value: the host
// copy (place_input), the DMA or the in-place routing and the slot's *_in_place fields (enqueue_input), and whether the result copy
// may be deferred (in_device).
enum class Input {
  frames_in_place,  // raftq_step_frames*: page-locked arrays the streaming decoder reads where they lie; nothing is staged
  wire_bar,         // raftq_step_stage_wire's arrays, filled in this slot's device (BAR) staging: the decoder reads them there
  wire_pinned,      // ... filled in this slot's pinned staging: two DMAs (the boundaries and the stream are not adjacent there)
  wire_copied,      // the caller's own arrays, copied into the pinned staging as [frame offsets][stream bytes]: one DMA moves both
  recs_bar_own,     // records filled in this slot's device staging (raftq_step_stage): the kernels read them where they lie
  recs_bar_other,   // records in another slot's device staging (a caller that kept an earlier batch's pointer): device to device
  recs_pinned,      // records in, or copied into, this slot's pinned staging: one DMA
};
static bool in_device(Input where) { return where == Input::wire_bar || where == Input::recs_bar_own || where == Input::recs_bar_other; }

struct Placed {
  Input where;
  size_t in_bytes;         // what a single DMA of the input moves
  const void* device_src;  // the in_device forms: where in device memory the input lies
};

// Submit, phase 2: where the input lies, and for the copied forms the host copy into the slot's pinned staging.
static int place_input(raftq_t* h, raftq::StepSlot& sl, const void* msgs, uint64_t n, const WireSrc* wire, size_t rec_bytes,
                       const char* who, Placed* out) {
  if (wire && wire->frames) {
    *out = {Input::frames_in_place, 0, nullptr};
  } else if (wire) {
    const size_t in_bytes = (size_t)(n + 1) * 8 + (size_t)wire->nbytes;
    const uint8_t* fo = (const uint8_t*)wire->frame_off;
    const uint8_t* sb = (const uint8_t*)wire->stream;
    auto inside = [&](const void* base, size_t cap) {
      const uint8_t* b = (const uint8_t*)base;
      return b && fo == b && sb == b + sl.w_stage_stream_off && sl.w_stage_stream_off >= (size_t)(n + 1) * 8 &&
             sl.w_stage_stream_off + (size_t)wire->nbytes <= cap;
    };
    if (inside(sl.in_bar.h, sl.in_bar.cap)) {
      sl.in_bar.publish();
      *out = {Input::wire_bar, in_bytes, sl.in_bar.h};
    } else if (inside(sl.in_h.h, sl.in_h.cap)) {
      *out = {Input::wire_pinned, in_bytes, nullptr};
    } else {
      if (int rc = ensure_slot_staging(h, sl, n, in_bytes)) return rc;
      std::memcpy(sl.in_h.h, wire->frame_off, (size_t)(n + 1) * 8);
      if (wire->nbytes) std::memcpy((uint8_t*)sl.in_h.h + (size_t)(n + 1) * 8, wire->stream, (size_t)wire->nbytes);
      *out = {Input::wire_copied, in_bytes, nullptr};
    }
  } else {
    const size_t in_bytes = (size_t)n * rec_bytes;
    // unless the caller filled a staging area in place (raftq_step_stage), copy into the pinned one.  Either slot's device staging
    // counts: a caller that keeps filling the buffer raftq_step_stage gave it for an earlier batch must not be served by a host
    // memcpy that READS device memory over the BAR -- 43 ms for 4 MB
    const void* device_src = nullptr;
    for (const raftq::StepSlot& t : h->step_slot)
      if (t.in_bar.holds_in_device(msgs, in_bytes)) device_src = msgs, t.in_bar.publish();
    if (device_src) {
      *out = {sl.in_bar.holds_in_device(device_src, in_bytes) ? Input::recs_bar_own : Input::recs_bar_other, in_bytes, device_src};
    } else {
      if ((const void*)msgs != sl.in_h.h) {
        if (int rc = ensure_slot_staging(h, sl, n)) return rc;
        std::memcpy(sl.in_h.h, msgs, in_bytes);
      } else if (in_bytes > sl.in_h.cap) {
        return fail(h, RAFTQ_EINVAL, std::string(who) + ": more messages than were staged");
      }
      *out = {Input::recs_pinned, in_bytes, nullptr};
    }
  }
  return RAFTQ_OK;
}

// Submit, phase 3: the input onto the device, or the scratch pointers turned to where it already lies.
// Copy-in stream -> the handle's stream (state changes stay ordered with every other call on the handle; the result copy follows the
// compute there), chained by an event.  In: one DMA over PCIe from the pinned staging.  A batch the producer wrote straight into
// device memory needs neither a DMA nor a copy: the kernels read it where it lies (the slot's staging stays untouched until the
// slot's next batch, which is after this one's collect -- the replay path reads it there as well).  Round 2 first kept a
// device-to-device copy into the slot's scratch; with the result copy inside the walk kernel that 3 us blit sat on the critical
// path, held back like every other kernel while a kernel writes to host memory (rocprof: 2.4 .. 75 us).
// *packed_src: where the unpack kernel finds packed records.
static int enqueue_input(raftq_t* h, raftq::StepSlot& sl, Scratch& s, const Placed& in, const WireSrc* wire, uint64_t n, bool packed,
                         const void** packed_src) {
  hipStream_t s_in = h->step_s_in;
  const void* device_src = in.device_src;
  const size_t in_bytes = in.in_bytes;
  void* in_dst = wire ? (void*)s.w_off : packed ? s.msgs40 : (void*)s.msgs;
  sl.msgs_in_place = nullptr;
  sl.w_off_in_place = sl.w_stream_in_place = nullptr;
  *packed_src = s.msgs40;
  switch (in.where) {
    case Input::frames_in_place:  // (the decoder is enqueued in phase 5, on the handle's stream, in front of Step's kernels)
      return RAFTQ_OK;
    case Input::wire_bar:
      s.w_off = (uint64_t*)const_cast<void*>(device_src);
      s.w_stream = (uint8_t*)const_cast<void*>(device_src) + sl.w_stage_stream_off;
      sl.w_off_in_place = s.w_off;
      sl.w_stream_in_place = s.w_stream;
      return RAFTQ_OK;
    case Input::recs_bar_own:
      if (packed) {
        *packed_src = device_src;
      } else {
        s.msgs = (MsgRec*)const_cast<void*>(device_src);
        sl.msgs_in_place = device_src;
      }
      return RAFTQ_OK;
    case Input::wire_pinned:
      HIPCHK(h, hipMemcpyAsync(s.w_off, sl.in_h.h, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s_in));
      if (wire->nbytes)
        HIPCHK(h, hipMemcpyAsync(s.w_stream, (const uint8_t*)sl.in_h.h + sl.w_stage_stream_off, (size_t)wire->nbytes,
                                 hipMemcpyHostToDevice, s_in));
      break;
    case Input::recs_bar_other:
      // that buffer may be handed out again while this batch is in flight, so the records are copied into this slot's scratch
      HIPCHK(h, hipMemcpyAsync(in_dst, device_src, in_bytes, hipMemcpyDeviceToDevice, s_in));
      break;
    case Input::wire_copied:
    case Input::recs_pinned:
      HIPCHK(h, hipMemcpyAsync(in_dst, sl.in_h.h, in_bytes, hipMemcpyHostToDevice, s_in));
      break;
  }
  HIPCHK(h, hipEventRecord(sl.ev_in, s_in));
  HIPCHK(h, hipStreamWaitEvent(h->stream, sl.ev_in, 0));
  return RAFTQ_OK;
}

// Submit, phase 4: the tail behind the result records zeroed, packed records widened.  (packed_src == nullptr: not packed)
static int enqueue_tail_reset_and_unpack(raftq_t* h, raftq::StepSlot& sl, const Scratch& s, uint64_t n, uint32_t rec, bool frames,
                                         const void* packed_src) {
  // touched count + bad + skipped: the default result copy leaves them zeroed behind it (step_d2h_kernel zero_tail)
  // (a frames batch: the decoder that heads the chain zeroes them)
  if (!frames && (!sl.tail_zeroed || sl.tail_n != n || sl.tail_rec != rec || sl.dev.d != sl.tail_dev)) {
    hipLaunchKernelGGL(step_reset_kernel, dim3(1), dim3(64), 0, h->stream, s.n_heads);
    HIPCHK(h, hipGetLastError());
  }
  sl.tail_zeroed = false;
  if (packed_src) {
    hipLaunchKernelGGL(raftqk::step_unpack40_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream,
                       (const raftqk::Msg40Rec*)packed_src, s.msgs, n);
    HIPCHK(h, hipGetLastError());
  }
  return RAFTQ_OK;
}

// Submit, phase 5: a wire batch's frames -> the batch's message records, on the handle's stream in front of Step's kernels.
static int enqueue_decode(raftq_t* h, const Scratch& s, const WireSrc* wire, uint64_t n) {
  if (wire && wire->frames) {
    // one kernel: readers pull boundaries + stream, workers parse, check, flag (RAFTQ_MSGF_*) and push records + entry headers
    // to the caller's arrays and the records once more into this slot's scratch
    return raftq_detail::wire_frames_enqueue(h, wire->stream, wire->nbytes, wire->frame_off, n, wire->msgs_h, wire->ents_h, wire->ents_cap,
                                             s.msgs, wire->tail_appends, s.n_heads, wire->packed);
  }
  if (wire) {
    // frames -> the batch's message records, in HBM: the 64-byte records never cross PCIe.  (s.w_bad only counts
    // malformed frames for raftq_wire_decode's callers; here a malformed frame fails the batch through its flag byte.)
    const dim3 grid1((unsigned)((n + 1 + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(wire_dec_kernel, grid1, dim3(kBlock), 0, h->stream, (const uint8_t*)s.w_stream, wire->nbytes,
                       (const uint64_t*)s.w_off, n, (WireMsg*)s.msgs, s.w_cnt, s.w_bad);
    HIPCHK(h, hipGetLastError());
    // Step reads only the headers.  The entry headers (count -> scan -> second parse) are produced when
    // raftq_step_wire_msgs / _entries first asks for them: fetch_wire below.
  }
  return RAFTQ_OK;
}

// Submit, phase 6: the walk, and with it the result copy of the batch submitted just before this one if that copy was deferred (phase
// 7): it rides in the list walk's kernels, or goes as a kernel of its own in front of the sorted walk.  *lists: which walk it was.
static int enqueue_walk(raftq_t* h, const Scratch& s, uint64_t n, int end_bit, uint8_t recs, bool* lists) {
  // traffic that keeps producing long runs (a few very hot groups) would stall and replay every batch: after two
  // stalls in a row the next 16 batches go straight to the sorted walk, then the list walk is tried again
  if (h->step_sorted_left) --h->step_sorted_left;
  *lists = h->step_walk_mode == 1 && h->step_sorted_left == 0;
  raftq::StepSlot* carry = nullptr;
  if (h->step_submitted > h->step_collected) {
    raftq::StepSlot& prev = h->step_slot[(h->step_submitted - 1) % raftq::kStepSlots];
    if (prev.busy && prev.copy_pending) carry = &prev;
  }
  if (*lists) return enqueue_list_walk(h, s, n, recs, carry);
  if (carry)
    if (int rc = enqueue_result_copy(h, *carry, true)) return rc;
  return enqueue_sorted_walk(h, s, n, end_bit, recs);
}

// Submit, phase 8: what collect, a replay and raftq_step_wire_* need to know of the batch now in flight in the slot.
static void book_slot(raftq_t* h, raftq::StepSlot& sl, const Scratch& s, uint64_t n, const WireSrc* wire, uint8_t recs, uint32_t rec,
                      int end_bit, bool lists) {
  sl.tail_zeroed = true;  // (once the copy has run) holds for the next batch of the same size and format in the same scratch
  sl.tail_n = n;
  sl.tail_rec = rec;
  sl.tail_dev = sl.dev.d;
  sl.n = n;
  sl.busy = true;
  sl.lists = lists;
  sl.replayed = false;
  sl.end_bit = end_bit;
  sl.rec = rec;
  sl.w_nbytes = wire ? wire->nbytes : 0;
  sl.wire = wire != nullptr && !wire->frames;
  sl.recs = recs;
  sl.w_msgs_d = s.msgs;
  sl.w_ents_d = s.w_ents;
  sl.w_ent_total_d = s.w_base + n;
  sl.w_ents_cap = s.w_ents_cap;
  sl.w_msgs_fetched = sl.w_ents_fetched = false;
  sl.w_n_ents = 0;
  h->step_submitted++;
}

// One batch into the pipeline, in eight phases.  rec_bytes: sizeof(raftq_msg_t), or sizeof(raftq_msg40_t) for packed records
// (widened on the device)
static int submit_impl(raftq_t* h, const void* msgs, uint64_t n, const WireSrc* wire, const char* who,
                       size_t rec_bytes = sizeof(raftq_msg_t)) {
  const bool packed = rec_bytes != sizeof(raftq_msg_t);
  const bool frames = wire && wire->frames;
  // 1. refusals, in this order; a refused or failed call applies nothing
  if (int rc = use_device(h)) return rc;
  if (int rc = raftq_detail::refuse_voters(h, who, !h->resp_on, false, h->resp_on)) return rc;  // (raftq_step_frames_respond: raftq_bcast_set_voters' call)
  if (n == 0 || (!wire && !msgs)) return fail(h, RAFTQ_EINVAL, std::string(who) + ": empty batch");
  if (n > 0x7ffffffeull) return fail(h, RAFTQ_EINVAL, std::string(who) + ": batch too large (2^31 - 2 messages at most)");
  if (wire && ((!wire->stream && wire->nbytes) || !wire->frame_off))
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  const int slot_no = (int)(h->step_submitted % raftq::kStepSlots);
  raftq::StepSlot& sl = h->step_slot[slot_no];
  if (sl.busy) return fail(h, RAFTQ_ESTATE, std::string(who) + ": three batches already in flight; collect one first");
  if (int rc = ensure_node_state(h)) return rc;
  if (frames && !h->step_msg_flags)
    return fail(h, RAFTQ_ESTATE, std::string(who) + ": the handle has not opted in to RAFTQ_MSGF_* (raftq_step_set_msg_flags)");
  int end_bit = 1;
  while (end_bit < 64 && (h->G >> end_bit) != 0) ++end_bit;
  const uint8_t recs = frames ? raftqk::kRecsFrames : wire ? raftqk::kRecsWire : raftqk::kRecsCaller;
  const uint32_t rec = result_rec_bytes(h);
  // 2. input placement, host side
  Placed in;
  if (int rc = place_input(h, sl, msgs, n, wire, rec_bytes, who, &in)) return rc;
  if (h->step_last_slot == slot_no) h->step_last_slot = -1;  // that batch's decoded records are about to be overwritten
  sl.wire = false;
  Scratch s;
  if (int rc = ensure_slot(h, sl, n, &s, wire != nullptr && !frames, wire && !frames ? wire->nbytes : 0)) return rc;
  // Step moves the live commit index: a what-if (NO_ADOPT) sweep's shadow values are no longer what
  // raftq_read_committed should hand out
  h->last_flags &= ~RAFTQ_SWEEP_NO_ADOPT;
  // 3. input enqueue   4. tail reset and unpack   5. decode   6. walk, with the carried copy
  const void* packed_src = nullptr;
  bool lists = false;
  if (int rc = enqueue_input(h, sl, s, in, wire, n, packed, &packed_src)) return rc;
  if (int rc = enqueue_tail_reset_and_unpack(h, sl, s, n, rec, frames, packed ? packed_src : nullptr)) return rc;
  if (int rc = enqueue_decode(h, s, wire, n)) return rc;
  if (int rc = enqueue_walk(h, s, n, end_bit, recs, &lists)) return rc;
  // 7. own copy or defer.  With everything on the handle's stream (the default topology) a batch's copy is DEFERRED: it rides in
  // the walk kernel of the batch submitted behind it (phase 6 of that submit), or is launched by its own collect if none is.
  // Only for batches that arrived in device memory (raftq_step_stage behind a large BAR): a batch that needs an inbound
  // DMA is better off with its own copy kernel -- the DMA of the batch after next cannot start while a kernel is writing
  // to host memory either, and the fused kernel writes for longer (measured: caller-owned arrays 157 us per batch with
  // their own copy kernels, 189 us deferred; staged batches 101 -> 77 us; profiles/r02/step_deferred_copy_ab.txt).
  sl.outs_d = s.outs;
  sl.out_quads = tail_off(n, rec) / 16 + 1;  // records + the 16-byte tail
  if (h->step_defer_copy && in_device(in.where)) {
    sl.copy_pending = true;
  } else if (int rc = enqueue_result_copy(h, sl, true)) {
    return rc;
  }
  // 8. slot bookkeeping
  book_slot(h, sl, s, n, wire, recs, rec, end_bit, lists);
  return RAFTQ_OK;
}

int raftq_step_submit(raftq_t* h, const raftq_msg_t* msgs, uint64_t n) {
  return submit_impl(h, msgs, n, nullptr, "raftq_step_submit");
}

int raftq_step_stage_packed(raftq_t* h, uint64_t n, raftq_msg40_t** msgs) {
  static_assert(sizeof(raftq_msg40_t) == sizeof(raftqk::Msg40Rec), "ABI struct mismatch");
  return raftq_step_stage(h, n, (raftq_msg_t**)msgs);  // a staging area for n 64-byte records holds n packed ones
}

int raftq_step_submit_packed(raftq_t* h, const raftq_msg40_t* msgs, uint64_t n) {
  if (h && h->G > 0x100000000ull) return fail(h, RAFTQ_EINVAL, "raftq_step_submit_packed: group ids of this handle do not fit 32 bits");
  return submit_impl(h, msgs, n, nullptr, "raftq_step_submit_packed", sizeof(raftq_msg40_t));
}

int raftq_step_stage_wire(raftq_t* h, uint64_t n_cap, uint64_t nbytes_cap, uint64_t** frame_off, void** stream) {
  if (int rc = use_device(h)) return rc;
  if (!frame_off || !stream) return fail(h, RAFTQ_EINVAL, "raftq_step_stage_wire: null argument");
  const int slot_no = (int)(h->step_submitted % raftq::kStepSlots);
  raftq::StepSlot& sl = h->step_slot[slot_no];  // the slot the next submit will use
  if (sl.busy) return fail(h, RAFTQ_ESTATE, "raftq_step_stage_wire: three batches already in flight; collect one first");
  // the slot's previous batch may still be the one raftq_step_wire_msgs / _entries would parse entries for -- from the
  // very bytes the producer is about to overwrite
  if (h->step_last_slot == slot_no) h->step_last_slot = -1;
  const size_t off_bytes = align256((size_t)(n_cap + 1) * 8);
  void* p = nullptr;
  if (int rc = ensure_slot_bar(h, sl, n_cap, &p, off_bytes + (size_t)nbytes_cap + 16)) return rc;
  sl.w_stage_stream_off = off_bytes;
  *frame_off = (uint64_t*)p;
  *stream = (uint8_t*)p + off_bytes;
  return RAFTQ_OK;
}

int raftq_step_submit_wire(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n) {
  const WireSrc w = {stream, nbytes, frame_off};
  return submit_impl(h, nullptr, n, &w, "raftq_step_submit_wire");
}

// the decoded records of the last collected batch, fetched from its slot on demand
static int fetch_wire(raftq_t* h, bool want_ents, const char* who, raftq::StepSlot** out) {
  if (int rc = use_device(h)) return rc;
  if (h->step_last_slot < 0 || !h->step_slot[h->step_last_slot].wire)
    return fail(h, RAFTQ_ESTATE, std::string(who) + ": the last collected batch was not submitted from the wire "
                                                      "(or its slot has been reused)");
  raftq::StepSlot& sl = h->step_slot[h->step_last_slot];
  const size_t msg_bytes = (size_t)sl.n * sizeof(WireMsg);
  hipStream_t st = h->step_s_out;  // not behind whatever batch is in flight on the handle's stream
  if (!sl.w_msgs_fetched) {
    // first request for this batch: the decoder's second pass (entry counts -> exclusive scan -> entry headers in
    // message order, ent_first of every message), kept out of the Step chain because Step does not need it
    Scratch s;
    if (int rc = ensure_slot(h, sl, sl.n, &s, true, sl.w_nbytes)) return rc;
    if (sl.w_off_in_place) {  // the batch was decoded where the producer wrote it; so are its entries
      s.w_off = (uint64_t*)const_cast<void*>(sl.w_off_in_place);
      s.w_stream = (uint8_t*)const_cast<void*>(sl.w_stream_in_place);
    }
    HIPCHK(h, exclusive_sum_u64((const uint64_t*)s.w_cnt, s.w_base, sl.n + 1, (uint64_t*)s.w_scan, st));
    hipLaunchKernelGGL(wire_dec_ents_kernel, dim3((unsigned)((sl.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       (const uint8_t*)s.w_stream, sl.w_nbytes, (const uint64_t*)s.w_off, sl.n, (WireMsg*)s.msgs,
                       (const uint64_t*)s.w_base, s.w_ents, s.w_ents_cap);
    HIPCHK(h, hipGetLastError());
    // learn the entry count, size the pinned block for both arrays (so a pointer handed out for the messages
    // stays valid when the entries are asked for later)
    uint64_t total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, sl.w_ent_total_d, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (total > sl.w_ents_cap) total = sl.w_ents_cap;  // cannot happen: the cap is the worst case
    const size_t need = align256(msg_bytes) + (size_t)total * sizeof(WireEnt);
    HIPCHK(h, sl.w_pin.grow(need, std::max(need * 2, (size_t)1 << 20), nullptr));
    HIPCHK(h, hipMemcpyAsync(sl.w_pin.h, sl.w_msgs_d, msg_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    sl.w_n_ents = total;
    sl.w_msgs_fetched = true;
  }
  if (want_ents && !sl.w_ents_fetched) {
    if (sl.w_n_ents) {
      HIPCHK(h, hipMemcpyAsync((uint8_t*)sl.w_pin.h + align256(msg_bytes), sl.w_ents_d,
                               (size_t)sl.w_n_ents * sizeof(WireEnt), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
    }
    sl.w_ents_fetched = true;
  }
  *out = &sl;
  return RAFTQ_OK;
}

int raftq_step_wire_msgs(raftq_t* h, const raftq_wire_msg_t** msgs, uint64_t* n) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (!msgs || !n) return fail(h, RAFTQ_EINVAL, "raftq_step_wire_msgs: null argument");
  raftq::StepSlot* sl = nullptr;
  if (int rc = fetch_wire(h, false, "raftq_step_wire_msgs", &sl)) return rc;
  *msgs = (const raftq_wire_msg_t*)sl->w_pin.h;
  *n = sl->n;
  return RAFTQ_OK;
}

int raftq_step_wire_entries(raftq_t* h, const raftq_wire_ent_t** ents, uint64_t* n_ents) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (!ents || !n_ents) return fail(h, RAFTQ_EINVAL, "raftq_step_wire_entries: null argument");
  raftq::StepSlot* sl = nullptr;
  if (int rc = fetch_wire(h, true, "raftq_step_wire_entries", &sl)) return rc;
  *ents = (const raftq_wire_ent_t*)((const uint8_t*)sl->w_pin.h + align256((size_t)sl->n * sizeof(WireMsg)));
  *n_ents = sl->w_n_ents;
  return RAFTQ_OK;
}

// batch `first` (already taken out of flight by its collect) reported `skipped`; the batches submitted behind it are
// still in flight and were skipped as well: all of them go through the sorted walk again, in submission order
static int replay_stalled(raftq_t* h, uint64_t first) {
  for (uint64_t b = first; b < h->step_submitted; ++b) {
    raftq::StepSlot& sl = h->step_slot[b % raftq::kStepSlots];
    if (b != first) {
      if (!sl.busy) break;
      // its copy, if one was enqueued (it rode in the batch behind it), must be over before the replay's own lands in
      // the same host buffer; a pending one is simply replaced by the replay's
      if (!sl.copy_pending) HIPCHK(h, hipEventSynchronize(sl.ev_out));
    }
    Scratch s;
    if (int rc = ensure_slot(h, sl, sl.n, &s, sl.wire, sl.w_nbytes)) return rc;
    if (sl.msgs_in_place) s.msgs = (MsgRec*)const_cast<void*>(sl.msgs_in_place);
    hipLaunchKernelGGL(step_reset_kernel, dim3(1), dim3(64), 0, h->stream, s.n_heads);
    if (int rc = enqueue_sorted_walk(h, s, sl.n, sl.end_bit, sl.recs)) return rc;
    sl.outs_d = s.outs;
    sl.out_quads = tail_off(sl.n, sl.rec) / 16 + 1;
    if (int rc = enqueue_result_copy(h, sl, /*zero_tail=*/false)) return rc;  // (the tail stays: no batch may count on a zeroed one)
    sl.tail_zeroed = false;
    sl.replayed = true;
    h->step_replays++;
  }
  HIPCHK(h, hipMemsetAsync(h->step_stall, 0, 4, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return RAFTQ_OK;
}

int raftq_step_collect(raftq_t* h, raftq_step_out_t* out, raftq_step_counts_t* counts) {
  if (int rc = use_device(h)) return rc;
  if (counts) counts->n_msgs = counts->n_groups_touched = 0;
  if (h->step_collected == h->step_submitted) return fail(h, RAFTQ_ESTATE, "raftq_step_collect: nothing in flight");
  raftq::StepSlot& sl = h->step_slot[h->step_collected % raftq::kStepSlots];
  if (sl.copy_pending)  // nothing was submitted behind this batch: its results leave now
    if (int rc = enqueue_result_copy(h, sl, true)) return rc;
  HIPCHK(h, hipEventSynchronize(sl.ev_out));
  sl.busy = false;
  h->step_last_slot = (int)(h->step_collected % raftq::kStepSlots);
  h->step_collected++;
  const uint64_t n = sl.n;
  const uint8_t* tail = (const uint8_t*)sl.out.h + tail_off(n, sl.rec);
  unsigned long long heads;
  unsigned int bad_h, skipped_h;
  std::memcpy(&skipped_h, tail + 12, 4);
  if (skipped_h) {
    // this batch has a run longer than the list walk takes: nothing of it, nor of the batch submitted behind it,
    // was applied.  Replay them in submission order through the sorted walk, then let the list walk resume.
    if (int rc = replay_stalled(h, h->step_collected - 1)) return rc;
    if (++h->step_stalls_in_a_row >= 2) h->step_sorted_left = 16;
  } else if (sl.lists && !sl.replayed) {
    h->step_stalls_in_a_row = 0;
  }
  std::memcpy(&heads, tail, 8);
  std::memcpy(&bad_h, tail + 8, 4);
  if (bad_h) {
    forget_results(h);
    return fail(h, RAFTQ_EINVAL,
                "raftq_step: a message is malformed (group or from out of range, or a type Step does not take); "
                "nothing of that batch was applied");
  }
  h->step_last_out = sl.out.h;
  h->step_last_n = n;
  h->step_last_rec = sl.rec;
  if (out) {
    if (sl.rec != sizeof(StepOutRec))
      return fail(h, RAFTQ_EINVAL, "raftq_step_collect: compact result records are read in place (raftq_step_results_c), pass out = NULL");
    std::memcpy(out, sl.out.h, (size_t)n * sizeof(StepOutRec));
  }
  if (counts) {
    counts->n_msgs = n;
    counts->n_groups_touched = heads;
  }
  return RAFTQ_OK;
}

int raftq_step_batch(raftq_t* h, const raftq_msg_t* msgs, uint64_t n, raftq_step_out_t* out,
                     raftq_step_counts_t* counts) {
  if (int rc = one_call_open(h, "raftq_step_batch", [&] { if (counts) counts->n_msgs = counts->n_groups_touched = 0; })) return rc;
  if (n == 0) return RAFTQ_OK;
  if (!msgs) return fail(h, RAFTQ_EINVAL, "raftq_step_batch: null messages");
  if (out && h->step_compact)
    return fail(h, RAFTQ_EINVAL, "raftq_step_batch: compact result records are read in place (raftq_step_results_c), pass out = NULL");
  if (int rc = raftq_step_submit(h, msgs, n)) return rc;
  return raftq_step_collect(h, out, counts);
}

int raftq_step_frames(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, int tail_appends,
                      raftq_wire_msg_t* msgs, raftq_wire_ent_t* ents, uint64_t ents_cap, raftq_wire_counts_t* counts) {
  if (int rc = one_call_open(h, "raftq_step_frames", [&] { if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0}; })) return rc;
  if (n == 0) return RAFTQ_OK;
  if ((!stream && nbytes) || !frame_off || !msgs) return fail(h, RAFTQ_EINVAL, "raftq_step_frames: null argument");
  WireSrc w{stream, nbytes, frame_off, true, msgs, ents, ents ? ents_cap : 0, tail_appends};
  if (int rc = submit_impl(h, nullptr, n, &w, "raftq_step_frames")) return rc;
  // one wait: the result copy is the last kernel of the chain the decoder heads
  const int rc_step = raftq_step_collect(h, nullptr, nullptr);
  if (int rc = frames_close(h, frame_off, n, ents != nullptr, ents_cap, counts)) return rc;
  return rc_step;
}

int raftq_step_frames_packed(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, int tail_appends, int form,
                             uint32_t head_types, void* narrow, raftq_wire_msg_t* wide, uint64_t wide_cap, raftq_wire_ent_t* ents, uint64_t ents_cap,
                             raftq_wire_counts_t* counts, uint64_t* n_wide) {
  const char* who = "raftq_step_frames_packed";
  auto zero_counts = [&] {
    if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
    if (n_wide) *n_wide = 0;
  };
  if (int rc = one_call_open(h, who, zero_counts)) return rc;
  if (form != RAFTQ_WIRE_FORM_40 && form != RAFTQ_WIRE_FORM_HEAD)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": form is neither RAFTQ_WIRE_FORM_40 nor RAFTQ_WIRE_FORM_HEAD");
  if (h->self_peer >= 255) return fail(h, RAFTQ_EINVAL, std::string(who) + ": the handle's own slot must be a peer slot (< 255)");
  if (n == 0) return RAFTQ_OK;
  if ((!stream && nbytes) || !frame_off || !narrow || (wide_cap && !wide)) return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  const raftq_detail::PackedDst pd{form, head_types, wide, wide_cap};
  WireSrc w{stream, nbytes, frame_off, true, narrow, ents, ents ? ents_cap : 0, tail_appends, &pd};
  if (int rc = submit_impl(h, nullptr, n, &w, who)) return rc;
  // one wait, as raftq_step_frames
  const int rc_step = raftq_step_collect(h, nullptr, nullptr);
  if (int rc = frames_close(h, frame_off, n, ents != nullptr, ents_cap, counts)) return rc;
  if (n_wide) *n_wide = raftq_detail::wire_frames_n_wide(h);  // more than wide_cap is no error here: the frames have been stepped
  return rc_step;
}

int raftq_step_frames_respond(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, int tail_appends,
                              raftq_wire_msg_t* msgs, raftq_wire_ent_t* ents, uint64_t ents_cap, const uint64_t* at_tail, void* out, uint64_t cap,
                              uint64_t* resp_off, uint64_t* peer_off, raftq_wire_counts_t* counts, raftq_wire_counts_t* resp_counts) {
  const char* who = "raftq_step_frames_respond";
  auto zero_counts = [&] {
    if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
    if (resp_counts) *resp_counts = raftq_wire_counts_t{0, 0, 0, 0};
  };
  if (int rc = one_call_open(h, who, zero_counts)) return rc;
  if (!peer_off) return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  if (n == 0) {
    for (uint32_t p = 0; p <= h->N; ++p) peer_off[p] = 0;
    if (resp_off) resp_off[0] = 0;
    return RAFTQ_OK;
  }
  if ((!stream && nbytes) || !frame_off || !msgs || !out) return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  if (!h->step_msg_flags)
    return fail(h, RAFTQ_ESTATE, std::string(who) + ": the handle has not opted in to RAFTQ_MSGF_* (raftq_step_set_msg_flags)");
  if (h->N < 2) return fail(h, RAFTQ_EINVAL, std::string(who) + ": a single-peer group has nobody to answer -- use raftq_step_frames");
  // the exact worst case: every result a commit broadcast (N - 1 frames) of RAFTQ_RESPOND_FRAME_MAX bytes -- refused before
  // anything runs, so a call that has stepped never fails for output space.  With raftq_respond_set_lead on every result may be
  // becomeLeader's broadcast instead, whose frames carry the empty entry: RAFTQ_RESPOND_LEAD_FRAME_MAX
  const uint64_t n_max = n * (h->N - 1);
  const uint64_t frame_max = h->resp_lead ? RAFTQ_RESPOND_LEAD_FRAME_MAX : RAFTQ_RESPOND_FRAME_MAX;
  const char* frame_max_name = h->resp_lead ? "RAFTQ_RESPOND_LEAD_FRAME_MAX" : "RAFTQ_RESPOND_FRAME_MAX";
  if (n_max > 0x7ffffffeull || n_max > (((uint64_t)1 << 31) / frame_max))
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": batch too large (n * (N - 1) * " + frame_max_name + " must stay within 2^31 bytes)");
  if (cap < n_max * frame_max)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": cap is below n * (N - 1) * " + frame_max_name + " = " +
                                     std::to_string(n_max * frame_max) + " bytes -- nothing was applied");
  // raftq_respond_set_props: every entry of the batch may go out again to every peer -- its payload (all of them lie inside the
  // stream) and at most RAFTQ_RESPOND_ENT_MAX bytes around it; the device stamps the decoder's headers, so there must be some
  if (h->resp_props) {
    if (!ents) return fail(h, RAFTQ_EINVAL, std::string(who) + ": raftq_respond_set_props needs ents (the device stamps the decoder's entry headers) -- nothing was applied");
    const uint64_t per_peer = nbytes + (ents_cap > ((uint64_t)1 << 31) ? (uint64_t)1 << 40 : ents_cap * RAFTQ_RESPOND_ENT_MAX);
    const uint64_t bound = n_max * frame_max + (h->N - 1) * per_peer;
    if (bound > ((uint64_t)1 << 31))
      return fail(h, RAFTQ_EINVAL, std::string(who) + ": batch too large (n * (N - 1) * " + frame_max_name +
                                       " + (N - 1) * (nbytes + ents_cap * RAFTQ_RESPOND_ENT_MAX) must stay within 2^31 bytes)");
    if (cap < bound)
      return fail(h, RAFTQ_EINVAL, std::string(who) + ": cap is below n * (N - 1) * " + frame_max_name + " + (N - 1) * (nbytes + ents_cap * RAFTQ_RESPOND_ENT_MAX) = " +
                                       std::to_string(bound) + " bytes -- nothing was applied");
  }
  raftq_detail::RespPlan rp;
  if (int rc = raftq_detail::respond_prepare(h, stream, nbytes, frame_off, msgs, ents, ents_cap, at_tail, out, cap, resp_off, peer_off, n, &rp)) return rc;
  // from here on: raftq_step_frames, with the walks answering (node_arrays), then the layout and the marshal behind them
  h->resp_on = true;
  WireSrc w{stream, nbytes, frame_off, true, msgs, ents, ents ? ents_cap : 0, tail_appends};
  int rc = submit_impl(h, nullptr, n, &w, who);
  if (rc == RAFTQ_OK) rc = raftq_detail::respond_enqueue(h, rp);
  if (rc != RAFTQ_OK) {
    h->resp_on = false;
    return rc;
  }
  // one wait for the decode, the walk, the result copy, the layout and the marshal
  if (hipError_t e = raftq_detail::wait_call(h); e != hipSuccess) {
    h->resp_on = false;
    return fail(h, RAFTQ_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  const uint64_t replays = h->step_replays;
  int rc_step = raftq_step_collect(h, nullptr, nullptr);
  // a stalled batch (a run longer than the list walk takes) was applied by the collect's replay (its own wait): its answers are
  // laid out and marshalled again (a third) -- the first pass, which found nothing answered, must not have given up either
  if (rc_step == RAFTQ_OK && h->step_replays != replays) {
    rc_step = raftq_detail::respond_pass_ok(h);
    if (rc_step == RAFTQ_OK) rc_step = raftq_detail::respond_enqueue(h, rp);
    if (rc_step == RAFTQ_OK && raftq_detail::wait_call(h) != hipSuccess) rc_step = fail(h, RAFTQ_EHIP, std::string(who) + ": the replay's marshal failed");
  }
  h->resp_on = false;
  if (int rc = frames_close(h, frame_off, n, ents != nullptr, ents_cap, counts)) return rc;
  if (rc_step != RAFTQ_OK) return rc_step;
  return raftq_detail::respond_finish(h, rp, resp_counts);
}

// wait = false (raftq_apply_log_deltas_nowait): the same kernels from a staging area of their own, enqueued and left
static int log_deltas_impl(raftq_t* h, const raftq_log_delta_t* d, uint64_t n, uint64_t* committed_out, bool wait) {
  if (int rc = raftq_detail::use_device_idle(h, wait ? "raftq_apply_log_deltas" : "raftq_apply_log_deltas_nowait")) return rc;
  if (int rc = raftq_detail::refuse_voters(h, wait ? "raftq_apply_log_deltas" : "raftq_apply_log_deltas_nowait", true)) return rc;
  if (n == 0) return RAFTQ_OK;
  if (!d) return fail(h, RAFTQ_EINVAL, "raftq_apply_log_deltas: null argument");
  for (uint64_t i = 0; i < n; ++i)
    if (d[i].group >= h->G) return fail(h, RAFTQ_EINVAL, "a log delta is out of range; nothing applied");
  if (int rc = ensure_node_state(h)) return rc;
  if (int rc = ensure_mirror(h)) return rc;
  const size_t off_out = align256((size_t)n * sizeof(raftq_log_delta_t));
  if (n > 0xfffffffeull) return fail(h, RAFTQ_EINVAL, "raftq_apply_log_deltas: batch too large (n must fit 32 bits)");
  void *stage_h = nullptr, *stage_d = nullptr;
  hipEvent_t stage_ev = nullptr;
  if (wait) {
    if (int rc = ensure_staging(h, off_out + (size_t)n * 8)) return rc;
    stage_h = h->stage.h;
    stage_d = h->stage.d;
  } else {
    // two pinned areas taken in turn: the host may not write into one before the kernels that read it have run -- which they
    // have, two calls later, in anything but a pathological queue (the event says so)
    raftq_t::LdNowait& q = h->ld_nowait[h->ld_nowait_next++ & 1];
    if (q.ev) HIPCHK(h, hipEventSynchronize(q.ev));
    else HIPCHK(h, hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
    const size_t need = (size_t)n * sizeof(raftq_log_delta_t);
    HIPCHK(h, q.buf.grow(need, std::max(need * 2, (size_t)1 << 16), nullptr));  // (its event has been waited for)
    stage_h = q.buf.h;
    stage_d = q.buf.d;
    stage_ev = q.ev;
  }
  // records of one group apply in order: the k-th record of a group goes into launch k (raftq_step_rounds.hpp).  The common batch
  // names every group once: one launch, caller order
  uint32_t n_rounds = 1;
  try {  // a bad_alloc must not cross the extern "C" boundary
    n_rounds = raftq_rounds::plan(h->G, n, [d](uint64_t i) { return d[i].group; }, h->ld_mark, h->ld_epoch, h->ld_round, h->ld_start, h->ld_pos);
  } catch (...) {
    return fail(h, RAFTQ_ENOMEM, "raftq_apply_log_deltas: host allocation failed");
  }
  const uint64_t whole[2] = {0, n};
  const uint64_t* round_start = n_rounds == 1 ? whole : h->ld_start.data();  // staged position where round r begins (+ the end)
  const uint32_t* pos_of = n_rounds == 1 ? nullptr : h->ld_pos.data();       // pos_of[staged position] = caller's index
  h->last_flags &= ~RAFTQ_SWEEP_NO_ADOPT;  // as in raftq_step_submit: the live commit index moves
  raftq_log_delta_t* dst = (raftq_log_delta_t*)stage_h;
  uint64_t* out_h = (uint64_t*)((uint8_t*)stage_h + off_out);
  uint64_t* out_d = (uint64_t*)((uint8_t*)stage_d + off_out);
  if (!pos_of) std::memcpy(dst, d, (size_t)n * sizeof(raftq_log_delta_t));
  else
    for (uint64_t k = 0; k < n; ++k) dst[k] = d[pos_of[k]];
  for (uint32_t r = 0; r < n_rounds; ++r) {
    const uint64_t start = round_start[r], m = round_start[r + 1] - start;
    if (m == 0) continue;
    launch_walk(h, dim3((unsigned)((m + kBlock - 1) / kBlock)), log_deltas_kernel, log_deltas_voters_kernel, nullptr, nullptr, node_arrays(h),
                (const LogDeltaRec*)stage_d + start, m, committed_out ? out_d + start : nullptr);
    HIPCHK(h, hipGetLastError());
  }
  if (!wait) {
    HIPCHK(h, hipEventRecord(stage_ev, h->stream));
    return RAFTQ_OK;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (committed_out && !pos_of) std::memcpy(committed_out, out_h, (size_t)n * 8);
  else if (committed_out)
    for (uint64_t k = 0; k < n; ++k) committed_out[pos_of[k]] = out_h[k];
  return RAFTQ_OK;
}

int raftq_apply_log_deltas(raftq_t* h, const raftq_log_delta_t* d, uint64_t n, uint64_t* committed_out) {
  return log_deltas_impl(h, d, n, committed_out, true);
}

int raftq_apply_log_deltas_nowait(raftq_t* h, const raftq_log_delta_t* d, uint64_t n) {
  return log_deltas_impl(h, d, n, nullptr, false);
}

}  // extern "C"
