// raftq_tick_voters_block.inc -- one 1,024-group block of the Tick with promotable(): the statements of a kernel's body, in scope
// `a` (TickArgs), `voters` (const uint16_t*, [ld]) and `self` (uint32_t).  Included TWICE by raftq_kernels.hpp:
//   tick_voters_kernel (one handle per launch)   token for token what it was before the set form
//   tick_set_voters_kernel (a set per launch)    behind the member's table entry
// The includer sets RAFTQ_TV_MASKS(at): the lane's four masks, voters[at .. at + 4), as one u64 -- the set form answers all-ones
// for a member whose mask pointer is null (`mine` true everywhere: tick_kernel's arithmetic).  An include and not a called body
// for raftq_sweep_voters_tile.inc's reason: tick_voters_kernel keeps its assembly.
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t key = tick_key(a.seed, a.tick_no);  // wave-uniform
  const uint64_t blk = blockIdx.x;
  const uint64_t g = (blk * kBlock + tid) * 4;
  const uint32_t roles = ldg<false>(reinterpret_cast<const uint32_t*>(a.role + g));
  const u32x4 el = ldg<false>(reinterpret_cast<const u32x4*>(a.elapsed + g));
  const uint64_t vm = RAFTQ_TV_MASKS(g);  // (padding groups hold 0: they never act anyway)
  uint32_t e[4] = {el.x, el.y, el.z, el.w};
  uint32_t acts = 0;
  uint32_t n_hup = 0, n_beat = 0;  // wave-uniform
  uint64_t hb[4], bb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t role = (roles >> (8 * k)) & 0xffu;
    const bool valid = g + k < a.n_groups;
    const bool mine = (((uint32_t)(vm >> (16 * k)) >> self) & 1u) != 0;
    const bool idle = role != 2u && !mine;  // tickElection: `if !r.promotable() { r.elapsed = 0; return }`
    uint32_t v = e[k] + 1;
    const bool beat = role == 2u && v >= a.heartbeat_tick;
    const int64_t d = (int64_t)v - (int64_t)a.election_tick;
    bool hup = role != 2u && mine && d >= 0;
    if (__ballot(hup) != 0) hup = hup && d > (int64_t)tick_mod(tick_rand(key, (uint32_t)g + k), a.election_tick, a.et_magic);
    const uint32_t act = !valid ? 0u : (hup ? 1u : (beat ? 2u : 0u));
    e[k] = !valid ? e[k] : ((act || idle) ? 0u : v);
    acts |= act << (8 * k);
    hb[k] = __ballot(act == 1u);
    bb[k] = __ballot(act == 2u);
    n_hup += __popcll(hb[k]);
    n_beat += __popcll(bb[k]);
  }
  u32x4 out;
  out.x = e[0]; out.y = e[1]; out.z = e[2]; out.w = e[3];
  stg<false>(reinterpret_cast<u32x4*>(a.elapsed + g), out);
  stg<false>(reinterpret_cast<uint32_t*>(a.action + g), acts);
  tick_chunk_out(a, blk * kWaves + wave, lane, hb, bb, n_hup, n_beat);
