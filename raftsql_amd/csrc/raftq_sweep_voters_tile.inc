// raftq_sweep_voters_tile.inc -- one tile of the masked sweep: the statements of a function body, from the tile's constants to the
// per-wave partials.  Included TWICE by raftq_kernels.hpp, inside a function template over <N, GPL, COMMIT, GATED, VOTES, POLICY>:
//   sweep_voters_kernel (one handle per launch)      token for token what it was before the set form
//   sweep_set_voters_kernel (a set per launch)       the same tile for a member of a set, masks loaded or not
// The includer sets
//   RAFTQ_VT_PROLOGUE       the statements that name `a` (const SweepArgs&), `tid` and `tile` (the set form fetches its masks here)
//   RAFTQ_VT_VMASK(at)      the eight masks of the vote lane's eight groups, voters[at .. at + 8), as a u32x4p
//   RAFTQ_VT_CMASK(j, at)   round j: the two masks of the commit lane's pair, voters[at], voters[at + 1], as one dword
// Why an include and not a body both kernels call: raftq_step_walk_kernels.inc says it -- a called body is simplified before it
// meets the kernel, and sweep_voters_kernel came out with other assembly in all 135 instantiations (tools/isa_unchanged.py,
// profiles/r16/README.md).
  constexpr bool NT = (POLICY & kLdNT) != 0;
  constexpr bool STNT = (POLICY & kStNT) != 0;
  constexpr int kTile = kBlock * GPL;
  constexpr int kRounds = GPL / 2;
  constexpr int kVoteLanes = kTile / 8;
  RAFTQ_VT_PROLOGUE
  const uint64_t tile0 = (uint64_t)tile * kTile;
  const bool vote_lane = VOTES && tid < kVoteLanes;  // wave-uniform (kVoteLanes % 64 == 0)

  TileRegs<N, GPL, COMMIT, GATED, VOTES> r;
  u32x4p vmask;                          // the 8 masks of the vote lane's 8 groups
  uint32_t cmask[COMMIT ? kRounds : 1];  // the 2 masks of the lane's pair, per round
  if constexpr (VOTES) {
    if (vote_lane) vmask = RAFTQ_VT_VMASK(tile0 + 8ull * tid);
  }
  tile_load<N, GPL, COMMIT, GATED, VOTES, POLICY>(r, a, tile);  // every row: r.skip stays 0
  if constexpr (COMMIT) {
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
      const uint64_t g = tile0 + (uint64_t)(tid >> 6) * (64 * GPL) + (uint64_t)j * 128 + 2 * (tid & 63);
      cmask[j] = RAFTQ_VT_CMASK(j, g);
    }
  }

  uint32_t n_changed = 0;  // wave-uniform
  uint32_t won_lost = 0;   // per lane: won | lost << 16
  if constexpr (COMMIT) {
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
      const uint64_t g = tile0 + (uint64_t)(tid >> 6) * (64 * GPL) + (uint64_t)j * 128 + 2 * (tid & 63);
      uint64_t v0[N], v1[N];
#pragma unroll
      for (int p = 0; p < N; ++p) {
        v0[p] = r.m[j][p].x;
        v1[p] = r.m[j][p].y;
      }
      const uint64_t mci0 = select_quorum_voters<N>(v0, cmask[j] & 0xffffu);
      const uint64_t mci1 = select_quorum_voters<N>(v1, cmask[j] >> 16);
      u64x2 o;
      o.x = maybe_commit<GATED>(mci0, r.c[j].x, GATED ? r.f[j].x : 0);
      o.y = maybe_commit<GATED>(mci1, r.c[j].y, GATED ? r.f[j].y : 0);
      const uint64_t b0 = __ballot(o.x != r.c[j].x);
      const uint64_t b1 = __ballot(o.y != r.c[j].y);
      n_changed += __popcll(b0) + __popcll(b1);
      if (a.changed_bits != nullptr && (tid & 63) == 0) {  // word 2k = even groups, 2k+1 = odd groups of the k-th 128-group run
        u64x2 w;
        w.x = b0;
        w.y = b1;
        stg<false>(reinterpret_cast<u64x2*>(a.changed_bits + (g >> 6)), w);
      }
      stg<STNT>(reinterpret_cast<u64x2*>(a.committed_out + g), o);
    }
  }

  if constexpr (VOTES) {
    if (vote_lane) {
      const uint64_t g = tile0 + 8ull * tid;
      uint32_t out = 0, n_won = 0, n_lost = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        uint32_t w;
        if constexpr (N <= 8) {
          const uint32_t pair = k < 2 ? r.vw[0].x : k < 4 ? r.vw[0].y : k < 6 ? r.vw[0].z : r.vw[0].w;
          w = (k & 1) ? pair >> 16 : pair & 0xffffu;
        } else {
          w = k == 0 ? r.vw[0].x : k == 1 ? r.vw[0].y : k == 2 ? r.vw[0].z : k == 3 ? r.vw[0].w
            : k == 4 ? r.vw[1].x : k == 5 ? r.vw[1].y : k == 6 ? r.vw[1].z : r.vw[1].w;
        }
        const uint32_t mpair = k < 2 ? vmask.x : k < 4 ? vmask.y : k < 6 ? vmask.z : vmask.w;
        const uint32_t oc = poll_word_voters(w, (k & 1) ? mpair >> 16 : mpair & 0xffffu);
        out |= oc << (2 * k);
        n_won += oc & 1u;
        n_lost += oc >> 1;
      }
      stg<STNT>(reinterpret_cast<uint16_t*>(a.outcome + (g >> 2)), (uint16_t)out);  // 8 groups = 16 bits
      won_lost = n_won | (n_lost << 16);
    }
  }

  const uint32_t wl = VOTES ? wave_sum_u32(won_lost) : 0u;
  if ((tid & 63) == 0) {
    uint4 t;
    t.x = n_changed;
    t.y = wl & 0xffffu;
    t.z = wl >> 16;
    t.w = 0;
    stg_u4(a.partials + ((uint64_t)tile * kWaves + (tid >> 6)), t);
  }
