// raftq_tick_lists32.inc -- tick_lists32_kernel's text (raftq_kernels.hpp, inside namespace raftqk), included twice: as
// tick_lists32_kernel<BEAT_BITMAP>, the two-list form, and as tick_lists32_checks_kernel<BEAT_BITMAP>, which also lists the groups
// whose check failed (raftq_tick_set_checks on a handle with raftq_set_check_quorum on): tick_check_kernel's third bitmap and the
// partials' third word, ranked and written exactly as the MsgHup ids are; their total goes to totals[4] (words 1 .. 3 of that block
// carry other calls' flags).  Each time it sets
//   RAFTQ_LISTS_KERNEL      the kernel's name
//   RAFTQ_LISTS_N           2 or 3: lists compacted in LDS
//   RAFTQ_LISTS_PARAM       the three-list form's extra, LAST parameter (", TickChecksArgs c")
//   RAFTQ_LISTS_CHK(...)    its arguments in the three-list form, nothing in the two-list form
// An include and not a template <bool CHECKS> body both kernels call, for the reason raftq_step_walk_kernels.inc gives: as a body the
// two-list kernels came out with other machine code than their parent's (tools/isa_unchanged.py; profiles/r28/README.md); as an
// include the two-list expansion is token for token what it was.
template <bool BEAT_BITMAP>
static __global__ __launch_bounds__(kBlock) void RAFTQ_LISTS_KERNEL(const uint64_t* __restrict__ hup_bits, const uint64_t* __restrict__ beat_bits,
                                                                      const uint4* __restrict__ partials, uint64_t n_chunks /* gpad / 256 */,
                                                                      uint32_t* hup_out, uint64_t hup_cap, uint32_t* beat_out, uint64_t beat_cap,
                                                                      uint64_t* beat_map, uint64_t* totals /*[2]*/,
                                                                      const uint64_t* __restrict__ wave_off_hup, const uint64_t* __restrict__ wave_off_beat RAFTQ_LISTS_PARAM) {
  constexpr int kC = kWaves;  // 256-group chunks (a tick wave's share) per workgroup
  __shared__ uint64_t red[RAFTQ_LISTS_N][kWaves];
  __shared__ uint32_t mine[RAFTQ_LISTS_N][kC];
  __shared__ uint32_t ids[RAFTQ_LISTS_N][kBlock * 4];
  __shared__ uint64_t map_words[kC * 4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t first_wave = (uint64_t)blockIdx.x * kC;
  uint64_t acc_h = 0, acc_b = 0;
  RAFTQ_LISTS_CHK(uint64_t acc_c = 0;)
  if (wave_off_hup == nullptr) {
    uint32_t h0 = 0, h1 = 0, b0 = 0, b1 = 0;
    RAFTQ_LISTS_CHK(uint32_t c0 = 0, c1 = 0;)
    uint64_t i = tid;
    for (; i + kBlock < first_wave; i += 2 * kBlock) {
      const uint4 p0 = partials[i], p1 = partials[i + kBlock];
      h0 += p0.x; b0 += p0.y;
      h1 += p1.x; b1 += p1.y;
      RAFTQ_LISTS_CHK(c0 += p0.z; c1 += p1.z;)
    }
    if (i < first_wave) {
      const uint4 p0 = partials[i];
      h0 += p0.x; b0 += p0.y;
      RAFTQ_LISTS_CHK(c0 += p0.z;)
    }
    acc_h = (uint64_t)h0 + h1;
    acc_b = (uint64_t)b0 + b1;
    RAFTQ_LISTS_CHK(acc_c = (uint64_t)c0 + c1;)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      acc_h += __shfl_xor(acc_h, o, 64);
      acc_b += __shfl_xor(acc_b, o, 64);
      RAFTQ_LISTS_CHK(acc_c += __shfl_xor(acc_c, o, 64);)
    }
  } else if (lane == 0 && wave == 0) {
    acc_h = wave_off_hup[first_wave];
    acc_b = wave_off_beat[first_wave];
    RAFTQ_LISTS_CHK(acc_c = c.wave_off_chk[first_wave];)
  }
  if (lane == 0) {
    red[0][wave] = acc_h;
    red[1][wave] = acc_b;
    RAFTQ_LISTS_CHK(red[2][wave] = acc_c;)
  }
  if (tid < kC) {
    uint4 p;
    p.x = p.y = p.z = p.w = 0;
    if (first_wave + tid < n_chunks) p = partials[first_wave + tid];
    mine[0][tid] = p.x;
    mine[1][tid] = p.y;
    RAFTQ_LISTS_CHK(mine[2][tid] = p.z;)
  }
  __syncthreads();
  uint64_t pos_h = 0, pos_b = 0;  // where this workgroup's ids start in the two lists
  uint32_t tot_h = 0, tot_b = 0;  // the lengths of its two runs
  RAFTQ_LISTS_CHK(uint64_t pos_c = 0; uint32_t tot_c = 0;)
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    pos_h += red[0][k];
    pos_b += red[1][k];
    RAFTQ_LISTS_CHK(pos_c += red[2][k];)
  }
#pragma unroll
  for (int k = 0; k < kC; ++k) {
    tot_h += mine[0][k];
    tot_b += mine[1][k];
    RAFTQ_LISTS_CHK(tot_c += mine[2][k];)
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    totals[0] = pos_h + tot_h;
    totals[1] = pos_b + tot_b;
    RAFTQ_LISTS_CHK(totals[4] = pos_c + tot_c;)
  }
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const uint32_t ci = wave;  // this wave's chunk
  const uint64_t wv = first_wave + ci;
  if (wv < n_chunks) {  // wave-uniform
    uint32_t loc_h = 0, loc_b = 0;  // this chunk's first id inside the workgroup's runs
    RAFTQ_LISTS_CHK(uint32_t loc_c = 0;)
#pragma unroll
    for (int k = 0; k < kC; ++k) {
      loc_h += (uint32_t)k < ci ? mine[0][k] : 0u;
      loc_b += (uint32_t)k < ci ? mine[1][k] : 0u;
      RAFTQ_LISTS_CHK(loc_c += (uint32_t)k < ci ? mine[2][k] : 0u;)
    }
    uint64_t hb[4], bb[4];
    RAFTQ_LISTS_CHK(uint64_t cb[4];)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hb[k] = hup_bits[wv * 4 + k];
      bb[k] = beat_bits[wv * 4 + k];
      RAFTQ_LISTS_CHK(cb[k] = c.chk_bits[wv * 4 + k];)
    }
    uint32_t rh = loc_h + __popcll(hb[0] & below) + __popcll(hb[1] & below) + __popcll(hb[2] & below) + __popcll(hb[3] & below);
    uint32_t rb = loc_b + __popcll(bb[0] & below) + __popcll(bb[1] & below) + __popcll(bb[2] & below) + __popcll(bb[3] & below);
    RAFTQ_LISTS_CHK(uint32_t rc = loc_c + __popcll(cb[0] & below) + __popcll(cb[1] & below) + __popcll(cb[2] & below) + __popcll(cb[3] & below);)
    uint32_t nib = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t g = (uint32_t)(wv * 256 + 4ull * lane + k);
      if ((hb[k] >> lane) & 1) ids[0][rh++] = g;
      if (!BEAT_BITMAP) {
        if ((bb[k] >> lane) & 1) ids[1][rb++] = g;
      } else {
        nib |= (uint32_t)((bb[k] >> lane) & 1) << k;
      }
      RAFTQ_LISTS_CHK(if ((cb[k] >> lane) & 1) ids[2][rc++] = g;)
    }
    if (BEAT_BITMAP) {
      // lane l holds the four bits of groups 4l .. 4l+3 of the chunk's 256: group-order word j is lanes 16j .. 16j+15
      uint64_t v = (uint64_t)nib << (4 * (lane & 15));
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v |= __shfl_xor(v, o, 64);
      if ((lane & 15) == 0) map_words[ci * 4 + (lane >> 4)] = v;
    }
  }
  __syncthreads();
  run_out(hup_out, hup_cap, pos_h, ids[0], tot_h, tid);
  if (!BEAT_BITMAP) {
    run_out(beat_out, beat_cap, pos_b, ids[1], tot_b, tid);
  } else if (tid < kC * 4 && first_wave * 4 + tid < n_chunks * 4) {
    beat_map[first_wave * 4 + tid] = map_words[tid];
  }
  RAFTQ_LISTS_CHK(run_out(c.chk_out, c.chk_cap, pos_c, ids[2], tot_c, tid);)
}
