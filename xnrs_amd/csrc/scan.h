// The wave and workgroup steps of the row-list kernels (row_lists.hip), each written once.  A list kernel turns mask rows
// into ascending lists of token rows; what it repeats is: count the live tokens of a row (a ballot, or the popcount of a
// bit word), scan the counts to first places, and put every live token at "first place of its row + live tokens before it
// in the row".  Everything here is forceinline and takes its LDS from the kernel: a kernel's LDS layout is its own.
//
//   lanes_below, wave_incl_scan   one wave (64 lanes)
//   wg_excl_scan2                 a 1 024-thread workgroup, two values per thread, rounds joined by a running carry
//   PassLists                     where pass p of launch_compact_rows writes (kernels.h)
//   ballot_walk_row               a wave walks one mask row of any length and places its live tokens
//   place_flat                    one token of rows of <= 64 tokens kept as bit words: its place from the bits below it
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace xnrs {

// the lanes before this one
__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// x summed over the lanes 0 .. lane of the wave
__device__ __forceinline__ int wave_incl_scan(int x, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(x, off);
    if (lane >= off) x += up;
  }
  return x;
}

// Exclusive scans of v0 and v1 over the 1 024 threads of the workgroup, behind what earlier rounds summed: wave scans
// joined through s_wsum.  s_ex[0 / 1][tid] = s_carry[0 / 1] + the v0 / v1 of the threads before tid; then s_carry moves on
// by the round's totals.  On entry s_carry is readable (a barrier since it was written; zero before the first round).  Two
// barriers: the prefixes are written behind the first, and own(ex0, ex1) -- the thread's stores of what follows from its
// OWN two prefixes -- runs there, before the second (behind it the thread would have to carry or reload them).  Behind
// the second every thread may read every s_ex, and thread 1023 hands the carry over: the next round reads it behind ITS
// first barrier, so the caller needs no barrier for the carry (it needs one before s_ex is written again).  The values
// come in by value: as a reference to the kernel's array they cost compact_rows_kernel two VGPRs.
template <class Own>
__device__ __forceinline__ void wg_excl_scan2(int v0, int v1, int (*s_ex)[1024], int (*s_wsum)[16], int* s_carry, Own own) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int v[2] = {v0, v1};
  int incl[2];
  for (int which = 0; which < 2; ++which) {
    incl[which] = wave_incl_scan(v[which], lane);
    if (lane == 63) s_wsum[which][wave] = incl[which];
  }
  __syncthreads();
  for (int which = 0; which < 2; ++which) {
    int before = s_carry[which];
    for (int w = 0; w < wave; ++w) before += s_wsum[which][w];
    s_ex[which][tid] = before + incl[which] - v[which];
  }
  own(s_ex[0][tid], s_ex[1][tid]);
  __syncthreads();
  if (tid == 1023) {
    s_carry[0] = s_ex[0][1023] + v0;
    s_carry[1] = s_ex[1][1023] + v1;
  }
}

// the outputs of pass p (= blockIdx.x) of launch_compact_rows: its offsets start at p*(chunk+1), its lists at p*chunk*S,
// its blocks at p*chunk, its counts at 3*p
struct PassLists {
  int64_t* row_off;
  int32_t* live_src;
  int32_t* kv_src;
  int32_t* kv_block;
  int64_t* counts;
  __device__ __forceinline__ PassLists(int64_t p, int64_t chunk, int S, int64_t* row_off_all, int32_t* live_all, int32_t* kvs_all,
                                       int32_t* kvb_all, int64_t* counts_all)
      : row_off(row_off_all + p * (chunk + 1)),
        live_src(live_all + p * chunk * S),
        kv_src(kvs_all + p * chunk * S),
        kv_block(kvb_all + p * chunk),
        counts(counts_all + 3 * p) {}
};

// A wave walks the mask row mp[0 .. len) 64 tokens at a time: live(place, s) for every token s with mp[s] != 0, in
// ascending order from place `first` on (the lanes of a ballot take consecutive places), and -- when the row is `kept` --
// each(s) for every token of the row.  Called by all 64 lanes with the same arguments.  A place is handed over as it is
// computed, UNSIGNED (__popcll is): a functor that takes it as int makes every store sign-extend its index first.
template <class Live, class Each>
__device__ __forceinline__ void ballot_walk_row(const float* mp, int len, int first, bool kept, int lane, Live live, Each each) {
  const uint64_t below = lanes_below(lane);
  int w = first;
  for (int s0 = 0; s0 < len; s0 += 64) {
    const int sl = s0 + lane;
    const bool on = sl < len && mp[sl] != 0.f;
    const uint64_t b = __ballot(on);
    if (on) live(w + __popcll(b & below), sl);
    w += __popcll(b);
    if (kept && sl < len) each(sl);
  }
}

// Element i of the flattened sweep of a workgroup over rows of S <= 64 tokens whose live tokens are the bits of
// s_bits[row] (element i -> row i / S, token i % S): each(row, s) if the row has a live token at all, live(row, s, place)
// if this token is live, place = the row's first place + the popcount of the bits below it, unsigned as above.  (The loop
// over i stays with the kernel: how far it is unrolled is the kernel's matter.)
template <class Each, class Live>
__device__ __forceinline__ void place_flat(const unsigned long long* s_bits, const int* s_first, int i, int S, Each each, Live live) {
  const int jj = i / S, sl = i - jj * S;
  const unsigned long long b = s_bits[jj];
  if (b == 0ull) return;
  each(jj, sl);
  if ((b >> sl) & 1ull) live(jj, sl, s_first[jj] + __popcll(b & ((1ull << sl) - 1ull)));
}

}  // namespace xnrs
