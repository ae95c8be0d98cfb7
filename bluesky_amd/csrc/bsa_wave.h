// Wave64 helpers of the conflict detection kernels (scan, broadcast, lane
// prefix, min / max) and the per-detect state's zeroing (zero_state: k_zero,
// k_prep_cols, k_rank_rows).
#pragma once
#include "bsa_cd_args.h"

namespace bsa {

// inclusive wave64 prefix sum on the DPP crossbar (no LDS round trips):
// row_shr 1/2/4/8 within each 16-lane row, then row_bcast 15 / 31 across rows
__device__ __forceinline__ unsigned wave_incl_scan(unsigned x) {
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);
  x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
  return x;
}

__device__ __forceinline__ unsigned long long wave_bcast_u64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned lane_prefix(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ float wmin(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wmax(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Counters words that belong to the candidate list (kept across detects by reuse)
__device__ __forceinline__ bool list_word(int k) {
  constexpr int kCand = (int)(offsetof(Counters, cand) / 8), kTiles = (int)(offsetof(Counters, tiles) / 8);
  constexpr int kGroups = (int)(offsetof(Counters, groups) / 8), kStamp = (int)(offsetof(Counters, stamp) / 8);
  constexpr int kNear = (int)(offsetof(Counters, tiles_near) / 8);
  constexpr int kAny = (int)(offsetof(Counters, any_conf) / 8);  // (each detect's evaluation sets it anew)
  return k == kCand || k == kTiles || k == kNear || k == kGroups || (k >= kStamp && k != kAny);
}

__device__ __forceinline__ void zero_state(const ZeroArgs &z, int t, int nt) {
  constexpr int kWords = (int)(sizeof(Counters) / 8);
  constexpr int kTilesWord = (int)(offsetof(Counters, tiles) / 8);
  constexpr int kNearWord = (int)(offsetof(Counters, tiles_near) / 8);
  const int m = max(max(max(2 * (z.nrows + 1), kWorkShards * kWorkStride), kWords),
                    max(max(z.xn[0], z.xn[1]), z.xn[2]));
  for (int k = t; k < m; k += nt) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (k < z.xn[r]) z.x[r][k] = 0u;
    if (k < kWords && (z.full || (k != kTilesWord && k != kNearWord)) && !(z.keep && list_word(k)))
      reinterpret_cast<unsigned long long *>(z.cnt)[k] = 0;
    if (k < kWorkShards * kWorkStride) z.work[k] = 0;
    if (k < z.nrows) {
      z.inconf[k] = 0;
      z.tcpamax[k] = 0;
    }
    if (k < 2 * (z.nrows + 1)) z.rowcnt[k] = 0;
  }
}

}  // namespace bsa
