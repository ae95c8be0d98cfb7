// Exclusive prefix sum of unsigned words in one launch (scan_excl,
// bsa_internal.h): K2's row offsets at bucket width 0, the halo plan's lists.
// On top of it the ordered index list of a flag array (flagged_list): the
// stopping stages' fired conditions and delete lists.  Both also as C entries
// over host arrays, for the tests (bsa_scan_excl, bsa_flagged_list).
#include <algorithm>

#include "bsa_internal.h"
#include "bsa_wave.h"

namespace bsa {

// ------------------------------------------------------------------ single-pass scan
// Exclusive prefix sum of n unsigned words in ONE launch (replaces hipcub's
// three: look-back init + scan, ~16 us per detect at 100k): decoupled
// look-back over 8192-word tiles.  Tiles are numbered by a ticket (a running
// device counter; the host knows its base), so a tile only ever waits on tiles
// that already started.  Tile status words carry the launch's epoch, so they
// need no zeroing between launches: {epoch:30 | flag:2 | value:32}, flag 1 =
// the tile's own total, 2 = inclusive prefix through the tile.
// Tiles of kScanThreads x kScanItems words: 2048 below 2^19 words (more tiles
// in flight: K2 26.3 -> 24.6 us at 100k, 19.9 -> 14.6 us for one rank of 8),
// 8192 above (at 1M a 2048-word tiling's ~1000 tiles lengthened the ticket
// queue and the look-back: 62 -> 139 us)
__device__ __forceinline__ unsigned long long scan_word(unsigned epoch, unsigned flag, unsigned v) {
  return ((unsigned long long)(epoch & 0x3fffffffu) << 34) | ((unsigned long long)flag << 32) | v;
}
template <int kScanThreads, int kScanItems>
__global__ __launch_bounds__(kScanThreads) void k_scan_excl(const unsigned *__restrict__ in, unsigned *__restrict__ out,
                                                            int n, unsigned long long *__restrict__ ticket,
                                                            unsigned long long base,
                                                            unsigned long long *__restrict__ status, unsigned epoch) {
  constexpr int kScanTile = kScanThreads * kScanItems;
  __shared__ unsigned wsum[kScanThreads / 64];
  __shared__ unsigned s_tile, s_excl;
  if (threadIdx.x == 0) s_tile = (unsigned)(atomicAdd(ticket, 1ull) - base);
  __syncthreads();
  const unsigned tile = s_tile;
  const long long i0 = (long long)tile * kScanTile + (long long)threadIdx.x * kScanItems;
  unsigned v[kScanItems], tsum = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = (i0 + k < n) ? in[i0 + k] : 0u;
    tsum += v[k];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned x = wave_incl_scan(tsum);
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  // wave 0: tile total, then a wave-wide look-back (64 predecessors per round:
  // the nearest inclusive prefix, plus the aggregates after it)
  if (w == 0) {
    const unsigned wv = lane < kScanThreads / 64 ? wsum[lane] : 0u;
    const unsigned wx = wave_incl_scan(wv);
    if (lane < kScanThreads / 64) wsum[lane] = wx - wv;  // exclusive per-wave offsets
    const unsigned total = __builtin_amdgcn_readlane(wx, 63);
    unsigned excl = 0;
    if (tile == 0) {
      if (lane == 0)
        __hip_atomic_store(&status[0], scan_word(epoch, 2, total), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (lane == 0)
        __hip_atomic_store(&status[tile], scan_word(epoch, 1, total), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      int top = (int)tile - 1;  // highest predecessor not yet summed
      for (;;) {
        const int j = top - lane;
        unsigned long long st = 0;
        if (j >= 0) st = __hip_atomic_load(&status[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned flag = ((unsigned)(st >> 34) == (epoch & 0x3fffffffu)) ? ((unsigned)(st >> 32) & 3u) : 0u;
        // lanes past tile 0 count as "inclusive 0"
        const bool incl = j < 0 || flag == 2, ready = j < 0 || flag != 0;
        const unsigned long long mi = __ballot(incl), mr = __ballot(ready);
        // first lane (nearest predecessor) holding an inclusive prefix, or 64
        const int fi = mi ? __builtin_ctzll(mi) : 64;
        // every lane up to fi must be ready, else spin on this window
        const unsigned long long need = fi >= 63 ? ~0ull : ((2ull << fi) - 1);
        if ((mr & need) != need) {
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        unsigned part = (lane <= fi && j >= 0) ? (unsigned)st : 0u;
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        excl += part;
        if (fi < 64) break;
        top -= 64;
      }
      if (lane == 0)
        __hip_atomic_store(&status[tile], scan_word(epoch, 2, excl + total), __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) s_excl = excl;
  }
  __syncthreads();
  unsigned run = s_excl + wsum[w] + x - tsum;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += v[k];
  }
}

int scan_excl(Ctx *c, const unsigned *in, unsigned *out, int n) {
  if (n <= 0) return 0;
  const bool small = n <= (1 << 19);
  const int kScanTile = small ? 512 * 4 : 1024 * 8;
  const unsigned tiles = ((unsigned)n + kScanTile - 1) / kScanTile;  // (unsigned: n + tile - 1 may pass 2^31)
  const size_t had = c->scan_ws.bytes;
  if (!ensure_keep(c, c->scan_ws, 8 * (size_t)(1 + tiles), "scan tile status")) return -1;
  if (c->scan_ws.bytes != had) c->scan_ready = false;  // grown: the new words are uninitialised
  if (!c->scan_ready) {  // ticket counter and tile status start at 0
    BSA_HIP(c, hipMemsetAsync(c->scan_ws.p, 0, c->scan_ws.bytes, c->stream));
    c->scan_ready = true;
    c->scan_tickets = 0;
    c->scan_epoch = 0;
  }
  const unsigned epoch = ++c->scan_epoch;  // never 0: fresh (zeroed) status words are never ready
  unsigned long long *ws = (unsigned long long *)c->scan_ws.p;
  if (small)
    hipLaunchKernelGGL((k_scan_excl<512, 4>), dim3(tiles), dim3(512), 0, c->stream, in, out, n, ws, c->scan_tickets,
                       ws + 1, epoch);
  else
    hipLaunchKernelGGL((k_scan_excl<1024, 8>), dim3(tiles), dim3(1024), 0, c->stream, in, out, n, ws,
                       c->scan_tickets, ws + 1, epoch);
  BSA_HIP(c, hipGetLastError());
  c->scan_tickets += tiles;
  return 0;
}

// ------------------------------------------------------------------ ordered index list
constexpr int kFlagBlock = 256;
__device__ __forceinline__ bool flag_set(int i, int n, const uint8_t *flag, const unsigned *id2h, unsigned mask) {
  return i < n && (flag[id2h ? id2h[i] : (unsigned)i] & mask) != 0;
}
// wcnt[w]: the flagged of wave w (i in 64 w .. 64 w + 63); wcnt[nw] = 0, so that the exclusive scan's last word is
// the total
__global__ __launch_bounds__(kFlagBlock) void k_flag_count(int n, const uint8_t *__restrict__ flag,
                                                             const unsigned *__restrict__ id2h, unsigned mask,
                                                             unsigned *__restrict__ wcnt) {
  const int i = blockIdx.x * kFlagBlock + threadIdx.x;
  const unsigned long long m = __ballot(flag_set(i, n, flag, id2h, mask));
  if ((threadIdx.x & 63) == 0 && i < n + 64) wcnt[i >> 6] = i < n ? (unsigned)__popcll(m) : 0u;
}
__global__ __launch_bounds__(kFlagBlock) void k_flag_emit(int n, const uint8_t *__restrict__ flag,
                                                            const unsigned *__restrict__ id2h, unsigned mask,
                                                            const unsigned *__restrict__ woff, int *__restrict__ out) {
  const int i = blockIdx.x * kFlagBlock + threadIdx.x;
  const bool f = flag_set(i, n, flag, id2h, mask);
  const unsigned long long m = __ballot(f);
  if (f) out[woff[i >> 6] + lane_prefix(m)] = i;  // (woff[w] + rank < total <= n)
}

// ws: (nw + 1) counts, (nw + 1) offsets, n indices (int / unsigned words)
size_t flagged_ws_words(int64_t n) { return 2 * (size_t)((n + 63) / 64 + 1) + (size_t)n; }
int flagged_list(Ctx *c, int64_t n, const uint8_t *flag, const unsigned *id2h, unsigned mask, unsigned *ws,
                 std::vector<int32_t> *out, const int **dev_list) {
  const int nw = (int)((n + 63) / 64);
  unsigned *wcnt = ws, *woff = ws + nw + 1;
  int *list = (int *)(ws + 2 * (nw + 1));
  if (dev_list) *dev_list = list;
  const auto grid = [](int64_t m) { return dim3((unsigned)((m + kFlagBlock - 1) / kFlagBlock)); };
  hipLaunchKernelGGL(k_flag_count, grid(n + 64), dim3(kFlagBlock), 0, c->stream, (int)n, flag, id2h, mask, wcnt);
  BSA_HIP(c, hipGetLastError());
  if (scan_excl(c, wcnt, woff, nw + 1)) return -1;
  hipLaunchKernelGGL(k_flag_emit, grid(n), dim3(kFlagBlock), 0, c->stream, (int)n, flag, id2h, mask,
                     (const unsigned *)woff, list);
  BSA_HIP(c, hipGetLastError());
  unsigned total = 0;
  BSA_HIP(c, hipMemcpyAsync(&total, woff + nw, 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  if (total > (unsigned)n) return fail(c, "internal: %u flagged of %lld", total, (long long)n);
  out->assign((size_t)total, 0);
  if (total) BSA_HIP(c, hipMemcpy(out->data(), list, (size_t)total * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace bsa

// ------------------------------------------------------------------ test seams
// The two primitives over host arrays (tests/test_gpu_scan.py): staged into device scratch, run by the functions
// above on the context's stream -- the context's scan_ws, tickets and epoch are the ones every other caller uses
extern "C" int bsa_scan_excl(bsa_ctx *cc, int64_t n, const uint32_t *in, uint32_t *out) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_scan_excl: bad n");
  if (n == 0) return 0;
  if (!in || !out) return bsa::fail(c, "bsa_scan_excl: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  if (!bsa::ensure(c, c->scan_stage, 2 * N * 4, "scan arrays")) return -1;
  unsigned *d_in = (unsigned *)c->scan_stage.p, *d_out = d_in + N;
  hipStream_t s = c->stream;
  BSA_HIP(c, hipMemcpyAsync(d_in, in, N * 4, hipMemcpyHostToDevice, s));
  if (bsa::scan_excl(c, d_in, d_out, (int)n)) return -1;
  BSA_HIP(c, hipMemcpyAsync(out, d_out, N * 4, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}

extern "C" int bsa_flagged_list(bsa_ctx *cc, int64_t n, const uint8_t *flag, const uint32_t *id2h, uint32_t mask,
                                int64_t cap, int32_t *out, int64_t *count) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!count) return bsa::fail(c, "bsa_flagged_list: NULL count");
  *count = 0;
  if (n < 0 || n > 0x7fffffff - 64 || cap < 0) return bsa::fail(c, "bsa_flagged_list: bad n or cap");
  if (n == 0) return 0;  // nothing is launched
  if (!flag) return bsa::fail(c, "bsa_flagged_list: NULL flags");
  if (id2h)
    for (int64_t k = 0; k < n; ++k)
      if (id2h[k] >= (uint64_t)n)
        return bsa::fail(c, "bsa_flagged_list: id2h[%lld] = %u of %lld", (long long)k, id2h[k], (long long)n);
  BSA_HIP(c, hipSetDevice(c->device));
  // stage: id2h | the compaction's words | flags
  const size_t N = (size_t)n, W = bsa::flagged_ws_words(n);
  if (!bsa::ensure(c, c->scan_stage, (N + W) * 4 + N, "flag list arrays")) return -1;
  unsigned *d_id = (unsigned *)c->scan_stage.p, *d_ws = d_id + N;
  uint8_t *d_flag = (uint8_t *)(d_ws + W);
  hipStream_t s = c->stream;
  if (id2h) BSA_HIP(c, hipMemcpyAsync(d_id, id2h, N * 4, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_flag, flag, N, hipMemcpyHostToDevice, s));
  std::vector<int32_t> list;
  if (bsa::flagged_list(c, n, d_flag, id2h ? d_id : (const unsigned *)nullptr, mask, d_ws, &list, nullptr)) return -1;
  *count = (int64_t)list.size();
  if (*count > cap) return bsa::fail(c, "bsa_flagged_list: %lld flagged, room for %lld", (long long)*count, (long long)cap);
  if (*count > 0 && !out) return bsa::fail(c, "bsa_flagged_list: NULL list");
  std::copy(list.begin(), list.end(), out);
  return 0;
}
