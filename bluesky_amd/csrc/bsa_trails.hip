// Trails.update (traffic/trails.py:71-135) on the device.
//
// k_trail_count   per wave of 64 aircraft indices, how many emit a segment (t - lasttim > dt); word 0 of the
//                 scan's input takes the running total of undrained segments
// scan_excl       (bsa_scan.hip) the waves' offsets -- they already include the total; the last word is the new one
// k_trail_emit    each emitting aircraft writes its segment at its wave's offset + its rank in the wave, and takes
//                 the new position and t as lastlat / lastlon / lasttim; one lane stores the new total
// k_trail_follow  the inactive form: lastlat / lastlon = the positions, lasttim = t
//
// The pass runs over the aircraft INDEX i = 0 .. n-1 (np.where's order), the arrays are read through id2h when they
// are in home order.  The total stays on the device: a pass neither synchronises nor copies.  Every number of a
// segment is a copy; the only arithmetic is the comparison's subtraction.
#include <algorithm>

#include "bsa_stop.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kTrailBlock = 256;

struct TrailArgs {
  int n;
  const double *lat, *lon;             // traf.lat / lon as the step left them
  double *lastlat, *lastlon, *lasttim;
  const unsigned *id2h;                // aircraft index -> position in the arrays, or NULL (identity)
  double t, dt;
};
// the segment buffers (struct of arrays, cap entries each) and the control words {total, demand}
struct TrailSeg {
  double *lat0, *lon0, *lat1, *lon1, *time;
  int *idx;
  unsigned cap;
  unsigned *ctl;
};

// the behind-the-sticky-word decision of a resident launch (word NULL: the standalone entry always runs)
__device__ __forceinline__ bool trail_runs(const unsigned long long *word, unsigned tag) {
  return !word || stop_runs(word, tag);
}

// np.where(t - lasttim > dt): strict, and false for a NaN delta
__device__ __forceinline__ bool trail_emits(const TrailArgs &a, int i, unsigned *h) {
  if (i >= a.n) return false;
  *h = a.id2h ? a.id2h[i] : (unsigned)i;
  return a.t - a.lasttim[*h] > a.dt;
}

// in[0] = the total so far, in[1 + w] = the emitting aircraft of wave w (i in 64 w .. 64 w + 63), in[nw + 1] = 0:
// the exclusive scan's word 1 + w is where wave w writes, its last word the new total
__global__ __launch_bounds__(kTrailBlock) void k_trail_count(TrailArgs a, const unsigned *__restrict__ ctl,
                                                               unsigned *__restrict__ in,
                                                               const unsigned long long *__restrict__ word,
                                                               unsigned tag) {
  if (!trail_runs(word, tag)) return;
  const int i = blockIdx.x * kTrailBlock + threadIdx.x;
  unsigned h;
  const unsigned long long m = __ballot(trail_emits(a, i, &h));
  if ((threadIdx.x & 63) == 0 && i < a.n) in[1 + (i >> 6)] = (unsigned)__popcll(m);
  if (i == 0) {
    in[0] = ctl[0];
    in[1 + ((a.n + 63) >> 6)] = 0u;
  }
}

// Takes the decision k_trail_count took: nothing between the two launches raises the sticky word (the scan between
// them raises nothing, and every launch of a later step is behind them on the stream), and lasttim is written
// here only.  A position past the buffers' end is counted into the demand word, not written (the host sized the
// buffers for the batch: trails_reserve)
__global__ __launch_bounds__(kTrailBlock) void k_trail_emit(TrailArgs a, TrailSeg s, const unsigned *__restrict__ off,
                                                              const unsigned long long *__restrict__ word,
                                                              unsigned tag) {
  if (!trail_runs(word, tag)) return;
  const int i = blockIdx.x * kTrailBlock + threadIdx.x;
  unsigned h = 0;
  const bool e = trail_emits(a, i, &h);
  const unsigned long long m = __ballot(e);
  if (i == 0) s.ctl[0] = off[1 + ((a.n + 63) >> 6)];  // the only store of the total; no lane of this launch reads it
  if (!e) return;
  const unsigned at = off[1 + (i >> 6)] + lane_prefix(m);
  const double lat = a.lat[h], lon = a.lon[h];
  if (at < s.cap) {
    s.lat0[at] = a.lastlat[h];
    s.lon0[at] = a.lastlon[h];
    s.lat1[at] = lat;
    s.lon1[at] = lon;
    s.time[at] = a.t;
    s.idx[at] = i;
  } else {
    atomicAdd(s.ctl + 1, 1u);
  }
  a.lastlat[h] = lat;
  a.lastlon[h] = lon;
  a.lasttim[h] = a.t;
}

// Trails.update while inactive (trails.py:73-77); elementwise, so the arrays' own order serves
__global__ __launch_bounds__(kTrailBlock) void k_trail_follow(TrailArgs a, const unsigned long long *__restrict__ word,
                                                                unsigned tag) {
  if (!trail_runs(word, tag)) return;
  const int k = blockIdx.x * kTrailBlock + threadIdx.x;
  if (k >= a.n) return;
  a.lastlat[k] = a.lat[k];
  a.lastlon[k] = a.lon[k];
  a.lasttim[k] = a.t;
}

static size_t trail_ws_words(int64_t n) { return 2 * (size_t)((n + 63) / 64 + 2); }
static TrailSeg trail_seg(void *base, int64_t cap, unsigned *ctl) {
  double *d = (double *)base;
  const size_t C = (size_t)cap;
  return TrailSeg{d, d + C, d + 2 * C, d + 3 * C, d + 4 * C, (int *)(d + 5 * C), (unsigned)cap, ctl};
}
constexpr size_t kTrailSegBytes = 5 * 8 + 4;

// one Trails.update: enqueue only (ws: trail_ws_words(n) words)
static int trail_pass(Ctx *c, const TrailArgs &a, bool active, const TrailSeg &s, unsigned *ws,
                      const unsigned long long *word, unsigned tag) {
  if (a.n <= 0) return 0;
  const dim3 grid((unsigned)((a.n + kTrailBlock - 1) / kTrailBlock)), blk(kTrailBlock);
  if (!active) {
    hipLaunchKernelGGL(k_trail_follow, grid, blk, 0, c->stream, a, word, tag);
    BSA_HIP(c, hipGetLastError());
    return 0;
  }
  const int nw = (a.n + 63) / 64;
  unsigned *in = ws, *off = ws + nw + 2;
  hipLaunchKernelGGL(k_trail_count, grid, blk, 0, c->stream, a, (const unsigned *)s.ctl, in, word, tag);
  BSA_HIP(c, hipGetLastError());
  if (scan_excl(c, in, off, nw + 2)) return -1;
  hipLaunchKernelGGL(k_trail_emit, grid, blk, 0, c->stream, a, s, (const unsigned *)off, word, tag);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// ---- the resident step's stage
static unsigned *trail_ctl(Ctx *c) { return (unsigned *)((char *)c->sim_ctl.p + kSimCtlTrail); }

int trails_sim_launch(Ctx *c, double t, unsigned tag) {
  const int64_t n = c->n;
  if (!ensure(c, c->tr_ws, trail_ws_words(n) * 4, "trail offsets")) return -1;
  TrailArgs a{(int)n,
              (const double *)c->own[0].p,
              (const double *)c->own[1].p,
              (double *)c->s_tlat.p,
              (double *)c->s_tlon.p,
              (double *)c->s_ttim.p,
              (const unsigned *)c->id2h.p,
              t,
              c->tr_dt};
  return trail_pass(c, a, c->tr_active, trail_seg(c->tr_seg.p, c->tr_cap, trail_ctl(c)), (unsigned *)c->tr_ws.p,
                    (const unsigned long long *)((char *)c->sim_ctl.p + kSimCtlSticky), tag);
}

// The most k steps can emit: an aircraft emits when more than dt has passed since its last segment, so at most
// floor(k simdt / dt) + 1 times in k steps (the + 1: it may be due in the first), and at most once per step
int trails_reserve(Ctx *c, int64_t nsteps) {
  if (!c->sim_trails || !c->tr_active || nsteps <= 0) return 0;
  const double per = std::floor((double)nsteps * c->simp.simdt / c->tr_dt) + 1.0;
  const int64_t passes = per < (double)nsteps ? (int64_t)per : nsteps;
  const int64_t bound = c->tr_undrained + c->n * passes;
  if (bound > c->tr_max)
    return fail(c, "trails: %lld steps may emit %lld segments on top of %lld undrained, max_segments is %lld: drain "
                   "(bsa_sim_trails_drain) or step less", (long long)nsteps, (long long)(c->n * passes),
                (long long)c->tr_undrained, (long long)c->tr_max);
  if (bound <= c->tr_cap) return 0;
  // grow (twice the bound while that fits), keeping what is undrained: the arrays move to their new stride
  const int64_t cap = std::min<int64_t>(c->tr_max, 2 * bound);
  DevBuf nb;
  if (!ensure(c, nb, (size_t)cap * kTrailSegBytes, "trail segments")) return -1;
  const TrailSeg o = trail_seg(c->tr_seg.p, c->tr_cap, nullptr), f = trail_seg(nb.p, cap, nullptr);
  const size_t u = (size_t)c->tr_undrained;
  if (u) {
    const double *from[5] = {o.lat0, o.lon0, o.lat1, o.lon1, o.time};
    double *to[5] = {f.lat0, f.lon0, f.lat1, f.lon1, f.time};
    for (int q = 0; q < 5; ++q) BSA_HIP(c, hipMemcpyAsync(to[q], from[q], u * 8, hipMemcpyDeviceToDevice, c->stream));
    BSA_HIP(c, hipMemcpyAsync(f.idx, o.idx, u * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  release(c->tr_seg);
  c->tr_seg = nb;
  c->tr_cap = cap;
  return 0;
}

int trails_created(Ctx *c, int64_t n, int64_t m, const double *lat, const double *lon) {
  if (!c->sim_trails || m <= 0) return 0;
  // Trails.create (trails.py:64-69): TrafficArrays' defaults (0.0, already there) for all m, then only the LAST new
  // aircraft gets its position; lasttim stays 0 for every one of them
  const size_t last = (size_t)(n + m - 1);
  BSA_HIP(c, hipMemcpyAsync((double *)c->s_tlat.p + last, lat + (m - 1), 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync((double *)c->s_tlon.p + last, lon + (m - 1), 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

void trails_off(Ctx *c) {
  c->sim_trails = c->tr_active = false;
  c->tr_undrained = c->tr_demand = 0;
  c->clk.trail_simt = c->clk.trail_last = 0.0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" {

int bsa_trails_update(bsa_ctx *cc, int64_t n, const double *lat, const double *lon, double *lastlat, double *lastlon,
                      double *lasttim, double t, double dt, int active, int64_t cap, double *lat0, double *lon0,
                      double *lat1, double *lon1, double *time, int32_t *idx, int64_t *count) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!count) return bsa::fail(c, "bsa_trails_update: NULL count");
  *count = 0;
  if (n < 0 || n > 0x7fffffff - 64 || cap < 0) return bsa::fail(c, "bsa_trails_update: bad n or cap");
  if (n == 0) return 0;  // nothing is launched
  if (!lat || !lon || !lastlat || !lastlon || !lasttim) return bsa::fail(c, "bsa_trails_update: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  // stage: lat lon lastlat lastlon lasttim (fp64) | the segments (room for all n) | offsets | {total, demand}
  const size_t N = (size_t)n, W = bsa::trail_ws_words(n);
  if (!bsa::ensure(c, c->tr_stage, 5 * N * 8 + N * bsa::kTrailSegBytes + 8 + W * 4 + 8, "trail arrays")) return -1;
  double *d = (double *)c->tr_stage.p;
  char *seg = (char *)(d + 5 * N);
  unsigned *ws = (unsigned *)(seg + (N * bsa::kTrailSegBytes + 7) / 8 * 8), *ctl = ws + W;
  hipStream_t s = c->stream;
  const double *in[5] = {lat, lon, lastlat, lastlon, lasttim};
  for (int q = 0; q < 5; ++q) BSA_HIP(c, hipMemcpyAsync(d + q * N, in[q], N * 8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemsetAsync(ctl, 0, 8, s));
  const bsa::TrailArgs a{(int)n, d, d + N, d + 2 * N, d + 3 * N, d + 4 * N, nullptr, t, dt};
  const bsa::TrailSeg sg = bsa::trail_seg(seg, n, ctl);
  if (bsa::trail_pass(c, a, active != 0, sg, ws, nullptr, 0u)) return -1;
  unsigned h[2] = {0u, 0u};
  BSA_HIP(c, hipMemcpyAsync(h, ctl, 8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  if (h[1] || h[0] > (unsigned)n) return bsa::fail(c, "internal: %u trail segments of %lld aircraft", h[0] + h[1], (long long)n);
  *count = (int64_t)h[0];
  if (*count > cap) return bsa::fail(c, "bsa_trails_update: %lld segments, room for %lld", (long long)*count, (long long)cap);
  if (*count > 0 && (!lat0 || !lon0 || !lat1 || !lon1 || !time || !idx)) return bsa::fail(c, "bsa_trails_update: NULL segment array");
  double *out[3] = {lastlat, lastlon, lasttim};
  for (int q = 0; q < 3; ++q) BSA_HIP(c, hipMemcpyAsync(out[q], d + (2 + q) * N, N * 8, hipMemcpyDeviceToHost, s));
  const size_t u = (size_t)h[0];
  if (u) {
    double *to[5] = {lat0, lon0, lat1, lon1, time};
    const double *from[5] = {sg.lat0, sg.lon0, sg.lat1, sg.lon1, sg.time};
    for (int q = 0; q < 5; ++q) BSA_HIP(c, hipMemcpyAsync(to[q], from[q], u * 8, hipMemcpyDeviceToHost, s));
    BSA_HIP(c, hipMemcpyAsync(idx, sg.idx, u * 4, hipMemcpyDeviceToHost, s));
  }
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}

int bsa_sim_set_trails(bsa_ctx *cc, int on, int active, double dt, double simt, const double *lasttim,
                       int64_t max_segments) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_trails before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  if (!on) {
    bsa::trails_off(c);
    return 0;
  }
  if (c->nranks > 1)
    return bsa::fail(c, "bsa_sim_set_trails on %d ranks: the ordered emission runs over all aircraft indices on one "
                        "device, and the merge of several ranks' streams is not built (one rank only)", c->nranks);
  if (!(dt > 0.0)) return bsa::fail(c, "bsa_sim_set_trails: dt must be > 0");
  const int64_t n = c->n;
  if (max_segments < n || max_segments > 0x7fffffff - 64)
    return bsa::fail(c, "bsa_sim_set_trails: max_segments %lld holds less than one pass of %lld aircraft (or more than "
                        "2^31 - 1)", (long long)max_segments, (long long)n);
  hipStream_t s = c->stream;
  if (!c->sim_trails) {  // enabling: as after an inactive Trails.update at `lasttim`
    if (!lasttim) return bsa::fail(c, "bsa_sim_set_trails: NULL lasttim");
    bsa::DevBuf *f8[3] = {&c->s_tlat, &c->s_tlon, &c->s_ttim};
    for (bsa::DevBuf *b : f8)
      if (!bsa::ensure(c, *b, (size_t)n * 8, "trail arrays")) return -1;
    BSA_HIP(c, hipMemcpyAsync(c->s_tlat.p, c->own[0].p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    BSA_HIP(c, hipMemcpyAsync(c->s_tlon.p, c->own[1].p, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    bsa::HomeBatch up(c, true);
    if (up.add(c->s_ttim.p, lasttim, nullptr, 8) || up.run()) return -1;
    BSA_HIP(c, hipMemsetAsync(bsa::trail_ctl(c), 0, 8, s));
    BSA_HIP(c, hipStreamSynchronize(s));
    c->tr_undrained = c->tr_demand = 0;
    c->clk.trail_simt = c->clk.trail_last = simt;
  } else if (c->tr_active && !active) {
    // setTrails(False): clear() drops the undrained segments (clearnew); the next step's inactive update then
    // sets lastlat / lastlon / lasttim
    BSA_HIP(c, hipMemsetAsync(bsa::trail_ctl(c), 0, 4, s));
    BSA_HIP(c, hipStreamSynchronize(s));
    c->tr_undrained = 0;
  }
  c->tr_active = active != 0;
  c->tr_dt = dt;
  c->tr_max = max_segments;
  c->sim_trails = true;
  return 0;
}

int bsa_sim_trails_drain(bsa_ctx *cc, int64_t cap, double *lat0, double *lon0, double *lat1, double *lon1, double *time,
                         int32_t *idx, int64_t *count, double *lastlat, double *lastlon) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!count) return bsa::fail(c, "bsa_sim_trails_drain: NULL count");
  *count = 0;
  if (!c->sim_ready || !c->sim_trails) return bsa::fail(c, "bsa_sim_trails_drain: trails are off");
  BSA_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  unsigned h[2] = {0u, 0u};
  BSA_HIP(c, hipMemcpyAsync(h, bsa::trail_ctl(c), 8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  if (h[1] || (int64_t)h[0] > c->tr_cap)
    return bsa::fail(c, "internal error: %u trail segments did not fit (%u of %lld)", h[1], h[0], (long long)c->tr_cap);
  *count = (int64_t)h[0];
  if (*count > cap) return 0;  // (nothing consumed: ask again with room)
  const size_t u = (size_t)h[0];
  if (u) {
    if (!lat0 || !lon0 || !lat1 || !lon1 || !time || !idx) return bsa::fail(c, "bsa_sim_trails_drain: NULL segment array");
    const bsa::TrailSeg sg = bsa::trail_seg(c->tr_seg.p, c->tr_cap, nullptr);
    // through the pinned staging, 2^18 segments at a time (a DMA straight into pageable memory made the NEXT
    // batch slow: 100 box100k steps 10.7 -> 25 .. 36 ms after a drain of 100 000 segments)
    const size_t chunk = (size_t)1 << 18;
    for (size_t at = 0; at < u; at += chunk) {
      const size_t m = std::min(chunk, u - at);
      unsigned char *pin = bsa::pin_stage(c, m * bsa::kTrailSegBytes);
      if (!pin) return -1;
      const void *from[6] = {sg.lat0 + at, sg.lon0 + at, sg.lat1 + at, sg.lon1 + at, sg.time + at, sg.idx + at};
      void *to[6] = {lat0 + at, lon0 + at, lat1 + at, lon1 + at, time + at, idx + at};
      bsa::HostCopy jobs[6];
      for (int q = 0; q < 6; ++q) {
        const size_t b = m * (q < 5 ? 8 : 4);
        BSA_HIP(c, hipMemcpyAsync(pin + (size_t)q * m * 8, from[q], b, hipMemcpyDeviceToHost, s));
        jobs[q] = bsa::HostCopy{to[q], pin + (size_t)q * m * 8, b};
      }
      BSA_HIP(c, hipStreamSynchronize(s));
      bsa::host_copy(jobs, 6);
    }
  }
  BSA_HIP(c, hipMemsetAsync(bsa::trail_ctl(c), 0, 4, s));  // clearnew()
  BSA_HIP(c, hipStreamSynchronize(s));
  c->tr_undrained = 0;
  if (lastlat || lastlon) {
    bsa::HomeBatch down(c, false);
    if ((lastlat && down.add(c->s_tlat.p, nullptr, lastlat, 8)) || (lastlon && down.add(c->s_tlon.p, nullptr, lastlon, 8)))
      return -1;
    return down.run();
  }
  return 0;
}

int bsa_sim_read_trails(bsa_ctx *cc, double *lastlat, double *lastlon, double *lasttim, double *simt, double *last_t,
                        int64_t *undrained) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready || !c->sim_trails) return bsa::fail(c, "bsa_sim_read_trails: trails are off");
  BSA_HIP(c, hipSetDevice(c->device));
  if (simt) *simt = c->clk.trail_simt;
  if (last_t) *last_t = c->clk.trail_last;
  if (undrained) *undrained = c->tr_undrained;
  bsa::HomeBatch down(c, false);
  double *dst[3] = {lastlat, lastlon, lasttim};
  bsa::DevBuf *src[3] = {&c->s_tlat, &c->s_tlon, &c->s_ttim};
  for (int k = 0; k < 3; ++k)
    if (dst[k] && down.add(src[k]->p, nullptr, dst[k], 8)) return -1;
  return down.run();
}

}  // extern "C"
