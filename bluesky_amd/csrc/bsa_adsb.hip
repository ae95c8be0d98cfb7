// ADSB.update (bluesky/traffic/adsbmodel.py:44-59) on the device: the truncated,
// noisy broadcast picture of the traffic (math and the draws' definition:
// bsa_adsb_math.h).
//
// k_adsb_draws    the Philox words, unit normals and uniform of a range of indices
// k_adsb          one update: over host-given arrays (bsa_adsb_update), or this
//                 rank's rows of the resident step (adsb_sim_launch)
//
// One lane per aircraft, no shared state.  A lane whose aircraft is due reads its
// seven state values and writes the seven picture values: 64 B in, 64 B out with
// lastupdate.  Only with per-aircraft noise does it draw (one Philox block, two
// log / sqrt, sincos + cos); the shared draw of the default mode is made once, by
// a one-lane k_adsb_draws launch in front, and read like given normals.  A lane
// that is not due reads lastupdate and nothing else; in the resident step it also
// stores it, into the other lastupdate buffer: 8 B in, 8 B out (bsa_adsb_update
// works in place and stores nothing for it).
#include <cmath>
#include <vector>

#include "bsa_adsb_math.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kAdsbBlock = 256;
constexpr int kAdsbFields = 7;  // lat lon alt trk tas gs vs

struct AdsbArgs {
  int rb, re;                           // rows [rb, re)
  const double *st[kAdsbFields];        // traf.lat lon alt trk tas gs vs
  const double *last_in;                // lastupdate before the call ...
  double *last_out;                     // ... and after it (may be last_in: then only due rows are written)
  double *pic[kAdsbFields];             // adsb.lat lon alt trk tas gs vs
  double time, trunctime, sigma[2];     // transerror: lat / lon [deg], alt [m]
  int noise, per_aircraft;
  const double *zin;                    // given unit normals lat | lon | alt, zstride apart (shared: 3 values), or NULL
  long long zstride;
  unsigned long long seed, call, first;  // the draws of (seed, call); first: the aircraft index of row 0 without h2id
  const unsigned *h2id;                 // resident step: home row -> aircraft index
  const unsigned *sticky;               // resident step: the batch's sticky word
};

__global__ __launch_bounds__(kAdsbBlock) void k_adsb(AdsbArgs a) {
  if (a.sticky && *a.sticky != 0u) return;
  const int h = a.rb + blockIdx.x * kAdsbBlock + threadIdx.x;
  if (h >= a.re) return;
  const double last = a.last_in[h];
  const bool up = adsb::due(last, a.trunctime, a.time);
  if (up)
    a.last_out[h] = last + a.trunctime;  // (not `time`: an aircraft far behind catches up one period per call)
  else if (a.last_out != a.last_in)
    a.last_out[h] = last;
  if (!up) return;
  double v[kAdsbFields];
#pragma unroll
  for (int q = 0; q < kAdsbFields; ++q) v[q] = a.st[q][h];
  if (a.noise) {
    double z[3];
    if (a.zin) {
      const long long i = a.per_aircraft ? (long long)(h - a.rb) : 0;
      for (int q = 0; q < 3; ++q) z[q] = a.zin[q * a.zstride + i];
    } else {
      // (per aircraft only: the shared draw comes in through zin, adsb_shared_draw)
      const unsigned long long idx = a.h2id ? (unsigned long long)a.h2id[h] : a.first + (unsigned long long)(h - a.rb);
      const turb::Draw d = adsb::draw(a.seed, a.call, idx, adsb::kStreamUpdate);
      for (int q = 0; q < 3; ++q) z[q] = d.z[q];
    }
    v[0] = adsb::noisy(v[0], a.sigma[0], z[0]);
    v[1] = adsb::noisy(v[1], a.sigma[0], z[1]);
    v[2] = adsb::noisy(v[2], a.sigma[1], z[2]);
  }
#pragma unroll
  for (int q = 0; q < kAdsbFields; ++q) a.pic[q][h] = v[q];
}

__global__ __launch_bounds__(kAdsbBlock) void k_adsb_draws(long long n, unsigned long long seed,
                                                             unsigned long long call, unsigned long long first,
                                                             unsigned long long stream,
                                                             unsigned long long *__restrict__ raw,
                                                             double *__restrict__ z, double *__restrict__ u) {
  const long long i = (long long)blockIdx.x * kAdsbBlock + threadIdx.x;
  if (i >= n) return;
  const turb::Draw d = adsb::draw(seed, call, first + (unsigned long long)i, stream);
  if (raw)
    for (int q = 0; q < 4; ++q) raw[4 * i + q] = d.b.w[q];
  if (z)
    for (int q = 0; q < 3; ++q) z[3 * i + q] = d.z[q];
  if (u) u[i] = turb::uniform(d.b.w[0]);
}

static unsigned adsb_grid(int64_t n) { return (unsigned)((n + kAdsbBlock - 1) / kAdsbBlock); }

// the settings every entry takes: SetNoise's transerror and trunctime
static int adsb_check(Ctx *c, const char *who, const double *transerror, double trunctime, int noise, int per_aircraft) {
  if (!transerror) return fail(c, "%s: NULL transerror", who);
  for (int k = 0; k < 2; ++k)
    if (!std::isfinite(transerror[k]) || transerror[k] < 0.0)
      return fail(c, "%s: transerror[%d] must be finite and >= 0", who, k);
  if (!std::isfinite(trunctime) || trunctime < 0.0) return fail(c, "%s: trunctime must be finite and >= 0", who);
  if ((noise != 0 && noise != 1) || (per_aircraft != 0 && per_aircraft != 1))
    return fail(c, "%s: noise and per_aircraft must be 0 or 1", who);
  return 0;
}

// The shared draw (the reference's nup = 1): the three normals of index 0 of (seed, call), made once
// by one lane into z3 in front of k_adsb, which reads them as given normals -- not once per due lane
static int adsb_shared_draw(Ctx *c, AdsbArgs *a, double *z3) {
  hipLaunchKernelGGL(k_adsb_draws, dim3(1), dim3(kAdsbBlock), 0, c->stream, 1ll, a->seed, a->call, 0ull,
                     adsb::kStreamUpdate, (unsigned long long *)nullptr, z3, (double *)nullptr);
  BSA_HIP(c, hipGetLastError());
  a->zin = z3;
  a->zstride = 1;
  return 0;
}

static DevBuf &adsb_last(Ctx *c, int which) { return which ? c->s_adlast1 : c->s_adlast0; }
static void adsb_picture(Ctx *c, DevBuf *out[kAdsbFields]) {
  DevBuf *p[kAdsbFields] = {&c->s_adlat, &c->s_adlon, &c->s_adalt, &c->s_adtrk, &c->s_adtas, &c->s_adgs, &c->s_advs};
  for (int q = 0; q < kAdsbFields; ++q) out[q] = p[q];
}
// traf.lat lon alt trk tas gs vs of the resident sim
static void adsb_state(Ctx *c, const double *out[kAdsbFields]) {
  const DevBuf *s[kAdsbFields] = {&c->own[0], &c->own[1], &c->own[4], &c->own[2], &c->s_tas, &c->own[3], &c->own[5]};
  for (int q = 0; q < kAdsbFields; ++q) out[q] = (const double *)s[q]->p;
}

int adsb_sim_launch(Ctx *c, double t) {
  const int64_t rb = c->sim_rb, re = c->sim_re;
  if (rb < 0 || re > c->n || c->n > 0x7fffffff)
    return fail(c, "internal: ADS-B rows [%lld, %lld) of %lld", (long long)rb, (long long)re, (long long)c->n);
  if (re <= rb) return 0;
  AdsbArgs a{};
  a.rb = (int)rb, a.re = (int)re;
  adsb_state(c, a.st);
  const int cur = c->clk.adsb_cur;
  a.last_in = (const double *)adsb_last(c, cur).p;
  a.last_out = (double *)adsb_last(c, cur ^ 1).p;
  DevBuf *pic[kAdsbFields];
  adsb_picture(c, pic);
  for (int q = 0; q < kAdsbFields; ++q) a.pic[q] = (double *)pic[q]->p;
  a.time = t, a.trunctime = c->ad_trunc, a.sigma[0] = c->ad_sigma[0], a.sigma[1] = c->ad_sigma[1];
  a.noise = c->ad_noise ? 1 : 0, a.per_aircraft = c->ad_per_ac ? 1 : 0;
  a.seed = c->ad_seed, a.call = (unsigned long long)c->clk.adsb_call;
  a.h2id = (const unsigned *)c->h2id.p;
  a.sticky = (const unsigned *)((char *)c->sim_ctl.p + kSimCtlSticky);
  // (the draw's launch writes only its three words, a pure function of seed and call: harmless behind an abort)
  if (a.noise && !a.per_aircraft && adsb_shared_draw(c, &a, (double *)c->ad_shared.p)) return -1;
  hipLaunchKernelGGL(k_adsb, dim3(adsb_grid(re - rb)), dim3(kAdsbBlock), 0, c->stream, a);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

int adsb_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_state *s) {
  if (!c->sim_adsb || m <= 0) return 0;
  // ADSB.create (adsbmodel.py:33-42): lastupdate = -trunctime * rand(), the picture from the new aircraft's state,
  // vs at the 0 the append gave it (already there, like the spare lastupdate buffer's rows)
  std::vector<double> lu((size_t)m);
  for (int64_t k = 0; k < m; ++k)
    lu[(size_t)k] = adsb::create_lastupdate(c->ad_trunc, c->ad_seed, (unsigned long long)c->clk.adsb_call,
                                            (unsigned long long)(n + k));
  const size_t at = (size_t)n * 8, mb = (size_t)m * 8;
  BSA_HIP(c, hipMemcpyAsync((char *)adsb_last(c, c->clk.adsb_cur).p + at, lu.data(), mb, hipMemcpyHostToDevice, c->stream));
  DevBuf *pic[kAdsbFields];
  adsb_picture(c, pic);
  const int field[6] = {0, 1, 2, 7, 3, 6};  // bsa_sim_state's lat lon alt trk tas gs
  for (int q = 0; q < 6; ++q)
    BSA_HIP(c, hipMemcpyAsync((char *)pic[q]->p + at, ptr_at(s, field[q]), mb, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

void adsb_off(Ctx *c) {
  c->sim_adsb = false;
  c->clk.adsb_simt = 0.0, c->clk.adsb_call = 0, c->clk.adsb_cur = 0;
  DevBuf *pic[kAdsbFields];
  adsb_picture(c, pic);
  for (DevBuf *b : pic) release(*b);
  release(c->s_adlast0);
  release(c->s_adlast1);
  release(c->ad_shared);
}

// bsa_sim_set_adsb's enabling: the picture is the current state (vs too), lastupdate the caller's.  The caller
// switches the stage off again (adsb_off) when this fails, so that off keeps meaning no allocation
static int adsb_enable(Ctx *c, double simt, const double *lastupdate) {
  if (!lastupdate) return fail(c, "bsa_sim_set_adsb: NULL lastupdate");
  const size_t N8 = (size_t)c->n * 8;
  DevBuf *pic[kAdsbFields];
  adsb_picture(c, pic);
  const double *st[kAdsbFields];
  adsb_state(c, st);
  hipStream_t s = c->stream;
  if (!ensure(c, c->s_adlast0, N8, "ADS-B lastupdate") || !ensure(c, c->s_adlast1, N8, "ADS-B lastupdate") ||
      !ensure(c, c->ad_shared, 3 * 8, "ADS-B shared draw"))
    return -1;
  for (int q = 0; q < kAdsbFields; ++q)
    if (!ensure(c, *pic[q], N8, "ADS-B picture")) return -1;
  for (int q = 0; q < kAdsbFields; ++q) BSA_HIP(c, hipMemcpyAsync(pic[q]->p, st[q], N8, hipMemcpyDeviceToDevice, s));
  BSA_HIP(c, hipMemsetAsync(c->s_adlast1.p, 0, N8, s));
  HomeBatch up(c, true);
  if (up.add(c->s_adlast0.p, lastupdate, nullptr, 8) || up.run()) return -1;
  c->clk.adsb_simt = simt, c->clk.adsb_call = 0, c->clk.adsb_cur = 0;
  return 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" {

int bsa_adsb_draws(bsa_ctx *cc, int64_t n, uint64_t seed, uint64_t call, uint64_t first_index, int stream,
                   uint64_t *raw4n, double *z3n, double *un) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_adsb_draws: bad n");
  if (stream != 1 && stream != 2) return bsa::fail(c, "bsa_adsb_draws: stream must be 1 (update) or 2 (create)");
  if (n == 0) return 0;
  if (!raw4n && !z3n && !un) return bsa::fail(c, "bsa_adsb_draws: no output");
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  if (!bsa::ensure(c, c->adsb_stage, 8 * N * 8, "ADS-B draws")) return -1;
  unsigned long long *raw = (unsigned long long *)c->adsb_stage.p;
  double *z = (double *)c->adsb_stage.p + 4 * N, *u = z + 3 * N;
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(bsa::k_adsb_draws, dim3(bsa::adsb_grid(n)), dim3(bsa::kAdsbBlock), 0, s, (long long)n,
                     (unsigned long long)seed, (unsigned long long)call, (unsigned long long)first_index,
                     (unsigned long long)stream, raw4n ? raw : (unsigned long long *)nullptr,
                     z3n ? z : (double *)nullptr, un ? u : (double *)nullptr);
  BSA_HIP(c, hipGetLastError());
  if (raw4n) BSA_HIP(c, hipMemcpyAsync(raw4n, raw, 4 * N * 8, hipMemcpyDeviceToHost, s));
  if (z3n) BSA_HIP(c, hipMemcpyAsync(z3n, z, 3 * N * 8, hipMemcpyDeviceToHost, s));
  if (un) BSA_HIP(c, hipMemcpyAsync(un, u, N * 8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}

int bsa_adsb_update(bsa_ctx *cc, int64_t n, double time, double trunctime, int noise, const double *transerror,
                    int per_aircraft, const double *draws, uint64_t seed, uint64_t call, uint64_t first_index,
                    const double *lat, const double *lon, const double *alt, const double *trk, const double *tas,
                    const double *gs, const double *vs, double *lastupdate, double *alat, double *alon, double *aalt,
                    double *atrk, double *atas, double *ags, double *avs) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_adsb_update: bad n");
  if (bsa::adsb_check(c, "bsa_adsb_update", transerror, trunctime, noise, per_aircraft)) return -1;
  if (n == 0) return 0;
  const double *in[bsa::kAdsbFields] = {lat, lon, alt, trk, tas, gs, vs};
  double *out[bsa::kAdsbFields] = {alat, alon, aalt, atrk, atas, ags, avs};
  for (int q = 0; q < bsa::kAdsbFields; ++q)
    if (!in[q] || !out[q]) return bsa::fail(c, "bsa_adsb_update: NULL array");
  if (!lastupdate) return bsa::fail(c, "bsa_adsb_update: NULL lastupdate");
  BSA_HIP(c, hipSetDevice(c->device));
  // stage: the 7 state arrays | lastupdate | the 7 picture arrays | draws: the shared 3 (given, or made in front),
  // or the given 3 n per aircraft
  const size_t N = (size_t)n, N8 = N * 8, nz = !noise ? 0 : per_aircraft ? (draws ? 3 * N : 0) : 3;
  if (!bsa::ensure(c, c->adsb_stage, 15 * N8 + nz * 8, "ADS-B arrays")) return -1;
  double *d = (double *)c->adsb_stage.p;
  hipStream_t s = c->stream;
  bsa::AdsbArgs a{};
  a.rb = 0, a.re = (int)n;
  for (int q = 0; q < bsa::kAdsbFields; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d + q * N, in[q], N8, hipMemcpyHostToDevice, s));
    BSA_HIP(c, hipMemcpyAsync(d + (8 + q) * N, out[q], N8, hipMemcpyHostToDevice, s));
    a.st[q] = d + q * N;
    a.pic[q] = d + (8 + q) * N;
  }
  BSA_HIP(c, hipMemcpyAsync(d + 7 * N, lastupdate, N8, hipMemcpyHostToDevice, s));
  a.last_in = a.last_out = d + 7 * N;
  a.time = time, a.trunctime = trunctime, a.sigma[0] = transerror[0], a.sigma[1] = transerror[1];
  a.noise = noise, a.per_aircraft = per_aircraft;
  a.seed = seed, a.call = call, a.first = first_index;
  if (nz && draws) {
    BSA_HIP(c, hipMemcpyAsync(d + 15 * N, draws, nz * 8, hipMemcpyHostToDevice, s));
    a.zin = d + 15 * N;
    a.zstride = per_aircraft ? (long long)n : 1;
  } else if (nz && bsa::adsb_shared_draw(c, &a, d + 15 * N)) {
    return -1;
  }
  hipLaunchKernelGGL(bsa::k_adsb, dim3(bsa::adsb_grid(n)), dim3(bsa::kAdsbBlock), 0, s, a);
  BSA_HIP(c, hipGetLastError());
  for (int q = 0; q < bsa::kAdsbFields; ++q)
    BSA_HIP(c, hipMemcpyAsync(out[q], d + (8 + q) * N, N8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipMemcpyAsync(lastupdate, d + 7 * N, N8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}

int bsa_sim_set_adsb(bsa_ctx *cc, int on, int noise, const double *transerror, double trunctime, uint64_t seed,
                     int per_aircraft, double simt, const double *lastupdate) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_adsb before bsa_sim_init");
  if (on != 0 && on != 1) return bsa::fail(c, "bsa_sim_set_adsb: on must be 0 or 1");
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  // the stage reads nothing a detect writes and writes nothing a detect reads: every kept detect state stays (bsa_kept.h)
  bsa::invalidate(c, bsa::Change::Adsb);
  if (!on) {
    bsa::adsb_off(c);
    return 0;
  }
  if (bsa::adsb_check(c, "bsa_sim_set_adsb", transerror, trunctime, noise, per_aircraft)) return -1;
  if (!c->sim_adsb && bsa::adsb_enable(c, simt, lastupdate)) {
    bsa::adsb_off(c);
    return -1;
  }
  c->ad_noise = noise != 0, c->ad_per_ac = per_aircraft != 0;
  c->ad_sigma[0] = transerror[0], c->ad_sigma[1] = transerror[1];
  c->ad_trunc = trunctime;
  c->ad_seed = seed;
  c->sim_adsb = true;
  return 0;
}

int bsa_sim_read_adsb(bsa_ctx *cc, double *lastupdate, double *lat, double *lon, double *alt, double *trk, double *tas,
                      double *gs, double *vs, double *simt, int64_t *call) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready || !c->sim_adsb) return bsa::fail(c, "bsa_sim_read_adsb: the ADS-B stage is off");
  BSA_HIP(c, hipSetDevice(c->device));
  if (simt) *simt = c->clk.adsb_simt;
  if (call) *call = c->clk.adsb_call;
  bsa::DevBuf *pic[bsa::kAdsbFields];
  bsa::adsb_picture(c, pic);
  double *dst[bsa::kAdsbFields] = {lat, lon, alt, trk, tas, gs, vs};
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);
  if (lastupdate && down.add(bsa::adsb_last(c, c->clk.adsb_cur).p, nullptr, lastupdate, 8)) return -1;
  for (int q = 0; q < bsa::kAdsbFields; ++q)
    if (dst[q] && down.add(pic[q]->p, nullptr, dst[q], 8)) return -1;
  return down.run();
}

int bsa_sim_adsb_call(bsa_ctx *cc, int64_t *call, const int64_t *set_to) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_adsb_call before bsa_sim_init");
  if (set_to) {
    if (*set_to < 0) return bsa::fail(c, "bsa_sim_adsb_call: negative call number");
    c->clk.adsb_call = *set_to;
  }
  if (call) *call = c->clk.adsb_call;
  return 0;
}

}  // extern "C"
