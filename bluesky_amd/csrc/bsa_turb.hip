// Turbulence.Woosh (bluesky/traffic/turbulence.py:24-46) on the device
// (math and the draws' definition: bsa_turb_math.h).
//
// k_turb_draws    the Philox words and unit normals of a range of indices
// k_turb_apply    one Woosh over host-given arrays, with given or generated draws
// k_sim_turb      the resident step's Woosh: this rank's rows, after K4'
//
// One lane per aircraft, no shared state: per aircraft one Philox block (40
// 64-bit multiplies), two log / sqrt, three sincos / cos, 32 B read (trk lat
// lon alt, + 4 B of the index map in the step) and 24 B written.
#include <cmath>

#include "bsa_turb_math.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kTurbBlock = 256;

struct TurbScale {
  double s[3];  // sd[k] * sqrt(dt): np.random.normal's scale of turbhf / turbhw / turbalt
};

__global__ __launch_bounds__(kTurbBlock) void k_turb_draws(long long n, unsigned long long seed,
                                                             unsigned long long call, unsigned long long first,
                                                             unsigned long long *__restrict__ raw,
                                                             double *__restrict__ z) {
  const long long i = (long long)blockIdx.x * kTurbBlock + threadIdx.x;
  if (i >= n) return;
  const turb::Draw d = turb::draw(seed, call, first + (unsigned long long)i);
  if (raw)
    for (int q = 0; q < 4; ++q) raw[4 * i + q] = d.b.w[q];
  for (int q = 0; q < 3; ++q) z[3 * i + q] = d.z[q];
}

// zin: the unit normals hf | hw | alt (3 x n), or NULL: aircraft i draws its own
__global__ __launch_bounds__(kTurbBlock) void k_turb_apply(long long n, TurbScale sc, const double *__restrict__ zin,
                                                             unsigned long long seed, unsigned long long call,
                                                             const double *__restrict__ trk,
                                                             const double *__restrict__ coslat,
                                                             double *__restrict__ lat, double *__restrict__ lon,
                                                             double *__restrict__ alt) {
  const long long i = (long long)blockIdx.x * kTurbBlock + threadIdx.x;
  if (i >= n) return;
  double z[3];
  if (zin) {
    z[0] = zin[i];
    z[1] = zin[n + i];
    z[2] = zin[2 * n + i];
  } else {
    const turb::Draw d = turb::draw(seed, call, (unsigned long long)i);
    z[0] = d.z[0];
    z[1] = d.z[1];
    z[2] = d.z[2];
  }
  double la = lat[i], lo = lon[i], al = alt[i];
  turb::woosh(sc.s, z, trk[i], coslat[i], la, lo, al);
  lat[i] = la;
  lon[i] = lo;
  alt[i] = al;
}

// Home rows [rb, re) after the step's K4': the draw of row h is that of the
// aircraft's index h2id[h].  traf.coslat is K4''s sincos of the new latitude
// (kin::step), taken again from the same latitude with the same function.
// Behind the batch's sticky abort word like every kernel that writes state
__global__ __launch_bounds__(kTurbBlock) void k_sim_turb(int rb, int re, TurbScale sc, unsigned long long seed,
                                                           unsigned long long call,
                                                           const unsigned *__restrict__ h2id,
                                                           const unsigned *__restrict__ sticky,
                                                           const double *__restrict__ trk, double *__restrict__ lat,
                                                           double *__restrict__ lon, double *__restrict__ alt) {
  if (*sticky != 0u) return;
  const int h = rb + blockIdx.x * kTurbBlock + threadIdx.x;
  if (h >= re) return;
  const turb::Draw d = turb::draw(seed, call, (unsigned long long)h2id[h]);
  double la = lat[h], lo = lon[h], al = alt[h];
  double sl, cl;
  sincos(la * kD2R, &sl, &cl);
  turb::woosh(sc.s, d.z, trk[h], cl, la, lo, al);
  lat[h] = la;
  lon[h] = lo;
  alt[h] = al;
}

// Turbulence.SetStandards' clamp and np.random.normal's scale, on the host
static int turb_scale(Ctx *c, const char *who, double dt, const double *sd3, TurbScale *out) {
  if (!sd3) return fail(c, "%s: NULL sd", who);
  if (!std::isfinite(dt) || dt < 0.0) return fail(c, "%s: dt must be finite and >= 0", who);
  const double ts = std::sqrt(dt);
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(sd3[k]) || sd3[k] < 0.0) return fail(c, "%s: sd[%d] must be finite and >= 0", who, k);
    const double sd = sd3[k] > 1e-6 ? sd3[k] : 1e-6;  // turbulence.py:22
    out->s[k] = sd * ts;
  }
  return 0;
}

static unsigned turb_grid(int64_t n) { return (unsigned)((n + kTurbBlock - 1) / kTurbBlock); }

int turb_sim_launch(Ctx *c, int64_t rb, int64_t re, const unsigned *sticky, const double *trk, double *lat,
                    double *lon, double *alt) {
  if (rb < 0 || re > c->n || c->n > 0x7fffffff)
    return fail(c, "internal: turbulence rows [%lld, %lld) of %lld", (long long)rb, (long long)re, (long long)c->n);
  if (re <= rb) return 0;
  TurbScale sc;
  if (turb_scale(c, "turbulence", c->simp.simdt, c->turb_sd, &sc)) return -1;
  hipLaunchKernelGGL(k_sim_turb, dim3(turb_grid(re - rb)), dim3(kTurbBlock), 0, c->stream, (int)rb, (int)re, sc,
                     c->turb_seed, (unsigned long long)c->clk.turb_call, (const unsigned *)c->h2id.p, sticky, trk, lat,
                     lon, alt);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

void turb_off(Ctx *c) { c->sim_turb = false, c->clk.turb_call = 0; }

}  // namespace bsa

extern "C" int bsa_turb_draws(bsa_ctx *cc, int64_t n, uint64_t seed, uint64_t call, uint64_t first_index,
                              uint64_t *raw4n, double *z3n) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_turb_draws: bad n");
  if (n == 0) return 0;
  if (!z3n) return bsa::fail(c, "bsa_turb_draws: NULL output");
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  if (!bsa::ensure(c, c->turb_stage, 7 * N * 8, "turbulence draws")) return -1;
  unsigned long long *raw = (unsigned long long *)c->turb_stage.p;
  double *z = (double *)c->turb_stage.p + 4 * N;
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(bsa::k_turb_draws, dim3(bsa::turb_grid(n)), dim3(bsa::kTurbBlock), 0, s, (long long)n,
                     (unsigned long long)seed, (unsigned long long)call, (unsigned long long)first_index,
                     raw4n ? raw : (unsigned long long *)nullptr, z);
  BSA_HIP(c, hipGetLastError());
  if (raw4n) BSA_HIP(c, hipMemcpyAsync(raw4n, raw, 4 * N * 8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipMemcpyAsync(z3n, z, 3 * N * 8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}

extern "C" int bsa_turb_apply(bsa_ctx *cc, int64_t n, double dt, const double *sd3, const double *hf,
                              const double *hw, const double *valt, uint64_t seed, uint64_t call, const double *trk,
                              const double *coslat, double *lat, double *lon, double *alt) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_turb_apply: bad n");
  bsa::TurbScale sc;
  if (bsa::turb_scale(c, "bsa_turb_apply", dt, sd3, &sc)) return -1;
  const bool given = hf || hw || valt;
  if (given && !(hf && hw && valt)) return bsa::fail(c, "bsa_turb_apply: all three draw arrays or none");
  if (n == 0) return 0;
  if (!trk || !coslat || !lat || !lon || !alt) return bsa::fail(c, "bsa_turb_apply: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N = (size_t)n, N8 = N * 8;
  if (!bsa::ensure(c, c->turb_stage, 8 * N8, "turbulence arrays")) return -1;
  double *d = (double *)c->turb_stage.p;  // trk coslat lat lon alt | hf hw alt draws
  hipStream_t s = c->stream;
  const double *in[5] = {trk, coslat, lat, lon, alt};
  for (int q = 0; q < 5; ++q) BSA_HIP(c, hipMemcpyAsync(d + q * N, in[q], N8, hipMemcpyHostToDevice, s));
  if (given) {
    const double *zs[3] = {hf, hw, valt};
    for (int q = 0; q < 3; ++q) BSA_HIP(c, hipMemcpyAsync(d + (5 + q) * N, zs[q], N8, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(bsa::k_turb_apply, dim3(bsa::turb_grid(n)), dim3(bsa::kTurbBlock), 0, s, (long long)n, sc,
                     given ? (const double *)(d + 5 * N) : (const double *)nullptr, (unsigned long long)seed,
                     (unsigned long long)call, (const double *)d, (const double *)(d + N), d + 2 * N, d + 3 * N,
                     d + 4 * N);
  BSA_HIP(c, hipGetLastError());
  double *out[3] = {lat, lon, alt};
  for (int q = 0; q < 3; ++q) BSA_HIP(c, hipMemcpyAsync(out[q], d + (2 + q) * N, N8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}

extern "C" int bsa_sim_set_turbulence(bsa_ctx *cc, int on, const double *sd3, uint64_t seed) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_turbulence before bsa_sim_init");
  if (on != 0 && on != 1) return bsa::fail(c, "bsa_sim_set_turbulence: on must be 0 or 1");
  bsa::TurbScale sc;
  if (bsa::turb_scale(c, "bsa_sim_set_turbulence", 0.0, sd3, &sc)) return -1;  // (the checks; the step scales by its simdt)
  // records prepared for the next detect and lists kept across detects were made for unperturbed drift (bsa_kept.h)
  bsa::invalidate(c, bsa::Change::Turbulence);
  c->sim_turb = on != 0;
  for (int k = 0; k < 3; ++k) c->turb_sd[k] = sd3[k];
  c->turb_seed = seed;
  return 0;
}

extern "C" int bsa_sim_turb_call(bsa_ctx *cc, int64_t *call, const int64_t *set_to) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_turb_call before bsa_sim_init");
  if (set_to) {
    if (*set_to < 0) return bsa::fail(c, "bsa_sim_turb_call: negative call number");
    c->clk.turb_call = *set_to;
  }
  if (call) *call = c->clk.turb_call;
  return 0;
}
