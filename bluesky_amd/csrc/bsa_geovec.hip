// Geovectoring (plugins/geovector.py:76-128) on the device:
// per area an allowed interval for ground speed, track and vertical speed,
// applied to the aircraft inside it by clamping selspd, ap.trk, selvs, selalt.
//
// k_geovec     every aircraft under every geovector of the list, in list order
// k_gv_begin   the resident stage's counters, saved behind the batch's abort word
//
// One lane per aircraft, one wave per workgroup, like k_area_inside: the
// geovectors are a sequential fold per aircraft (a later one reads what an
// earlier one wrote), so the lane walks the list with its four values in
// registers.  The inside test is the area filter's (bsa_area_wave.h): the
// wave-level cull on its lat / lon / alt intervals, a polygon's ring through
// LDS.  vtas2cas costs two pow calls: only lanes inside, only for a given
// bound.  A value is stored only where its bits changed.
#include <cmath>

#include "bsa_area_wave.h"
#include "bsa_kin_math.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kGvCntTot = 0, kGvCntUndo = 4, kGvCntWords = 8;  // Ctx::gv_cnt: changed totals, and as they were before the last application
constexpr int kGvGivenAll = BSA_GEOVEC_GSMIN | BSA_GEOVEC_GSMAX | BSA_GEOVEC_TRK | BSA_GEOVEC_VSMIN | BSA_GEOVEC_VSMAX;

struct GeovecArgs {
  int rb, re;  // aircraft [rb, re) of the arrays
  const double *lat, *lon, *alt, *trk, *vs;
  int ngv;
  const bsa_geovec *gv;
  const area::Shape *shapes;
  const area::Vert *verts;
  int nocull;
  double *out[4];  // selspd ap_trk selvs selalt, read and written
  // the resident stage: out[q][h] as it was goes to undo[q * ustride + h]; behind the batch's sticky abort word.
  // NULL in the stand-alone call
  double *undo;
  long long ustride;
  const unsigned *sticky;
  unsigned long long *changed;  // + aircraft whose out[q] changed, 4 words (or NULL)
};

// degto180 (tools/misc.py:102-104) with numpy's %
__device__ __forceinline__ double degto180(double a) { return np_rem(a + 180., 360.) - 180.; }

__device__ __forceinline__ bool bits_differ(double a, double b) {
  return __double_as_longlong(a) != __double_as_longlong(b);
}

__global__ __launch_bounds__(kAreaBlock) void k_geovec(GeovecArgs a) {
  if (a.sticky && *a.sticky != 0u) return;  // (nothing of an aborted batch's later steps: the undo set stays the aborted step's)
  __shared__ area::Vert ring[kAreaChunk];
  const int lane = threadIdx.x;
  const long long h = (long long)a.rb + (long long)blockIdx.x * kAreaBlock + lane;
  const bool live = h < a.re;
  // a lane past the end holds a NaN aircraft: inside nothing, and left out of the wave's intervals
  const double nan = __longlong_as_double((long long)kNanBits);
  const double lat = live ? a.lat[h] : nan, lon = live ? a.lon[h] : nan, alt = live ? a.alt[h] : nan;
  const double trk = live ? a.trk[h] : nan, vs = live ? a.vs[h] : nan;
  double v0[4], v[4];  // selspd ap_trk selvs selalt: as they came, as they are
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v0[q] = v[q] = live ? a.out[q][h] : nan;
    if (a.undo && live) a.undo[q * a.ustride + h] = v0[q];
  }
  const WaveBounds wb = wave_bounds(lat, lon, alt);
  const bool pt_ok = area::poly_point_ok(lat, lon);
  for (int g = 0; g < a.ngv; ++g) {
    const bsa_geovec G = a.gv[g];  // (the same address on every lane)
    const area::Shape sh = a.shapes[G.shape];
    if (!a.nocull && wave_skips(wb, sh)) continue;  // (the whole wave)
    const bool in = wave_shape_inside(sh, a.verts, ring, lane, lat, lon, alt, pt_ok);
    if (!in) continue;
    if (G.given & BSA_GEOVEC_GSMIN) {
      const double casmin = kin::vtas2cas(G.gsmin, alt);
      if (v[0] < casmin) v[0] = casmin;
    }
    if (G.given & BSA_GEOVEC_GSMAX) {  // (reads the selspd the minimum left)
      const double casmax = kin::vtas2cas(G.gsmax, alt);
      if (v[0] > casmax) v[0] = casmax;
    }
    if (G.given & BSA_GEOVEC_TRK) {
      if (degto180(trk - G.trkmin) < 0) v[1] = G.trkmin;  // left of the minimum
      if (degto180(trk - G.trkmax) > 0) v[1] = G.trkmax;  // right of the maximum: written last
    }
    if ((G.given & BSA_GEOVEC_VSMIN) && vs < G.vsmin) {
      v[2] = G.vsmin;
      v[3] = alt + kin::npsign(G.vsmin) * 200. * kFT;  // V/S mode: a selected altitude beyond the present one
    }
    if ((G.given & BSA_GEOVEC_VSMAX) && vs > G.vsmax) {  // (traf.vs, not the selvs just written)
      v[2] = G.vsmax;
      v[3] = alt + kin::npsign(G.vsmax) * 200. * kFT;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool ch = live && bits_differ(v[q], v0[q]);
    if (ch) a.out[q][h] = v[q];
    const unsigned long long b = __ballot(ch);
    if (lane == 0 && b != 0ull && a.changed) atomicAdd(&a.changed[q], (unsigned long long)__popcll(b));
  }
}

// an applying step's first launch: the totals as they are, for batch_rollback to put back
__global__ void k_gv_begin(const unsigned *sticky, unsigned long long *cnt) {
  if (*sticky != 0u) return;
  if (threadIdx.x < 4) cnt[kGvCntUndo + threadIdx.x] = cnt[kGvCntTot + threadIdx.x];
}

static int geovec_launch(Ctx *c, const GeovecArgs &a) {
  if (a.re <= a.rb || a.ngv <= 0) return 0;
  const unsigned grid = (unsigned)(((int64_t)a.re - a.rb + kAreaBlock - 1) / kAreaBlock);
  hipLaunchKernelGGL(k_geovec, dim3(grid), dim3(kAreaBlock), 0, c->stream, a);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// every index the kernel uses unguarded, and what the reference would read differently
static int geovec_check(Ctx *c, const char *who, int64_t ngv, const bsa_geovec *gv, int64_t nshapes) {
  if (ngv < 0 || ngv > BSA_GEOVEC_MAX) return fail(c, "%s: %lld geovectors, at most %d", who, (long long)ngv, BSA_GEOVEC_MAX);
  if (ngv > 0 && !gv) return fail(c, "%s: NULL geovector table", who);
  for (int64_t k = 0; k < ngv; ++k) {
    const bsa_geovec &g = gv[k];
    if (g.shape < 0 || g.shape >= nshapes)
      return fail(c, "%s: geovector %lld names shape %d of %lld", who, (long long)k, g.shape, (long long)nshapes);
    if (g.given & ~kGvGivenAll) return fail(c, "%s: geovector %lld: unknown given bits 0x%x", who, (long long)k, g.given);
    const struct {
      int bit;
      double v;
      const char *name;
    } b[6] = {{BSA_GEOVEC_GSMIN, g.gsmin, "gsmin"}, {BSA_GEOVEC_GSMAX, g.gsmax, "gsmax"}, {BSA_GEOVEC_TRK, g.trkmin, "trkmin"},
              {BSA_GEOVEC_TRK, g.trkmax, "trkmax"},  {BSA_GEOVEC_VSMIN, g.vsmin, "vsmin"}, {BSA_GEOVEC_VSMAX, g.vsmax, "vsmax"}};
    for (const auto &q : b)
      if ((g.given & q.bit) && q.v == 0.0)
        return fail(c, "%s: geovector %lld: %s is given and exactly 0, which the reference reads as off", who,
                    (long long)k, q.name);
  }
  return 0;
}

// ---- the resident step's stage
static GeovecArgs gv_sim_args(Ctx *c) {
  const size_t n = (size_t)c->n;
  GeovecArgs a{};
  a.rb = (int)c->sim_rb;
  a.re = (int)c->sim_re;
  a.lat = (const double *)c->own[0].p;
  a.lon = (const double *)c->own[1].p;
  a.alt = (const double *)c->own[4].p;
  a.trk = (const double *)c->own[2].p;
  a.vs = (const double *)c->own[5].p;
  a.ngv = c->gv_n;
  a.gv = (const bsa_geovec *)c->gv_tab.p;
  a.shapes = (const area::Shape *)c->gv_shapes.p;
  a.verts = (const area::Vert *)c->area_verts.p;
  a.nocull = area_env_nocull() ? 1 : 0;
  a.out[0] = (double *)c->s_fmsr.p + 12 * n;  // selspd, selvs: bsa_fms_state's reals 12 and 13
  a.out[1] = (double *)c->s_aptrk.p;
  a.out[2] = (double *)c->s_fmsr.p + 13 * n;
  a.out[3] = (double *)c->s_selalt.p;
  a.undo = (double *)c->gv_undo.p;
  a.ustride = (long long)n;
  a.sticky = (const unsigned *)((const char *)c->sim_ctl.p + kSimCtlSticky);
  a.changed = (unsigned long long *)c->gv_cnt.p + kGvCntTot;
  return a;
}

bool geovec_applies_at(const Ctx *c) { return c->clk.gv_ctr > 0 && c->clk.gv_ctr % c->gv_every == 0; }

int geovec_sim_launch(Ctx *c) {
  // (the aircraft count may have changed since the last application: bsa_sim_delete)
  if (!ensure(c, c->gv_undo, (size_t)c->n * 32, "geovector undo set")) return -1;
  const GeovecArgs a = gv_sim_args(c);
  hipLaunchKernelGGL(k_gv_begin, dim3(1), dim3(64), 0, c->stream, a.sticky, (unsigned long long *)c->gv_cnt.p);
  BSA_HIP(c, hipGetLastError());
  return geovec_launch(c, a);
}

int geovec_sim_restore(Ctx *c) {
  unsigned long long *cnt = (unsigned long long *)c->gv_cnt.p;
  BSA_HIP(c, hipMemcpyAsync(cnt + kGvCntTot, cnt + kGvCntUndo, 32, hipMemcpyDeviceToDevice, c->stream));
  const int64_t rb = c->sim_rb, re = c->sim_re;
  if (re <= rb) return 0;
  const GeovecArgs a = gv_sim_args(c);
  for (int q = 0; q < 4; ++q)
    BSA_HIP(c, hipMemcpyAsync(a.out[q] + rb, a.undo + q * a.ustride + rb, (size_t)(re - rb) * 8, hipMemcpyDeviceToDevice,
                              c->stream));
  return 0;
}

void geovec_off(Ctx *c) {
  c->sim_gv = false;
  c->gv_n = 0;
  c->clk.gv_ctr = 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" int bsa_sim_set_geovectors(bsa_ctx *cc, int64_t ngv, const bsa_geovec *gv, int64_t every) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_geovectors before bsa_sim_init");
  if (ngv > 0 && c->area_tab.empty()) return bsa::fail(c, "bsa_sim_set_geovectors: the sim has no areas (bsa_sim_set_areas)");
  if (ngv > 0 && !c->sim_fms)
    return bsa::fail(c, "bsa_sim_set_geovectors needs the FMS guidance (bsa_sim_set_fms): selspd and selvs are its arrays");
  if (ngv > 0 && every < 1) return bsa::fail(c, "bsa_sim_set_geovectors: every must be >= 1");
  if (bsa::geovec_check(c, "bsa_sim_set_geovectors", ngv, gv, (int64_t)c->area_tab.size())) return -1;
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));  // (no stage in flight reads the old tables)
  bsa::geovec_off(c);
  if (ngv == 0) return 0;
  std::vector<bsa_geovec> rows(gv, gv + ngv);
  std::vector<bsa::area::Shape> shapes((size_t)ngv);
  for (int64_t k = 0; k < ngv; ++k) {
    shapes[(size_t)k] = c->area_tab[(size_t)rows[(size_t)k].shape];
    rows[(size_t)k].shape = (int32_t)k;
  }
  if (!bsa::ensure(c, c->gv_tab, rows.size() * sizeof(bsa_geovec), "geovector table") ||
      !bsa::ensure(c, c->gv_shapes, shapes.size() * sizeof(bsa::area::Shape), "geovector shapes") ||
      !bsa::ensure(c, c->gv_undo, (size_t)c->n * 32, "geovector undo set") ||
      !bsa::ensure(c, c->gv_cnt, bsa::kGvCntWords * 8, "geovector counters"))
    return -1;
  hipStream_t s = c->stream;
  BSA_HIP(c, hipMemcpyAsync(c->gv_tab.p, rows.data(), rows.size() * sizeof(bsa_geovec), hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(c->gv_shapes.p, shapes.data(), shapes.size() * sizeof(bsa::area::Shape), hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemsetAsync(c->gv_cnt.p, 0, bsa::kGvCntWords * 8, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  c->gv_n = (int)ngv;
  c->gv_every = every;
  c->sim_gv = true;
  return 0;
}

extern "C" int bsa_sim_geovec_stats(bsa_ctx *cc, int64_t *applies, uint64_t *changed4_total) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready || !c->sim_gv) return bsa::fail(c, "bsa_sim_geovec_stats: no geovectors (bsa_sim_set_geovectors)");
  const int64_t ctr = c->clk.gv_ctr;
  if (applies) *applies = ctr >= 1 ? (ctr - 1) / c->gv_every : 0;  // steps k = every, 2 every, ... < gv_ctr
  if (changed4_total) {
    BSA_HIP(c, hipSetDevice(c->device));
    unsigned long long h[4];
    BSA_HIP(c, hipMemcpyAsync(h, (const unsigned long long *)c->gv_cnt.p + bsa::kGvCntTot, sizeof(h), hipMemcpyDeviceToHost,
                              c->stream));
    BSA_HIP(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < 4; ++q) changed4_total[q] = h[q];
  }
  return 0;
}

extern "C" int bsa_geovec_apply(bsa_ctx *cc, int64_t n, const double *lat, const double *lon, const double *alt,
                                const double *trk, const double *vs, int64_t nshapes, const bsa_area_shape *shapes,
                                int64_t nvert, const double *verts, int64_t ngv, const bsa_geovec *gv, int flags,
                                double *selspd, double *ap_trk, double *selvs, double *selalt, uint64_t *changed) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_geovec_apply: bad n");
  if (flags & ~BSA_AREA_NOCULL) return bsa::fail(c, "bsa_geovec_apply: unknown flag");
  std::vector<bsa::area::Shape> tab;
  if (bsa::area_pack(c, "bsa_geovec_apply", nshapes, shapes, nvert, verts, &tab)) return -1;
  if (bsa::geovec_check(c, "bsa_geovec_apply", ngv, gv, nshapes)) return -1;
  const double *in[5] = {lat, lon, alt, trk, vs};
  double *io[4] = {selspd, ap_trk, selvs, selalt};
  for (auto q : in)
    if (n > 0 && !q) return bsa::fail(c, "bsa_geovec_apply: NULL traffic array");
  for (auto q : io)
    if (n > 0 && !q) return bsa::fail(c, "bsa_geovec_apply: NULL target array");
  if (changed)
    for (int q = 0; q < 4; ++q) changed[q] = 0;
  if (n == 0 || ngv == 0) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  // lat lon alt trk vs | selspd ap_trk selvs selalt | changed | geovectors | shapes | vertices
  const size_t N8 = (size_t)n * 8, gb = (size_t)ngv * sizeof(bsa_geovec), tb = tab.size() * sizeof(bsa::area::Shape),
               vb = (size_t)nvert * 16;
  if (!bsa::ensure(c, c->gv_stage, 9 * N8 + 32 + gb + tb + vb + 16, "geovector arrays")) return -1;
  char *d = (char *)c->gv_stage.p;
  double *dp = (double *)d;
  unsigned long long *dcnt = (unsigned long long *)(d + 9 * N8);
  bsa_geovec *dgv = (bsa_geovec *)(dcnt + 4);
  bsa::area::Shape *dtab = (bsa::area::Shape *)((char *)dgv + gb);
  bsa::area::Vert *dv = (bsa::area::Vert *)((char *)dtab + tb);
  hipStream_t s = c->stream;
  for (int q = 0; q < 5; ++q) BSA_HIP(c, hipMemcpyAsync(dp + (size_t)q * n, in[q], N8, hipMemcpyHostToDevice, s));
  for (int q = 0; q < 4; ++q) BSA_HIP(c, hipMemcpyAsync(dp + (size_t)(5 + q) * n, io[q], N8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemsetAsync(dcnt, 0, 32, s));
  BSA_HIP(c, hipMemcpyAsync(dgv, gv, gb, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(dtab, tab.data(), tb, hipMemcpyHostToDevice, s));
  if (vb) BSA_HIP(c, hipMemcpyAsync(dv, verts, vb, hipMemcpyHostToDevice, s));
  bsa::GeovecArgs a{};
  a.rb = 0;
  a.re = (int)n;
  a.lat = dp;
  a.lon = dp + n;
  a.alt = dp + 2 * (size_t)n;
  a.trk = dp + 3 * (size_t)n;
  a.vs = dp + 4 * (size_t)n;
  a.ngv = (int)ngv;
  a.gv = dgv;
  a.shapes = dtab;
  a.verts = dv;
  a.nocull = ((flags & BSA_AREA_NOCULL) || bsa::area_env_nocull()) ? 1 : 0;
  for (int q = 0; q < 4; ++q) a.out[q] = dp + (size_t)(5 + q) * n;
  a.changed = dcnt;
  if (bsa::geovec_launch(c, a)) return -1;
  for (int q = 0; q < 4; ++q) BSA_HIP(c, hipMemcpyAsync(io[q], a.out[q], N8, hipMemcpyDeviceToHost, s));
  if (changed) BSA_HIP(c, hipMemcpyAsync(changed, dcnt, 32, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}
