// The area filter (bluesky/tools/areafilter.py:29-35, 61-104) on the device
// (tests and the shape table: bsa_area_math.h).
//
// k_area_inside   every point against every shape: bit masks and per-shape counts;
//                 as the resident step's sector pass (plugins/sectorcount.py:53-79)
//                 also the masks before, and who arrived and who left
// k_sect_zero     the sector pass's per-update counts, behind the batch's abort word
//
// One lane per point, one wave per workgroup.  Every wave walks the shapes in
// table order; a polygon's ring passes through LDS in chunks of kAreaChunk
// vertices, so all 64 lanes read the same vertex at the same time (a broadcast
// read: no bank conflicts).  Per point and ring vertex: one 16 B LDS read,
// 4 fp64 subtractions, 2 multiplications, 3 comparisons.  Per point: 24 B read,
// 8 B written per 64 shapes.
//
// The cull: a wave reduces its 64 points' lat / lon / alt intervals once and
// skips a shape whose cull bounds (area_pack) those intervals do not meet.  No
// point of the wave can be inside such a shape, so the masks and counts are
// those of the unculled run, bit for bit (BSA_AREA_NOCULL / env BSA_AREA_CULL=0).
#include <cmath>
#include <cstdlib>
#include <unordered_set>

#include "bsa_area_wave.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kAreaShapesMax = 1024, kAreaVertsMax = 65536;

struct AreaArgs {
  int rb, re;              // points [rb, re) of the arrays
  long long stride;        // mask word w of point h: mask[w * stride + h]
  const double *lat, *lon, *alt;
  int nshapes;
  const area::Shape *shapes;
  const area::Vert *verts;
  int nocull;
  unsigned long long *mask;
  unsigned long long *counts;  // + points inside, per shape (or NULL)
  // the sector pass (<= 64 shapes, one word): mask[h] as it was goes to prev[h]; sect (kSect* words) takes the
  // counts; behind the batch's sticky abort word.  All NULL in the stand-alone call
  unsigned long long *prev;
  unsigned long long *sect;
  const unsigned *sticky;
};
// Ctx::sect_cnt: per sector n_tot / arrived / left of the last update, arrived / left since bsa_sim_set_sectors
constexpr int kSectMax = 64, kSectTot = 0, kSectArr = 64, kSectLeft = 128, kSectArrCum = 192, kSectLeftCum = 256,
              kSectWords = 320;

__global__ void k_sect_zero(const unsigned *sticky, unsigned long long *sect) {
  if (*sticky != 0u) return;
  if (threadIdx.x < kSectArrCum) sect[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kAreaBlock) void k_area_inside(AreaArgs a) {
  if (a.sticky && *a.sticky != 0u) return;  // (like k_sim_turb: nothing of an aborted batch's later steps)
  __shared__ area::Vert ring[kAreaChunk];
  const int lane = threadIdx.x;
  const long long h = (long long)a.rb + (long long)blockIdx.x * kAreaBlock + lane;
  const bool live = h < a.re;
  // a lane past the end holds a NaN point: inside nothing, and left out of the wave's intervals
  const double nan = __longlong_as_double((long long)kNanBits);
  const double lat = live ? a.lat[h] : nan, lon = live ? a.lon[h] : nan, alt = live ? a.alt[h] : nan;
  const WaveBounds wb = wave_bounds(lat, lon, alt);
  const bool pt_ok = area::poly_point_ok(lat, lon);
  unsigned long long word = 0ull;
  for (int s = 0; s < a.nshapes; ++s) {
    const area::Shape sh = a.shapes[s];  // (the same address on every lane)
    const bool skip = !a.nocull && wave_skips(wb, sh);
    bool in = false;
    if (!skip) {
      in = wave_shape_inside(sh, a.verts, ring, lane, lat, lon, alt, pt_ok);
      const unsigned long long b = __ballot(in);
      if (lane == 0 && b != 0ull && a.counts) atomicAdd(&a.counts[s], (unsigned long long)__popcll(b));
    }
    word |= (unsigned long long)(in ? 1 : 0) << (s & 63);
    if (a.prev && s == a.nshapes - 1) {  // the sector pass: what changed against the masks of the update before
      const unsigned long long p = live ? a.mask[h] : 0ull;
      const unsigned long long arr = word & ~p, lef = p & ~word;
      if (live) a.prev[h] = p;
      if (__ballot((arr | lef) != 0ull) != 0ull)
        for (int q = 0; q <= s; ++q) {
          const unsigned long long ba = __ballot((arr >> q) & 1ull), bl = __ballot((lef >> q) & 1ull);
          if (lane == 0 && ba != 0ull) {
            atomicAdd(&a.sect[kSectArr + q], (unsigned long long)__popcll(ba));
            atomicAdd(&a.sect[kSectArrCum + q], (unsigned long long)__popcll(ba));
          }
          if (lane == 0 && bl != 0ull) {
            atomicAdd(&a.sect[kSectLeft + q], (unsigned long long)__popcll(bl));
            atomicAdd(&a.sect[kSectLeftCum + q], (unsigned long long)__popcll(bl));
          }
        }
    }
    if ((s & 63) == 63 || s == a.nshapes - 1) {
      if (live) a.mask[(long long)(s >> 6) * a.stride + h] = word;
      word = 0ull;
    }
  }
}

// BSA_AREA_CULL=0: every shape for every lane (A/B and test aid, read once)
bool area_env_nocull() {
  static const bool off = [] {
    const char *e = getenv("BSA_AREA_CULL");
    return e && e[0] == '0';
  }();
  return off;
}

// The caller's table -> the kernels': every argument checked, top / bottom and
// the box corners sorted as the reference's constructors sort them
// (areafilter.py:64-70, 85-86, 98-99), the cull bounds filled in:
//   altitude   [bottom, top]: the test's own comparison
//   BOX        its sorted corners: the test's own comparisons
//   POLY       lon: [min, max] of the ring's lon.  A point with lon > max has every flag (y_k >= y) false,
//              one with lon < min every flag true: no edge has f0 != f1, the count stays 0.  Comparisons only.
//              lat: [min - m, max + m] of the ring's lat, m ~ 2^-40 of the range: out there the two products of
//              every straddling edge differ by far more than their roundings, so above the range no edge
//              toggles and below it every straddling edge does -- an even number on a closed ring
//   CIRCLE     lat: clat -/+ degrees(r nm / re) widened by 1e-9 relative.  dangle >= sqrt(dlat * dlat) >= |dlat| (1 - 2^-52)
//              because fp64 addition of a non-negative term and sqrt are monotone, so outside the widened band
//              dist > r whatever the handful of 2^-53 roundings did.  lon: none
//   LINE       empty bounds (never inside)
int area_pack(Ctx *c, const char *who, int64_t nshapes, const bsa_area_shape *shapes, int64_t nvert,
              const double *verts, std::vector<area::Shape> *out) {
  if (nshapes < 0 || nshapes > kAreaShapesMax) return fail(c, "%s: %lld shapes, at most %d", who, (long long)nshapes, kAreaShapesMax);
  if (nvert < 0 || nvert > kAreaVertsMax) return fail(c, "%s: %lld vertices, at most %d", who, (long long)nvert, kAreaVertsMax);
  if (nshapes > 0 && !shapes) return fail(c, "%s: NULL shape table", who);
  if (nvert > 0 && !verts) return fail(c, "%s: NULL vertex array", who);
  const double inf = INFINITY;
  out->assign(shapes, shapes + nshapes);
  for (int64_t k = 0; k < nshapes; ++k) {
    area::Shape &s = (*out)[(size_t)k];
    const double top = s.top, bottom = s.bottom;
    s.top = bottom > top ? bottom : top;  // np.maximum / np.minimum propagate a NaN; so do these two lines
    s.bottom = bottom < top ? bottom : top;
    if (top != top || bottom != bottom) s.top = s.bottom = NAN;
    s.blat[0] = s.blon[0] = -inf;
    s.blat[1] = s.blon[1] = inf;
    switch (s.type) {
      case BSA_AREA_LINE:
        s.blat[0] = s.blon[0] = inf;
        s.blat[1] = s.blon[1] = -inf;
        break;
      case BSA_AREA_BOX: {
        for (double v : s.c)
          if (v != v) return fail(c, "%s: shape %lld: a box corner is NaN", who, (long long)k);
        const double la0 = std::min(s.c[0], s.c[2]), la1 = std::max(s.c[0], s.c[2]);
        const double lo0 = std::min(s.c[1], s.c[3]), lo1 = std::max(s.c[1], s.c[3]);
        s.c[0] = s.blat[0] = la0;
        s.c[2] = s.blat[1] = la1;
        s.c[1] = s.blon[0] = lo0;
        s.c[3] = s.blon[1] = lo1;
        break;
      }
      case BSA_AREA_CIRCLE: {
        const double rdeg = (s.c[2] * kNM / area::kRe) * kR2D;
        if (std::isfinite(rdeg) && std::isfinite(s.c[0]) && rdeg >= 0.0) {
          const double w = rdeg * (1.0 + 1e-9) + 1e-300;
          s.blat[0] = s.c[0] - w - std::fabs(s.c[0]) * 1e-15;
          s.blat[1] = s.c[0] + w + std::fabs(s.c[0]) * 1e-15;
        }
        break;
      }
      case BSA_AREA_POLY: {
        if (s.nvert < 1) return fail(c, "%s: shape %lld: a polygon of %d vertices", who, (long long)k, s.nvert);
        if (s.voff < 0 || s.voff > nvert || (int64_t)s.nvert > nvert - s.voff)
          return fail(c, "%s: shape %lld: vertices [%lld, %lld) outside the array of %lld", who, (long long)k,
                      (long long)s.voff, (long long)s.voff + s.nvert, (long long)nvert);
        double lo0 = inf, lo1 = -inf, la0 = inf, la1 = -inf, dymin = inf;
        bool finite = true;
        double yp = verts[2 * (s.voff + s.nvert - 1) + 1];
        for (int64_t v = s.voff; v < s.voff + s.nvert; ++v) {
          const double x = verts[2 * v], y = verts[2 * v + 1];
          finite = finite && std::isfinite(y) && std::isfinite(x);
          lo0 = std::min(lo0, y);
          lo1 = std::max(lo1, y);
          la0 = std::min(la0, x);
          la1 = std::max(la1, x);
          if (y != yp) dymin = std::min(dymin, std::fabs(y - yp));
          yp = y;
        }
        if (!finite) return fail(c, "%s: shape %lld: a vertex is not finite", who, (long long)k);
        s.blon[0] = lo0;
        s.blon[1] = lo1;
        // lat: beyond the ring's lat range by the margin m no edge's comparison is within rounding of equality
        // (DESIGN.md 3.26), given that no edge's lon difference is so small that a product could underflow
        const double m = (la1 - la0) * 0x1.0p-40 + std::max(std::fabs(la0), std::fabs(la1)) * 0x1.0p-40 + 1e-30;
        if (dymin >= 1e-100 && std::isfinite(la1 - la0)) {
          s.blat[0] = la0 - m;
          s.blat[1] = la1 + m;
        }
        break;
      }
      default:
        return fail(c, "%s: shape %lld: unknown type %d", who, (long long)k, s.type);
    }
    if (s.type != BSA_AREA_POLY) {
      s.nvert = 0;
      s.voff = 0;
    }
  }
  return 0;
}

int area_launch(Ctx *c, const AreaArgs &a) {
  if (a.re <= a.rb || a.nshapes <= 0) return 0;
  const unsigned grid = (unsigned)(((int64_t)a.re - a.rb + kAreaBlock - 1) / kAreaBlock);
  hipLaunchKernelGGL(k_area_inside, dim3(grid), dim3(kAreaBlock), 0, c->stream, a);
  BSA_HIP(c, hipGetLastError());
  return 0;
}


// ---- the resident step's sector pass
static AreaArgs sect_args(Ctx *c, bool seed) {
  AreaArgs a{};
  a.rb = (int)c->sim_rb;
  a.re = (int)c->sim_re;
  a.stride = c->n;
  a.lat = (const double *)c->own[0].p;
  a.lon = (const double *)c->own[1].p;
  a.alt = (const double *)c->own[4].p;
  a.nshapes = (int)c->sect_idx.size();
  a.shapes = (const area::Shape *)c->sect_tab.p;
  a.verts = (const area::Vert *)c->area_verts.p;
  a.nocull = area_env_nocull() ? 1 : 0;
  a.mask = (unsigned long long *)c->s_scur.p;
  a.counts = (unsigned long long *)c->sect_cnt.p + kSectTot;
  if (!seed) {
    a.prev = (unsigned long long *)c->s_sprev.p;
    a.sect = (unsigned long long *)c->sect_cnt.p;
    a.sticky = (const unsigned *)((const char *)c->sim_ctl.p + kSimCtlSticky);
  }
  return a;
}

// after the last stage of a step with which the step counter reaches a multiple of the cadence
// (StepPlan::sect_pass).  Reads simulation state only; an aborted batch replays the counter (batch_rollback) and
// the aborted and later steps' passes returned behind the sticky word, so no update is counted twice
int sect_sim_launch(Ctx *c) {
  const AreaArgs a = sect_args(c, false);
  hipLaunchKernelGGL(k_sect_zero, dim3(1), dim3(kSectArrCum), 0, c->stream, a.sticky, a.sect);
  BSA_HIP(c, hipGetLastError());
  if (a.re <= a.rb) return 0;
  return area_launch(c, a);
}

// bsa_sim_delete, before anything moves: the current mask words of this rank's rows among the deleted aircraft
int sect_note_deleted(Ctx *c, int64_t k, const int64_t *idx) {
  if (!c->sim_sect || k <= 0) return 0;
  const int64_t rb = c->sim_rb, re = c->sim_re;
  std::vector<unsigned long long> w((size_t)std::max<int64_t>(re - rb, 0));
  if (!w.empty())
    BSA_HIP(c, hipMemcpy(w.data(), (const unsigned long long *)c->s_scur.p + rb, w.size() * 8, hipMemcpyDeviceToHost));
  std::unordered_set<int64_t> seen;
  for (int64_t q = 0; q < k; ++q) {
    if (idx[q] < 0 || idx[q] >= c->n || !seen.insert(idx[q]).second) continue;  // (once; the caller reports a bad one)
    const int64_t h = c->id2h_h[(size_t)idx[q]];
    if (h >= rb && h < re) c->sect_gone.push_back({q, w[(size_t)(h - rb)]});
  }
  return 0;
}

void sect_off(Ctx *c) {
  c->sim_sect = false;
  c->sect_idx.clear();
  c->sect_gone.clear();
  c->clk.sect_ctr = 0;
}

}  // namespace bsa

extern "C" int bsa_sim_set_areas(bsa_ctx *cc, int64_t nshapes, const bsa_area_shape *shapes, int64_t nvert,
                                 const double *verts) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_areas before bsa_sim_init");
  std::vector<bsa::area::Shape> tab;
  if (bsa::area_pack(c, "bsa_sim_set_areas", nshapes, shapes, nvert, verts, &tab)) return -1;
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));  // (no pass in flight reads the old table)
  bsa::sect_off(c);  // the sectors named shapes of the old table
  bsa::geovec_off(c);  // ... and so did the geovectors
  c->xa_has_shape = false;  // ... and the experiment area, which keeps its arrays: bsa_sim_set_exparea names the new shape
  if (!bsa::ensure(c, c->area_verts, (size_t)std::max<int64_t>(nvert, 1) * 16, "area vertices")) return -1;
  if (nvert) BSA_HIP(c, hipMemcpy(c->area_verts.p, verts, (size_t)nvert * 16, hipMemcpyHostToDevice));
  c->area_tab = tab;
  return 0;
}

extern "C" int bsa_sim_set_sectors(bsa_ctx *cc, int64_t nsect, const int32_t *shape_idx, int64_t every) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_sectors before bsa_sim_init");
  if (nsect < 0 || nsect > bsa::kSectMax) return bsa::fail(c, "bsa_sim_set_sectors: %lld sectors, at most %d", (long long)nsect, bsa::kSectMax);
  if (nsect > 0 && !shape_idx) return bsa::fail(c, "bsa_sim_set_sectors: NULL shape indices");
  if (nsect > 0 && every < 1) return bsa::fail(c, "bsa_sim_set_sectors: every must be >= 1");
  for (int64_t k = 0; k < nsect; ++k)
    if (shape_idx[k] < 0 || (size_t)shape_idx[k] >= c->area_tab.size())
      return bsa::fail(c, "bsa_sim_set_sectors: sector %lld names shape %d of %zu (bsa_sim_set_areas)", (long long)k,
                       shape_idx[k], c->area_tab.size());
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  bsa::sect_off(c);
  if (nsect == 0) return 0;
  std::vector<bsa::area::Shape> tab((size_t)nsect);
  for (int64_t k = 0; k < nsect; ++k) tab[(size_t)k] = c->area_tab[(size_t)shape_idx[k]];
  const size_t NA = (size_t)std::max<int64_t>(c->n, c->sim_rpr * c->nranks) * 8;
  if (!bsa::ensure(c, c->sect_tab, tab.size() * sizeof(bsa::area::Shape), "sector table") ||
      !bsa::ensure(c, c->sect_cnt, bsa::kSectWords * 8, "sector counts") || !bsa::ensure(c, c->s_scur, NA, "sector masks") ||
      !bsa::ensure(c, c->s_sprev, NA, "previous sector masks"))
    return -1;
  hipStream_t s = c->stream;
  BSA_HIP(c, hipMemcpyAsync(c->sect_tab.p, tab.data(), tab.size() * sizeof(bsa::area::Shape), hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemsetAsync(c->sect_cnt.p, 0, bsa::kSectWords * 8, s));
  BSA_HIP(c, hipMemsetAsync(c->s_scur.p, 0, NA, s));
  c->sect_idx.assign(shape_idx, shape_idx + nsect);
  c->sect_every = every;
  // SECTORCOUNT ADD (sectorcount.py:91-96): the previous masks start as one inside pass at the current state
  if (bsa::area_launch(c, bsa::sect_args(c, true))) return -1;
  BSA_HIP(c, hipMemcpyAsync(c->s_sprev.p, c->s_scur.p, NA, hipMemcpyDeviceToDevice, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  c->sim_sect = true;
  return 0;
}

extern "C" int bsa_sim_sectors_poll(bsa_ctx *cc, uint64_t *n_tot, uint64_t *arrived, uint64_t *left,
                                    uint64_t *arrived_total, uint64_t *left_total, int64_t *step, int64_t *updates,
                                    uint64_t *cur_words, uint64_t *prev_words) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready || !c->sim_sect) return bsa::fail(c, "bsa_sim_sectors_poll: no sectors (bsa_sim_set_sectors)");
  BSA_HIP(c, hipSetDevice(c->device));
  unsigned long long h[bsa::kSectWords];
  BSA_HIP(c, hipMemcpyAsync(h, c->sect_cnt.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  uint64_t *dst[5] = {n_tot, arrived, left, arrived_total, left_total};
  const int off[5] = {bsa::kSectTot, bsa::kSectArr, bsa::kSectLeft, bsa::kSectArrCum, bsa::kSectLeftCum};
  for (int q = 0; q < 5; ++q)
    for (size_t k = 0; dst[q] && k < c->sect_idx.size(); ++k) dst[q][k] = h[off[q] + k];
  if (updates) *updates = c->clk.sect_ctr / c->sect_every;
  if (step) *step = c->clk.sect_ctr / c->sect_every * c->sect_every;
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);  // this rank's rows of the masks, index order (NULL: left out)
  if ((cur_words && down.add(c->s_scur.p, nullptr, cur_words, 8)) ||
      (prev_words && down.add(c->s_sprev.p, nullptr, prev_words, 8)))
    return -1;
  return down.run();
}

extern "C" int bsa_sim_sectors_deleted(bsa_ctx *cc, int64_t cap, int64_t *pos, uint64_t *words, int64_t *count) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_sectors_deleted before bsa_sim_init");
  if (cap < 0 || !count || (cap > 0 && (!pos || !words))) return bsa::fail(c, "bsa_sim_sectors_deleted: bad arguments");
  const int64_t m = (int64_t)c->sect_gone.size();
  *count = m;
  if (cap < m) return 0;  // (too small: the count alone; the list stays)
  for (int64_t k = 0; k < m; ++k) {
    pos[k] = c->sect_gone[(size_t)k].pos;
    words[k] = c->sect_gone[(size_t)k].word;
  }
  c->sect_gone.clear();
  return 0;
}

extern "C" int bsa_area_inside(bsa_ctx *cc, int64_t n, const double *lat, const double *lon, const double *alt,
                               int64_t nshapes, const bsa_area_shape *shapes, int64_t nvert, const double *verts,
                               int flags, uint64_t *out_words, uint64_t *counts) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_area_inside: bad n");
  if (flags & ~BSA_AREA_NOCULL) return bsa::fail(c, "bsa_area_inside: unknown flag");
  std::vector<bsa::area::Shape> tab;
  if (bsa::area_pack(c, "bsa_area_inside", nshapes, shapes, nvert, verts, &tab)) return -1;
  if (n > 0 && (!lat || !lon || !alt)) return bsa::fail(c, "bsa_area_inside: NULL point array");
  if (n > 0 && nshapes > 0 && !out_words) return bsa::fail(c, "bsa_area_inside: NULL output");
  if (counts)
    for (int64_t s = 0; s < nshapes; ++s) counts[s] = 0;
  if (n == 0 || nshapes == 0) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N8 = (size_t)n * 8, W = (size_t)(nshapes + 63) / 64;
  const size_t tb = tab.size() * sizeof(bsa::area::Shape), vb = (size_t)nvert * 16, cb = (size_t)nshapes * 8;
  // lat lon alt | mask words (W x n) | counts | shapes | vertices
  if (!bsa::ensure(c, c->area_stage, (3 + W) * N8 + cb + tb + vb + 16, "area filter arrays")) return -1;
  char *d = (char *)c->area_stage.p;
  double *dp = (double *)d;
  unsigned long long *dmask = (unsigned long long *)(d + 3 * N8), *dcnt = dmask + W * (size_t)n;
  bsa::area::Shape *dtab = (bsa::area::Shape *)(dcnt + nshapes);
  bsa::area::Vert *dv = (bsa::area::Vert *)((char *)dtab + tb);
  hipStream_t s = c->stream;
  const double *in[3] = {lat, lon, alt};
  for (int q = 0; q < 3; ++q) BSA_HIP(c, hipMemcpyAsync(dp + (size_t)q * n, in[q], N8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(dtab, tab.data(), tb, hipMemcpyHostToDevice, s));
  if (vb) BSA_HIP(c, hipMemcpyAsync(dv, verts, vb, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemsetAsync(dcnt, 0, cb, s));
  bsa::AreaArgs a{};
  a.rb = 0;
  a.re = (int)n;
  a.stride = n;
  a.lat = dp;
  a.lon = dp + n;
  a.alt = dp + 2 * (size_t)n;
  a.nshapes = (int)nshapes;
  a.shapes = dtab;
  a.verts = dv;
  a.nocull = ((flags & BSA_AREA_NOCULL) || bsa::area_env_nocull()) ? 1 : 0;
  a.mask = dmask;
  a.counts = dcnt;
  if (bsa::area_launch(c, a)) return -1;
  BSA_HIP(c, hipMemcpyAsync(out_words, dmask, W * N8, hipMemcpyDeviceToHost, s));
  if (counts) BSA_HIP(c, hipMemcpyAsync(counts, dcnt, cb, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}
