// Route edits (ADDWPT / DELWPT / DIRECT): the parts that need
// no device -- the stable grouping of a batch by aircraft, the check and the
// row counts of one aircraft's records, the reference's iactwp rules and the
// backward VNAV pass of Route.calcfp.  Host + device inline, no HIP header: a
// stand-alone CPU program compiles this file with a host compiler
// (tools/route_math_check.cpp).
//
// Route.addwpt / delwpt            bluesky/traffic/route.py:472-613, 808-838
// Route.calcfp (VNAV part)         bluesky/traffic/route.py:1014-1041
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/bsaccel.h"

#if defined(__HIPCC__)
#define BSA_RT_HD __host__ __device__ __forceinline__
#else
#define BSA_RT_HD inline
#endif

namespace bsa {
namespace route {

constexpr int kTypeDest = 3, kTypeCalc = 4, kTypeRunway = 5;  // Route.dest / calcwp / runway
constexpr double kNm = 1852.0;

// Stable grouping: order[] = the batch's record numbers sorted by aircraft,
// records of one aircraft in batch order; gstart[g] .. gstart[g + 1] are group
// g's entries of order[].  Returns the number of groups.
inline int64_t group(int64_t m, const bsa_route_edit_rec *rec, std::vector<int32_t> &order, std::vector<int32_t> &gstart) {
  order.resize((size_t)m);
  for (int64_t q = 0; q < m; ++q) order[(size_t)q] = (int32_t)q;
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return rec[a].aircraft < rec[b].aircraft; });
  gstart.clear();
  for (int64_t q = 0; q < m; ++q)
    if (q == 0 || rec[order[(size_t)q]].aircraft != rec[order[(size_t)q - 1]].aircraft) gstart.push_back((int32_t)q);
  gstart.push_back((int32_t)m);
  return (int64_t)gstart.size() - 1;
}

// One record against a route of n waypoints: BSA_ROUTE_OK or why it is refused
BSA_RT_HD int check(const bsa_route_edit_rec &r, int n) {
  switch (r.op) {
    case BSA_ROUTE_INSERT:
    case BSA_ROUTE_OVERWRITE:
      if (r.wptype == kTypeRunway || r.wptype == kTypeCalc || r.wptype < 0 || r.wptype > kTypeRunway)
        return BSA_ROUTE_ERR_WPTYPE;
      if (!(r.lat - r.lat == 0.) || !(r.lon - r.lon == 0.)) return BSA_ROUTE_ERR_NONFINITE;  // inf - inf, nan: not 0
      if (r.op == BSA_ROUTE_INSERT ? (r.pos < 0 || r.pos > n) : (r.pos < 0 || r.pos >= n)) return BSA_ROUTE_ERR_POS;
      return BSA_ROUTE_OK;
    case BSA_ROUTE_DELETE:
    case BSA_ROUTE_DIRECT: return (r.pos < 0 || r.pos >= n) ? BSA_ROUTE_ERR_POS : BSA_ROUTE_OK;
    default: return BSA_ROUTE_ERR_OP;
  }
}
BSA_RT_HD int count_after(int op, int n) {
  return op == BSA_ROUTE_INSERT ? n + 1 : op == BSA_ROUTE_DELETE ? n - 1 : n;
}

// One aircraft's records in batch order against its route of n0 waypoints:
// each sees the route the one before left.  n_final: the waypoints after the
// last; n_max: the most it holds on the way (the rows its new place needs).
// Returns BSA_ROUTE_OK or the first refusal, its entry of ord[] in *bad.
BSA_RT_HD int plan(const bsa_route_edit_rec *rec, const int32_t *ord, int cnt, int n0, int *n_final, int *n_max,
                   int *bad) {
  int n = n0, top = n0;
  for (int q = 0; q < cnt; ++q) {
    const bsa_route_edit_rec &r = rec[ord[q]];
    const int e = check(r, n);
    if (e != BSA_ROUTE_OK) {
      *bad = q;
      return e;
    }
    n = count_after(r.op, n);
    if (n > top) top = n;
  }
  *n_final = n, *n_max = top;
  return BSA_ROUTE_OK;
}

// iactwp after the record, n_after: the route's waypoints after it.
// Insert: route.py:578-579 (bump_active: AFTER was given and found).
// Delete: route.py:834-837; an emptied route ends at min(iactwp, -1) = -1.
BSA_RT_HD int iactwp_after(int op, int pos, int bump_active, int iactwp, int n_after) {
  if (op == BSA_ROUTE_INSERT) {
    if (bump_active && iactwp >= pos) iactwp += 1;
  } else if (op == BSA_ROUTE_DELETE) {
    if (iactwp > pos) iactwp = iactwp - 1 > 0 ? iactwp - 1 : 0;
    if (n_after - 1 < iactwp) iactwp = n_after - 1;
  }
  return iactwp;
}

// addwpt_data's wrap of the position (route.py:451-452), Python's float %
BSA_RT_HD double pymod(double a, double b) {
  double r = std::fmod(a, b);
  if (r != 0. && (r < 0.) != (b < 0.)) r += b;
  return r;
}
BSA_RT_HD double wrap_lat(double lat) { return pymod(lat + 90., 180.) - 90.; }
BSA_RT_HD double wrap_lon(double lon) { return pymod(lon + 180., 360.) - 180.; }

// The carried state of calcfp's backward loop (route.py:1016-1018)
struct Vnav {
  double toalt = -999., xtoalt = 0.;
};
// Waypoints i = i1 - 1 .. i0 of the loop, in its order of additions.  Entry j =
// i - i0 of each array belongs to waypoint i: alt / type, dist_next = wpdistto[i + 1]
// [nm] (unused for the last waypoint of the route, i == nwp - 1); out: toalt / xtoalt.
BSA_RT_HD void vnav_pass(Vnav &v, int i0, int i1, int nwp, const double *alt, const int *type, const double *dist_next,
                         double *toalt, double *xtoalt) {
  for (int i = i1 - 1; i >= i0; --i) {
    const int j = i - i0;
    if (type[j] == kTypeDest) {
      v.toalt = 0., v.xtoalt = 0.;
    } else if (alt[j] >= 0) {
      v.toalt = alt[j], v.xtoalt = 0.;
    } else if (i != nwp - 1) {
      v.xtoalt += dist_next[j] * kNm;
    } else {
      v.xtoalt = 0.0;
    }
    toalt[j] = v.toalt, xtoalt[j] = v.xtoalt;
  }
}

}  // namespace route
}  // namespace bsa
