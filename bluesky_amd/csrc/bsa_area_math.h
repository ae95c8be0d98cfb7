// The area filter's inside tests (bluesky/tools/areafilter.py:61-104) per point,
// and the shape table they read.  fp64, no contraction, the
// reference's operation order (tests/area_np.py restates it).
//
//   BOX     lat0 <= lat <= lat1 & lon0 <= lon <= lon1 & bottom <= alt <= top   areafilter.py:72-76
//   CIRCLE  kwikdist(clat, clon, lat, lon) <= r [NM] & bottom <= alt <= top     areafilter.py:88-91, geo.py:288-305
//   POLY    matplotlib's Path.contains_points on (x, y) = (lat, lon): an
//           even-odd crossing count over the closed ring          areafilter.py:101-104
//   LINE    never inside                                                      areafilter.py:57-58
#pragma once
#include <cstdint>

#include "bsa_internal.h"

#pragma clang fp contract(off)

namespace bsa {
namespace area {

constexpr double kRe = 6371000.;  // geo.py:297

// bsa_area_shape as the kernels read it: the caller's record, normalised by
// area_pack (corners and top / bottom sorted) with the cull bounds filled in
using Shape = bsa_area_shape;
static_assert(sizeof(Shape) == 96, "bsa_area_shape is 96 B");

struct Vert {  // one ring vertex: x = lat, y = lon [deg]
  double x, y;
};

__host__ __device__ __forceinline__ bool in_levels(const Shape &s, double alt) {
  return s.bottom <= alt && alt <= s.top;
}

__host__ __device__ __forceinline__ bool box_inside(const Shape &s, double lat, double lon, double alt) {
  return s.c[0] <= lat && lat <= s.c[2] && s.c[1] <= lon && lon <= s.c[3] && in_levels(s, alt);
}

// geo.kwikdist(clat, clon, lat, lon) [NM]: np.radians is a multiplication by pi / 180
__host__ __device__ __forceinline__ double kwikdist_nm(double lata, double lona, double latb, double lonb) {
  const double dlat = (latb - lata) * kD2R;
  const double dlon = (lonb - lona) * kD2R;
  const double cavelat = cos(((lata + latb) * kD2R) * 0.5);
  const double dangle = sqrt(dlat * dlat + dlon * dlon * cavelat * cavelat);
  return kRe * dangle / kNM;
}

__host__ __device__ __forceinline__ bool circle_inside(const Shape &s, double lat, double lon, double alt) {
  return (kwikdist_nm(s.c[0], s.c[1], lat, lon) <= s.c[2]) && in_levels(s, alt);
}

// one edge (x0, y0) -> (x1, y1) of the ring against the point (x, y): does the
// crossing count change?  f0 = (y0 >= y), the caller's from the edge before
__host__ __device__ __forceinline__ bool edge_toggles(double x0, double y0, double x1, double y1, bool f0, bool f1,
                                                      double x, double y) {
  return f0 != f1 && (((y1 - y) * (x0 - x1) >= (x1 - x) * (y0 - y1)) == f1);
}

// a point the path test answers at all: finite x and y, a ring of at least 3 vertices
__host__ __device__ __forceinline__ bool poly_point_ok(double x, double y) {
  return __builtin_isfinite(x) && __builtin_isfinite(y);
}
constexpr int kPolyMinVerts = 3;

// the whole ring, one point (the host's form; the kernel walks the ring in LDS chunks)
__host__ __device__ inline bool poly_inside(const Shape &s, const Vert *v, double lat, double lon, double alt) {
  if (s.nvert < kPolyMinVerts || !poly_point_ok(lat, lon)) return false;
  const Vert *r = v + s.voff;
  double x0 = r[s.nvert - 1].x, y0 = r[s.nvert - 1].y;
  bool f0 = y0 >= lon, in = false;
  for (int k = 0; k < s.nvert; ++k) {
    const double x1 = r[k].x, y1 = r[k].y;
    const bool f1 = y1 >= lon;
    in ^= edge_toggles(x0, y0, x1, y1, f0, f1, lat, lon);
    x0 = x1;
    y0 = y1;
    f0 = f1;
  }
  return in && in_levels(s, alt);
}

}  // namespace area
}  // namespace bsa
