// One wave of points against one shape of the area table: the wave-level cull
// and the inside test with a polygon's ring staged through LDS.  Shared by the
// area filter's kernel (bsa_area.hip, k_area_inside) and the geovector kernel
// (bsa_geovec.hip, k_geovec); the per-point tests are bsa_area_math.h's.
//
// One lane per point, one wave per workgroup: the cull and the LDS chunk are
// the wave's own.  Every lane of the workgroup calls these functions with the
// same shape (a polygon's __syncthreads), lanes past the end with a NaN point.
#pragma once
#include "bsa_area_math.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kAreaBlock = 64;  // one wave: the cull and the LDS chunk are the wave's own
constexpr int kAreaChunk = 64;  // ring vertices in LDS at a time (1 KiB)

__device__ __forceinline__ double wave_uniform(double v) {  // (equal on every lane already: tell the compiler)
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
// min / max over the wave, NaNs left out (fmin / fmax return the other operand)
__device__ __forceinline__ double wave_min(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return wave_uniform(v);
}
__device__ __forceinline__ double wave_max(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return wave_uniform(v);
}

// the lat / lon / alt intervals of the wave's points
struct WaveBounds {
  double lat0, lat1, lon0, lon1, alt0, alt1;
};
__device__ __forceinline__ WaveBounds wave_bounds(double lat, double lon, double alt) {
  return {wave_min(lat), wave_max(lat), wave_min(lon), wave_max(lon), wave_min(alt), wave_max(alt)};
}
// no point of the wave can be inside a shape whose cull bounds (area_pack) the wave's intervals do not meet.
// No comparison with a NaN interval end is true: such a wave skips nothing
__device__ __forceinline__ bool wave_skips(const WaveBounds &w, const area::Shape &sh) {
  return w.alt1 < sh.bottom || w.alt0 > sh.top || w.lat1 < sh.blat[0] || w.lat0 > sh.blat[1] || w.lon1 < sh.blon[0] ||
         w.lon0 > sh.blon[1];
}

// is the lane's point inside sh?  ring: the workgroup's kAreaChunk vertices of LDS; pt_ok = poly_point_ok(lat, lon)
__device__ __forceinline__ bool wave_shape_inside(const area::Shape &sh, const area::Vert *verts, area::Vert *ring,
                                                  int lane, double lat, double lon, double alt, bool pt_ok) {
  bool in = false;
  if (sh.type == BSA_AREA_BOX) {
    in = area::box_inside(sh, lat, lon, alt);
  } else if (sh.type == BSA_AREA_CIRCLE) {
    in = area::circle_inside(sh, lat, lon, alt);
  } else if (sh.type == BSA_AREA_POLY && sh.nvert >= area::kPolyMinVerts) {
    const area::Vert *r = verts + sh.voff;
    const int nv = sh.nvert;
    double x0 = r[nv - 1].x, y0 = r[nv - 1].y;  // the closing edge first: last vertex -> first
    bool f0 = y0 >= lon;
    for (int base = 0; base < nv; base += kAreaChunk) {
      const int m = nv - base < kAreaChunk ? nv - base : kAreaChunk;
      __syncthreads();  // (the chunk before has been read)
      if (lane < m) ring[lane] = r[base + lane];
      __syncthreads();
      for (int k = 0; k < m; ++k) {
        const double x1 = ring[k].x, y1 = ring[k].y;
        const bool f1 = y1 >= lon;
        in ^= area::edge_toggles(x0, y0, x1, y1, f0, f1, lat, lon);
        x0 = x1;
        y0 = y1;
        f0 = f1;
      }
    }
    in = in && pt_ok && area::in_levels(sh, alt);
  }
  return in;
}

}  // namespace bsa
