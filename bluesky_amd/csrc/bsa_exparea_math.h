// The experiment area's per-aircraft update, Area.update (plugins/area.py:112-142),
// expression by expression in numpy's order (fp64, no contraction; tests/exparea_np.py
// restates it).  The inside test itself is the area filter's
// (bsa_area_math.h, bsa_area_wave.h).
//
//   resultantspd = sqrt(gs * gs + vs * vs)                                   area.py:118
//   distance2D  += dt * gs                                                   area.py:119
//   distance3D  += dt * resultantspd                                         area.py:120
//   work        += (thrust * dt) * resultantspd                              area.py:123
//   TAXI OFF:  delalt = (oldalt >= swtaxialt) * (alt < swtaxialt); oldalt = alt   area.py:128-131
//   del         = inside_before * (inside_now == False)                      area.py:141
#pragma once
#include <cstdint>

#include "bsa_internal.h"

#pragma clang fp contract(off)

namespace bsa {
namespace exparea {

// the flag byte of an aircraft: inside at the last update; it left the area in the last update
// (exit delete pending); it sank through swtaxialt in the last update (taxi delete pending)
constexpr uint8_t kInside = 1, kExit = 2, kTaxi = 4;

struct Row {
  double d2, d3, work, oldalt;
};

// the accumulators and oldalt of one aircraft over one update; returns the taxi delete.
// has_thrust false (no OpenAP forces in the step): work stays as it is
__host__ __device__ __forceinline__ bool advance(Row &r, double dt, double gs, double vs, double alt, bool has_thrust,
                                                 double thrust, bool swtaxi, double swtaxialt) {
  const double resultantspd = sqrt(gs * gs + vs * vs);
  r.d2 = r.d2 + dt * gs;
  r.d3 = r.d3 + dt * resultantspd;
  if (has_thrust) r.work = r.work + (thrust * dt) * resultantspd;
  bool delalt = false;
  if (!swtaxi) {
    delalt = (r.oldalt >= swtaxialt) && (alt < swtaxialt);
    r.oldalt = alt;
  }
  return delalt;
}

// the new flag byte from the one before and this update's inside / taxi results
__host__ __device__ __forceinline__ uint8_t flags_after(uint8_t before, bool inside_now, bool delalt) {
  const bool exits = (before & kInside) != 0 && !inside_now;
  return (uint8_t)((inside_now ? kInside : 0) | (exits ? kExit : 0) | (delalt ? kTaxi : 0));
}

// one record of bsa_sim_exparea_poll, per exited aircraft (fp64 words)
constexpr int kRecWords = 19;

}  // namespace exparea
}  // namespace bsa
