// ADSB.update (bluesky/traffic/adsbmodel.py:44-59) per aircraft, with
// build-defined draws.  The reference takes its normals
// from numpy's global Mersenne state; here they are Philox4x64-10 blocks
// (bsa_turb_math.h's generator and uniform),
//   counter = {index, call number, stream, 0}, key = {seed, 0},
// stream 1 the update's three normals (lat, lon, alt), stream 2 create's
// uniform; stream 0 is turbulence's, so the stages never share a block.
// fp64, no contraction, numpy's evaluation order (tests/adsb_np.py restates it).
#pragma once
#include "bsa_turb_math.h"

#pragma clang fp contract(off)

namespace bsa {
namespace adsb {

constexpr unsigned long long kStreamUpdate = 1ull, kStreamCreate = 2ull;

// the block of (index, call, stream) and its three unit normals: the Box-Muller pairs of turb::draw
__device__ __forceinline__ turb::Draw draw(unsigned long long seed, unsigned long long call, unsigned long long index,
                                           unsigned long long stream) {
  turb::Draw d;
  d.b = turb::philox4x64_10(index, call, stream, 0ull, seed, 0ull);
  const double u0 = turb::uniform(d.b.w[0]), u1 = turb::uniform(d.b.w[1]), u2 = turb::uniform(d.b.w[2]),
               u3 = turb::uniform(d.b.w[3]);
  const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
  double s0, c0;
  sincos((2.0 * kPI) * u1, &s0, &c0);
  d.z[0] = r0 * c0;
  d.z[1] = r0 * s0;
  d.z[2] = r1 * cos((2.0 * kPI) * u3);
  return d;
}

// create's lastupdate (adsbmodel.py:36): -trunctime * rand(), rand() the uniform of the block's first word
__host__ __device__ __forceinline__ double create_lastupdate(double trunctime, unsigned long long seed,
                                                             unsigned long long call, unsigned long long index) {
  const turb::Block b = turb::philox4x64_10(index, call, kStreamCreate, 0ull, seed, 0ull);
  return -trunctime * turb::uniform(b.w[0]);
}

// adsbmodel.py:45: strict, false for a NaN
__host__ __device__ __forceinline__ bool due(double lastupdate, double trunctime, double time) {
  return lastupdate + trunctime < time;
}

// np.random.normal(0, sigma) is 0 + sigma * z; the sum with the state is a second rounding (adsbmodel.py:48-50)
__host__ __device__ __forceinline__ double noisy(double x, double sigma, double z) {
  const double e = 0.0 + sigma * z;
  return x + e;
}

}  // namespace adsb
}  // namespace bsa
