// Turbulence.Woosh (bluesky/traffic/turbulence.py:24-46) per aircraft, with
// build-defined draws: the reference draws three normal
// arrays from numpy's global Mersenne state, which is serial; here every
// aircraft of every call owns one Philox4x64-10 block,
//   counter = {aircraft index, call number, 0, 0}, key = {seed, 0},
// so the draws are a pure function of (seed, call, index) -- independent of
// the home order, the rank count, the batching and an abort's re-run.
// fp64, no contraction, numpy's evaluation order (tests/turb_np.py restates it).
#pragma once
#include <cstdint>

#include "bsa_internal.h"

#pragma clang fp contract(off)

namespace bsa {
namespace turb {

constexpr double kRearth = 6371000.;  // aero.py:28

struct Block {
  unsigned long long w[4];
};

// Philox4x64-10 (Salmon et al., SC'11; the constants of Random123 and numpy)
__host__ __device__ __forceinline__ unsigned long long mulhi64(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}
__host__ __device__ __forceinline__ Block philox4x64_10(unsigned long long c0, unsigned long long c1,
                                                        unsigned long long c2, unsigned long long c3,
                                                        unsigned long long k0, unsigned long long k1) {
  constexpr unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  constexpr unsigned long long W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long hi0 = mulhi64(M0, c0), lo0 = M0 * c0;
    const unsigned long long hi1 = mulhi64(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Block{{c0, c1, c2, c3}};
}

// u = ((w >> 11) + 0.5) * 2^-53: never 0, so log(u) is finite; in (0, 1] -- from 2^52 up the + 0.5 rounds
// to even, like numpy's float64 add
__host__ __device__ __forceinline__ double uniform(unsigned long long w) {
  return ((double)(w >> 11) + 0.5) * 0x1.0p-53;
}

// the aircraft's block and its three unit normals: two Box-Muller pairs,
// z0 / z1 the cosine / sine branch of (u0, u1), z2 the cosine branch of (u2, u3)
struct Draw {
  Block b;
  double z[3];
};
__device__ __forceinline__ Draw draw(unsigned long long seed, unsigned long long call, unsigned long long index) {
  Draw d;
  d.b = philox4x64_10(index, call, 0ull, 0ull, seed, 0ull);
  const double u0 = uniform(d.b.w[0]), u1 = uniform(d.b.w[1]), u2 = uniform(d.b.w[2]), u3 = uniform(d.b.w[3]);
  const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
  double s0, c0;
  sincos((2.0 * kPI) * u1, &s0, &c0);
  d.z[0] = r0 * c0;
  d.z[1] = r0 * s0;
  d.z[2] = r1 * cos((2.0 * kPI) * u3);
  return d;
}

// turbulence.py:28-46 on one aircraft.  scale[k] = sd[k] * sqrt(dt) (the host's
// product, np.random.normal's scale); z: the unit normals of hf / hw / alt.
// trk: the post-step track; coslat: traf.coslat as UpdatePosition left it
// (traffic.py:482), cos(deg2rad(lat)) of the latitude before the perturbation
__device__ __forceinline__ void woosh(const double scale[3], const double z[3], double trk, double coslat,
                                      double &lat, double &lon, double &alt) {
  const double turbhf = scale[0] * z[0];
  const double turbhw = scale[1] * z[1];
  const double turbalt = scale[2] * z[2];
  double st, ct;
  sincos(trk * kD2R, &st, &ct);
  const double turblat = ct * turbhf - st * turbhw;
  const double turblon = st * turbhf + ct * turbhw;
  alt = alt + turbalt;
  lat = lat + (turblat / kRearth) * kR2D;
  lon = lon + ((turblon / kRearth) / coslat) * kR2D;
}

}  // namespace turb
}  // namespace bsa
