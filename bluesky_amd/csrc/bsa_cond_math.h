// Condition.update (bluesky/traffic/conditional.py:25-49), one condition, in
// numpy's order of operations.  Shared by bsa_cond_update (host arrays) and
// k_sim_cond (the resident step's stage); DESIGN.md 3.29.
//
//   actual  = (type == alt) * traf.alt[idx] + (type == spd) * traf.cas[idx]   conditional.py:35-36
//   actdif  = target - actual                                                 :39
//   fired   = actdif * lastdif <= 0.0                                         :40
//   lastdif = actdif   (every condition, fired or not)                        :41
//
// `actual` is the reference's bool * value + bool * value, not a select: for
// finite values the two are the same bits (x * 1.0 + y * 0.0 = x), but a
// non-finite altitude or CAS of the aircraft makes BOTH types' actual NaN, and
// such a condition never fires -- as in the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace bsa {
namespace cond {

constexpr int kAltType = 0, kSpdType = 1;  // conditional.py:10

struct Eval {
  double actdif;
  bool fired;
};

__host__ __device__ __forceinline__ Eval eval(int type, double target, double lastdif, double alt, double cas) {
  const double actual = (type == kAltType ? 1.0 : 0.0) * alt + (type == kSpdType ? 1.0 : 0.0) * cas;
  const double actdif = target - actual;
  return Eval{actdif, actdif * lastdif <= 0.0};  // NaN never fires; an exact 0 fires
}

}  // namespace cond
}  // namespace bsa
