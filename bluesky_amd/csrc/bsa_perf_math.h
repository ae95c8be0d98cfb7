// Device-side math of the drag / thrust / fuel-flow half of OpenAP.update,
// shared by the standalone kernel and the resident step's (bsa_perf.hip).
//
// OpenAP.update             bluesky/traffic/performance/openap/perfoap.py:133-173
// compute_thrust_ratio      bluesky/traffic/performance/openap/thrust.py:5-39
// tr_takepff / inflight     thrust.py:41-129
// aero.vatmos / vtas2cas / vtas2mach / vmach2cas  bluesky/tools/aero.py:62-154
// Every expression keeps numpy's evaluation order (compile with
// -ffp-contract=off); np.where chains become ?: chains with the same
// comparisons, so a NaN takes the branch numpy gives it.
#pragma once
#include "bsa_kin_math.h"

namespace bsa {
namespace perf {

// force table (bsa_sim_set_forces, bluesky_amd/perf.py force_table): per type
// Sref engnum engthrust engbpr ff_a ff_b ff_c cd0_clean cd0_gd cd0_to cd0_ic
// cd0_ap cd0_ld k mass 0
constexpr int kForceCols = 16;
// one staged row: the 16 columns + the type's lift type (column 22 of the 24-column table)
constexpr int kStageCols = kForceCols + 1;
// types a staged table may hold (51 KiB of LDS)
constexpr int kForceTypesMax = 384;

enum Phase { NA = 0, TO, IC, CL, CR, DE, AP, LD, GD };  // phase.py:4-12

// thrust.inflight's altitude-independent terms: vpressure(10 000 ft),
// vpressure(35 000 ft), vmach2cas(0.8, 35 000 ft) -- computed once per context
// with the expressions below (k_force_consts)
struct ForceConst {
  double p10, p35, vcas_ref;
};

struct Forces {
  double cd0, drag, thrustratio, thrust, fuelflow, bank;
};

// perfoap.py:135-143
__device__ __forceinline__ double cd0_phase(const double *r, int ph) {
  return ph == TO ? r[9] : ph == IC ? r[10] : ph == AP ? r[11] : ph == LD ? r[12] : ph == GD ? r[8] : r[7];
}

// thrust.py:61-71
__device__ __forceinline__ double dfunc(double mr) {
  return mr < 0.85 ? 0.73
         : mr < 0.92 ? 0.73 + (0.69 - 0.73) / (0.92 - 0.85) * (mr - 0.85)
         : mr < 1.08 ? 0.66 + (0.63 - 0.66) / (1.08 - 1.00) * (mr - 1.00)
         : mr < 1.15 ? 0.63 + (0.60 - 0.63) / (1.15 - 1.08) * (mr - 1.08)
                     : 0.60;
}
// thrust.py:73-75
__device__ __forceinline__ double nfunc(double roc) { return roc < 1500 ? 0.89 : roc < 2500 ? 0.93 : 0.97; }
// thrust.py:77-92
__device__ __forceinline__ double mfunc(double vr, double roc) {
  const double m = vr < 0.67 ? 0.4 : vr < 0.75 ? 0.39 : vr < 0.83 ? 0.38 : vr < 0.92 ? 0.37 : 0.36;
  return roc < 1500 ? m - 0.06 : roc < 2500 ? m - 0.01 : m;
}

// tr_takepff (thrust.py:41-56); p = vpressure(h)
__device__ __forceinline__ double tr_takeoff(double bpr, double v, double h, double p) {
  const double G0 = 0.0606 * bpr + 0.6337;
  const double mach = kin::vtas2mach(v, h);
  const double PP = p / kin::kP0;
  const double PP2 = PP * PP, PP3 = pow(PP, 3.0);
  const double A = -0.4327 * PP2 + 1.3855 * PP + 0.0472;
  const double Z = 0.9106 * PP3 - 1.7736 * PP2 + 1.8697 * PP;
  const double X = 0.1377 * PP3 - 0.4374 * PP2 + 1.3003 * PP;
  return A - 0.377 * (1 + bpr) / sqrt((1 + 0.82 * bpr) * G0) * Z * mach +
         (0.23 + 0.19 * sqrt(bpr)) * X * (mach * mach);
}

// inflight (thrust.py:59-129); p, rho = vatmos(h).  Only the segment
// np.where selects is evaluated (the others' values are discarded there)
__device__ __forceinline__ double inflight(double v, double h, double vs, double thr0, double p, double rho,
                                           const ForceConst &fc) {
  const double roc = fabs(vs / kin::kFPM);
  v = v < 10 ? 10 : v;
  const double mach = kin::vtas2mach(v, h);
  const double F35 = (200 + 0.2 * thr0 / 4.448) * 4.448;
  double ratio;
  if (h > 35000 * kFT) {  // segment 3
    const double mr = mach / 0.8;
    ratio = dfunc(mr) * log(p / fc.p35) + pow(mr, -0.11);
  } else {
    // vtas2cas(v, h) with the shared vatmos (aero.py:139-147)
    const double qdyn = p * (pow(1. + rho * v * v / (7. * p), 3.5) - 1.);
    const double cas = sqrt(7. * kin::kP0 / kin::kRho0 * (pow(qdyn / kin::kP0 + 1., 2. / 7.) - 1.));
    const double vr = (v < 0 ? -1 * cas : cas) / fc.vcas_ref;
    const double a = pow(vr, -0.1);
    const double e = -0.355 * vr + nfunc(roc);
    if (h > 10000 * kFT) {  // segment 2
      ratio = a * pow(p / fc.p35, e);
    } else {  // segment 1
      const double F10 = F35 * a * pow(fc.p10 / fc.p35, e);
      const double m = mfunc(vr, roc);
      ratio = m * (p / fc.p35) + (F10 / F35 - m * (fc.p10 / fc.p35));
    }
  }
  return ratio * F35 / thr0;
}

// the constants of ForceConst (one lane)
__device__ __forceinline__ ForceConst force_consts() {
  ForceConst fc;
  double p, rho, T;
  kin::vatmos(10000 * kFT, p, rho, T);
  fc.p10 = p;
  kin::vatmos(35000 * kFT, p, rho, T);
  fc.p35 = p;
  fc.vcas_ref = kin::vmach2cas(0.8, 35000 * kFT);
  return fc;
}

// perfoap.py:133-173 for one aircraft: r its type's force-table row, lift its
// lift type, ph its flight phase, bank the previous perf.bank.  Anything but a
// fixed wing keeps the zeros the reference leaves (its cd0 is the row's
// cd0_clean: phase NA).  tas == 0 gives drag = NaN as numpy does (0 * inf).
__device__ __forceinline__ Forces forces(const double *r, double lift, int ph, double mass, double tas, double vs,
                                         double alt, double bank, const ForceConst &fc) {
  Forces o;
  o.cd0 = cd0_phase(r, ph);
  o.drag = o.thrustratio = o.thrust = o.fuelflow = 0.0;
  o.bank = (ph == TO || ph == LD) ? 15. : bank;
  o.bank = (ph == IC || ph == CR || ph == AP) ? 35. : o.bank;
  if (lift != 1.0) return o;
  double p, rho, T;
  kin::vatmos(alt, p, rho, T);
  const double rhovs = 0.5 * rho * (tas * tas) * r[0];
  const double cl = mass * kin::kG0 / rhovs;
  o.drag = rhovs * (o.cd0 + r[13] * (cl * cl));
  const double thr0 = r[1] * r[2];
  double tr = 0.0;
  if (ph == TO) tr = tr_takeoff(r[3], tas, alt, p);
  else if (ph == IC || ph == CL || ph == CR) tr = inflight(tas, alt, vs, thr0, p, rho, fc);
  else if (ph == DE) tr = 0.15 * inflight(tas, alt, vs, thr0, p, rho, fc);
  o.thrustratio = tr;
  o.thrust = r[1] * r[2] * tr;
  o.fuelflow = r[1] * (r[4] * (tr * tr) + r[5] * tr + r[6]);
  return o;
}

}  // namespace perf
}  // namespace bsa
