// Device-side math of one aircraft's Autopilot.update (LNAV / VNAV guidance and
// waypoint switching), shared by the kernels of bsa_fms.hip.
//
// Autopilot.update / ComputeVNAV    bluesky/traffic/autopilot.py:59-304
// ActiveWaypoint.Reached / calcturn bluesky/traffic/activewpdata.py:31-65
// Route.getnextwp on the route table bluesky/traffic/route.py:778-800
// geo.qdrdist (NOT qdrdist_matrix)   bluesky/tools/geo.py:57-107
// aero.atmos / cas2mach / mach2cas (scalar, the layer table) aero.py:178-368
// aero.vcasormach2tas                aero.py:170-172
// misc.degto180                      bluesky/tools/misc.py:102-104
// Every expression keeps numpy's evaluation order (compile with
// -ffp-contract=off).
#pragma once
#include "bsa_kin_math.h"

#pragma clang fp contract(off)

namespace bsa {
namespace fms {

constexpr double kSteepness = 3000. * kFT / (10. * kNM);  // autopilot.py:21
constexpr int kRouteCols = 8;  // lat, lon, alt, spd, xtoalt, toalt, flyby, nextqdr

// geo.qdrdist (geo.py:57-107) of one pair: the radius at the MEAN latitude,
// res2 in its weighted form, r = sw res1 + (1 - sw) res2 as written (two
// latitudes of exactly 0 give 0 / 0 = NaN in res2 and 0 * NaN = NaN in r, as
// numpy does).  qdr [deg], dist [nm].
__device__ __forceinline__ void qdrdist(double latd1, double lond1, double latd2, double lond2, double &qdr,
                                        double &dist_nm) {
  const double res1 = rwgs84(0.5 * (latd1 + latd2));
  const double a = kWGS84_A;
  const double lat1 = latd1 * kD2R, lon1 = lond1 * kD2R;
  const double lat2 = latd2 * kD2R, lon2 = lond2 * kD2R;
  double sinlat1, coslat1, sinlat2, coslat2;
  sincos(lat1, &sinlat1, &coslat1);
  sincos(lat2, &sinlat2, &coslat2);
  const double r1 = rwgs84_sc(sinlat1, coslat1);  // rwgs84(latd1): the same radians(latd1)
  const double r2 = rwgs84_sc(sinlat2, coslat2);
  const double res2 = (0.5 * (fabs(latd1) * (r1 + a) + fabs(latd2) * (r2 + a))) / (fabs(latd1) + fabs(latd2));
  const double sw = (latd1 * latd2 >= 0.) ? 1.0 : 0.0;
  const double r = sw * res1 + (1 - sw) * res2;
  const double sin1 = sin(0.5 * (lat2 - lat1));
  const double sin2 = sin(0.5 * (lon2 - lon1));
  const double root = sin1 * sin1 + ((coslat1 * coslat2) * sin2) * sin2;
  const double d = (2.0 * r) * atan2(sqrt(root), sqrt(1.0 - root));
  double sdl, cdl;
  sincos(lon2 - lon1, &sdl, &cdl);
  qdr = atan2(sdl * coslat2, coslat1 * sinlat2 - (sinlat1 * coslat2) * cdl) * kR2D;
  dist_nm = d / kNM;
}

__device__ __forceinline__ double degto180(double angle) { return np_rem(angle + 180., 360.) - 180.; }

// ActiveWaypoint.calcturn (activewpdata.py:57-65)
__device__ __forceinline__ void calcturn(double tas, double bank, double wpqdr, double next_wpqdr, double &turndist,
                                         double &turnrad) {
  turnrad = (tas * tas) / (np_max(0.01, tan(bank)) * kin::kG0);
  turndist = fabs(turnrad * tan((0.5 * fabs(degto180(np_rem(wpqdr, 360.) - np_rem(next_wpqdr, 360.)))) * kD2R));
}

// aero.atmos (aero.py:178-239): the scalar layer table; T and p only (rho = p / (R T))
__device__ __forceinline__ void atmos(double hin, double &p, double &rho, double &T) {
  static constexpr double h0[8] = {0.0, 11000., 20000., 32000., 47000., 51000., 71000., 86852.};
  static constexpr double p0[7] = {101325., 22631.7009099, 5474.71768857, 867.974468302, 110.898214043, 66.939, 3.9564};
  static constexpr double T0[7] = {288.15, 216.65, 216.65, 228.65, 270.65, 270.65, 214.65};
  static constexpr double a[7] = {-0.0065, 0, 0.001, 0.0028, 0, -0.0028, -0.002};
  // max(0.0, min(float(h), h0[-1])) with Python's min / max (the first argument unless the other is smaller / larger)
  const double hm = h0[7] < hin ? h0[7] : hin;
  const double h = hm > 0.0 ? hm : 0.0;
  int i = 0;
  while (h > h0[i + 1] && i < 6) i = i + 1;
  if (a[i] == 0) {
    T = T0[i];
    p = p0[i] * exp((-kin::kG0 / (kin::kRgas * T)) * (h - h0[i]));
  } else {
    T = T0[i] + a[i] * (h - h0[i]);
    p = p0[i] * pow(T / T0[i], -kin::kG0 / (a[i] * kin::kRgas));
  }
  rho = p / (kin::kRgas * T);
}
// aero.py:304-368 cas2mach = tas2mach(cas2tas), mach2cas = tas2cas(mach2tas), vsound by temp() = atmos's T
__device__ __forceinline__ double cas2mach(double cas, double h) {
  double p, rho, T;
  atmos(h, p, rho, T);
  const double qdyn = kin::kP0 * (pow(1. + kin::kRho0 * cas * cas / (7. * kin::kP0), 3.5) - 1.);
  const double tas = sqrt(7. * p / rho * (pow(1. + qdyn / p, 2. / 7.) - 1.));
  return (cas < 0 ? -1 * tas : tas) / sqrt(kin::kGamma * kin::kRgas * T);
}
__device__ __forceinline__ double mach2cas(double M, double h) {
  double p, rho, T;
  atmos(h, p, rho, T);
  const double tas = M * sqrt(kin::kGamma * kin::kRgas * T);
  const double qdyn = p * (pow(1. + rho * tas * tas / (7. * p), 3.5) - 1.);
  const double cas = sqrt(7. * kin::kP0 / kin::kRho0 * (pow(qdyn / kin::kP0 + 1., 2. / 7.) - 1.));
  return tas < 0 ? -1 * cas : cas;
}

// aero.vcasormach2tas (aero.py:170-172, vmach2tas :107-111, vcas2tas :128-136)
__device__ __forceinline__ double vcasormach2tas(double spd, double h) {
  if (fabs(spd) < 1) {
    const double T = np_max(288.15 - 0.0065 * h, kin::kTstrat);
    return spd * sqrt(kin::kGamma * kin::kRgas * T);
  }
  return kin::vcas2tas(spd, h);
}

// One aircraft: the pre-step traffic state ap.update reads, and everything of
// the FMS it reads or writes.
struct Lane {
  double lat, lon, alt, tas, gs, trk, ax, bank;                                   // read only
  double wlat, wlon, nextaltco, xtoalt, spd, vs, turndist, flyby, next_qdr;       // traf.actwp
  double dist2vs, vnavvs, swvnavvs, selspd;                                       // ap.dist2vs .. traf.selspd
  double selvs, apvsdef;                                                          // read only
  double ap_trk, ap_alt, ap_vs, selalt;
  bool swlnav, swvnav, abco, belco;                                               // abco / belco read only
  int iactwp;
};

// The waypoint-switch body for one aircraft that reached its waypoint
// (autopilot.py:78-137) and ComputeVNAV (:207-304).  route: this aircraft's
// rows (64 B each, 16-byte aligned).  ComputeVNAV's writes of ap.alt[i] and
// actwp.vs[i] are not restated: the continuous part overwrites both arrays
// whole in the same tick (:171, :182).
__device__ __forceinline__ void switch_waypoint(Lane &L, const double *route, int nwp, double &qdr) {
  const double oldspd = L.spd;
  // Route.getnextwp (route.py:778-800) on the table
  const bool lnavon = L.iactwp + 1 < nwp;
  if (lnavon) L.iactwp += 1;
  const double2 *row = (const double2 *)(route + (size_t)L.iactwp * kRouteCols);
  const double2 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  const double alt = r1.x, spd = r1.y, xtoalt = r2.x, toalt = r2.y;
  L.xtoalt = xtoalt;
  L.next_qdr = r3.y;
  L.swlnav = L.swlnav && lnavon;       // :86
  L.swvnav = L.swvnav && L.swlnav;     // :89
  L.wlat = r0.x;
  L.wlon = r0.y;
  L.flyby = trunc(r3.x);               // int(flyby)
  if (alt >= -0.01) L.nextaltco = alt;
  if (spd > -990. && L.swlnav && L.swvnav) {
    if (L.abco && spd > 1.0)
      L.spd = cas2mach(spd, L.alt);
    else if (L.belco && 0. < spd && spd <= 1.0)
      L.spd = mach2cas(spd, L.alt);
    else
      L.spd = spd;
  } else {
    L.spd = -999.;
  }
  if (L.swvnav && oldspd > 0.0) L.selspd = oldspd;   // :118-119
  double dummy;
  qdrdist(L.lat, L.lon, L.wlat, L.wlon, qdr, dummy);  // :122
  const double local_next_qdr = L.next_qdr < -900. ? qdr : L.next_qdr;
  calcturn(L.tas, L.bank, qdr, local_next_qdr, L.turndist, dummy);  // without the flyby factor (:132-134)
  // ---- ComputeVNAV(i, toalt, xtoalt)
  if (toalt < 0 || !L.swvnav) {
    L.dist2vs = -999.;
  } else if (L.alt > toalt + 10. * kFT) {
    const double lim = toalt + xtoalt * kSteepness;
    L.nextaltco = lim < L.alt ? lim : L.alt;   // min(alt, lim)
    L.xtoalt = xtoalt;
    L.dist2vs = L.turndist + fabs(L.alt - L.nextaltco) / kSteepness;
  } else if (L.alt < toalt - 10. * kFT) {
    L.nextaltco = toalt;
    L.xtoalt = xtoalt;
    L.dist2vs = 99999. * kNM;
  } else {
    L.dist2vs = -999.;
  }
}

// The FMS part of Autopilot.update (autopilot.py:66-199) for one aircraft.
// off / nwp: its rows of the route table.  The switch body is divergent and
// rare: it sits behind the lane's own reached flag, so a wave without a
// reached lane branches over it (exec = 0).
__device__ __forceinline__ void tick(Lane &L, const double *rows, int off, int nwp) {
  const double coslat = cos(L.lat * kD2R);   // traf.coslat as UpdatePosition left it (traffic.py:482)
  double qdr, distinnm;
  qdrdist(L.lat, L.lon, L.wlat, L.wlon, qdr, distinnm);
  const double dist = distinnm * kNM;
  // ---- ActiveWaypoint.Reached (activewpdata.py:31-54); flyby scales turnrad too (:39)
  {
    const double next_qdr = L.next_qdr < -900. ? qdr : L.next_qdr;
    double turndist, turnrad;
    calcturn(L.tas, L.bank, qdr, next_qdr, turndist, turnrad);
    L.turndist = L.flyby * turndist;
    turnrad = L.flyby * turnrad;
    const bool away = fabs(degto180(np_rem(L.trk, 360.) - np_rem(qdr, 360.))) > 90.;
    const bool incircle = dist < turnrad * 1.01;
    const bool reached = L.swlnav && ((dist < L.turndist) || (away && incircle));
    if (reached) switch_waypoint(L, rows + (size_t)off * kRouteCols, nwp, qdr);
  }
  // ---- continuous guidance (autopilot.py:147-199)
  const double dy = L.wlat - L.lat;
  const double dx = (L.wlon - L.lon) * coslat;
  const double dist2wp = (60. * kNM) * sqrt(dx * dx + dy * dy);
  const bool startdescent = (dist2wp < L.dist2vs) || (L.nextaltco > L.alt);
  const bool vv = L.swvnav && (L.swlnav ? startdescent : (dist <= np_max(185.2, L.turndist)));
  const double t2go2alt = np_max(0., (dist2wp + L.xtoalt) - L.turndist) / np_max(0.5, L.gs);
  L.vs = np_max(kSteepness * L.gs, fabs(L.nextaltco - L.alt) / np_max(1.0, t2go2alt));
  L.vnavvs = vv ? L.vs : L.vnavvs;
  const double selvs = fabs(L.selvs) > 0.1 ? L.selvs : L.apvsdef;
  L.ap_vs = vv ? L.vnavvs : selvs;
  L.ap_alt = vv ? L.nextaltco : L.selalt;
  L.selalt = vv ? L.nextaltco : L.selalt;
  L.ap_trk = L.swlnav ? qdr : L.ap_trk;
  const double nexttas = vcasormach2tas(L.spd, L.alt);
  const double tasdiff = nexttas - L.tas;
  const double absax = fabs(L.ax);
  const double dtspdchg = fabs(tasdiff) / np_max(0.01, absax);
  const double dxspdchg = (((0.5 * kin::npsign(tasdiff)) * absax) * dtspdchg) * dtspdchg + L.tas * dtspdchg;
  const bool usespdcon = (dist2wp < dxspdchg) && (L.spd > -990.) && L.swvnav;
  L.selspd = usespdcon ? L.spd : L.selspd;
  L.swvnavvs = vv ? 1.0 : 0.0;
}

// ---- waypoint recovery after ResumeNav dropped a resopair (asas.py:459-465):
// Route.findact (route.py:1043-1079) and Route.direct (route.py:635-688) on the
// route table.

// Route.findact: the aircraft's best active waypoint, -1 without a route.  The
// search reads lat, lon of each of the aircraft's rows; argmin keeps numpy's
// first minimum (a NaN is its minimum).  tan(bank) of 0 gives time_turn = inf,
// or NaN (never > time_straight) when delhdg is 0 too, as numpy does.
__device__ __forceinline__ int findact(const Lane &L, const double *route, int nwp) {
  if (nwp <= 0) return -1;
  if (nwp == 1) return 0;
  const double coslat = cos(L.lat * kD2R);   // traf.coslat (traffic.py:482)
  int near = 0;
  double best = 0.;
  for (int w = 0; w < nwp; ++w) {
    const double2 r0 = *(const double2 *)(route + (size_t)w * kRouteCols);
    const double dy = r0.x - L.lat;
    const double dx = (r0.y - L.lon) * coslat;
    const double d2 = dx * dx + dy * dy;
    if (w == 0 || d2 < best || (d2 != d2 && best == best)) {
      best = d2;
      near = w;
    }
  }
  int iw = near > L.iactwp ? near : L.iactwp;   // max(iactwp, argmin): never walks back
  if (iw + 1 < nwp) {
    const double2 r0 = *(const double2 *)(route + (size_t)iw * kRouteCols);
    const double dy = r0.x - L.lat;
    const double dx = (r0.y - L.lon) * coslat;
    const double dist2 = dx * dx + dy * dy;
    const double qdr = atan2(dx, dy) * kR2D;
    const double delhdg = fabs(degto180(L.trk - qdr));
    const double vt = L.tas > 0.01 ? L.tas : 0.01;   // max(0.01, tas)
    const double time_turn = (vt * (delhdg * kD2R)) / (kin::kG0 * tan(L.bank));
    const double time_straight = ((sqrt(dist2) * 60.) * kNM) / vt;
    if (time_turn > time_straight) iw += 1;
  }
  return iw;
}

// wpdirfrom[i] of Route.calcfp (route.py:1005-1012) from the table: the leg
// direction out of waypoint i, which is its row's nextqdr; the last waypoint
// repeats the one before it, a one-waypoint route has 0.
__device__ __forceinline__ double wpdirfrom(const double *route, int nwp, int i) {
  if (i + 1 < nwp) return route[(size_t)i * kRouteCols + 7];
  return nwp > 1 ? route[(size_t)(nwp - 2) * kRouteCols + 7] : 0.;
}

// Route.direct to waypoint wpidx, in the order it is written.  ComputeVNAV runs
// BEFORE turndist is updated and is restated whole: Pilot.APorASAS of the same
// step reads ap.alt, which only the next tick overwrites (next_qdr and, outside
// ComputeVNAV, nextaltco stay as they were: direct does not set them).
__device__ __forceinline__ void direct(Lane &L, const double *route, int nwp, int wpidx) {
  L.iactwp = wpidx;
  const double2 *row = (const double2 *)(route + (size_t)wpidx * kRouteCols);
  const double2 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  const double wpalt = r1.x, wpspd = r1.y, xtoalt = r2.x, toalt = r2.y;
  L.wlat = r0.x;
  L.wlon = r0.y;
  L.flyby = r3.x;
  // ---- ComputeVNAV(idx, wptoalt, wpxtoalt) (autopilot.py:207-304)
  if (toalt < 0 || !L.swvnav) {
    L.dist2vs = -999.;
  } else if (L.alt > toalt + 10. * kFT) {
    const double lim = toalt + xtoalt * kSteepness;
    L.nextaltco = lim < L.alt ? lim : L.alt;
    L.xtoalt = xtoalt;
    L.dist2vs = L.turndist + fabs(L.alt - L.nextaltco) / kSteepness;
    const double dy = L.wlat - L.lat;
    const double dx = (L.wlon - L.lon) * cos(L.lat * kD2R);
    const double legdist = (60. * kNM) * sqrt(dx * dx + dy * dy);
    if (legdist < L.dist2vs) {   // the urgent descent
      L.ap_alt = L.nextaltco;
      const double num = legdist + xtoalt;
      const double t2go = (num > 0.1 ? num : 0.1) / (L.gs > 0.01 ? L.gs : 0.01);
      L.vs = (L.nextaltco - L.alt) / t2go;
    } else {
      L.vs = -kSteepness * (L.gs + (L.gs < 0.2 * L.tas ? 1. : 0.) * L.tas);
    }
  } else if (L.alt < toalt - 10. * kFT) {
    L.nextaltco = toalt;
    L.xtoalt = xtoalt;
    L.ap_alt = L.nextaltco;
    L.dist2vs = 99999. * kNM;
    const double dy = L.wlat - L.lat;
    const double dx = (L.wlon - L.lon) * cos(L.lat * kD2R);
    const double legdist = (60. * kNM) * sqrt(dx * dx + dy * dy);
    const double num = legdist + xtoalt;
    const double t2go = (num > 0.1 ? num : 0.1) / (L.gs > 0.01 ? L.gs : 0.01);
    L.vs = np_max(kSteepness * L.gs, (L.nextaltco - L.alt) / t2go);
  } else {
    L.dist2vs = -999.;
  }
  // ---- the speed of the next leg (route.py:651-674)
  if (wpspd > 0.) {
    const double cas = wpspd < 2.0 ? mach2cas(wpspd, wpalt < 0.0 ? L.alt : wpalt) : wpspd;
    L.spd = cas;
    if (L.swvnav) L.selspd = cas;
  } else {
    L.spd = -999.;
  }
  // ---- turndist [nm, as written] with the fixed 25 deg bank (route.py:677-684)
  double qdr, dummy;
  qdrdist(L.lat, L.lon, L.wlat, L.wlon, qdr, dummy);
  const double turnrad = (((L.tas * L.tas) / tan(25. * kD2R)) / kin::kG0) / kNM;
  const double dq = fabs(degto180(qdr - wpdirfrom(route, nwp, wpidx)));
  L.turndist = ((L.flyby > 0.5 ? 1. : 0.) * turnrad) * fabs(tan(0.5 * ((dq > 5. ? dq : 5.) * kD2R)));
  L.swlnav = true;
}

// ResumeNav's recovery of one ownship that lost `count` resopairs in one call:
// findact + direct once per dropped pair, in sequence (the pair is not
// idempotent).  route: this aircraft's rows.  Of the lane it reads lat lon alt
// tas gs trk bank and reads or writes wlat wlon nextaltco xtoalt spd vs
// turndist flyby dist2vs selspd ap_alt swlnav swvnav iactwp.
__device__ __forceinline__ void fms_recover(Lane &L, const double *route, int nwp, int count) {
  for (int q = 0; q < count; ++q) {
    const int iw = findact(L, route, nwp);
    if (iw < 0) return;   // no waypoints: nothing at all, swlnav included
    direct(L, route, nwp, iw);
  }
}

}  // namespace fms
}  // namespace bsa
