// The exact evaluation of one candidate pair: the one copy that K1b (k_exact,
// bsa_rank.hip) and the K1b fused into K1a (k_prefilter, bsa_prefilter.hip) use.
#pragma once
#include "bsa_cd_args.h"
#include "bsa_geo_math.h"

#pragma clang fp contract(off)

namespace bsa {

// ------------------------------------------------------------------ K1b pair math (also fused into K1a)
struct PairResult {
  bool conf, los;
  double qdr, dist, tcpa, tin, dcpa;
};

// One (i, j) entry of StateBasedCD.detect + geo.qdrdist_matrix, i != j.
// KWIK (opt-in variant, BSA_FLAG_KWIK): geo.kwikqdrdist_matrix (geo.py:347-363)
// replaces qdrdist_matrix, its metre distance handed over in nm (/ nm) so that
// StateBasedCD.py:22's `* nm` restores metres -- the reference's own detect
// with the geo function swapped (tools/make_golden.py captures exactly that).
template <bool KWIK, bool SC = true>
__device__ __forceinline__ PairResult eval_pair(const RowRec &r, const ColRec &c, double rpz,
                                                double hpz, double tla) {
  PairResult o;
  double qdr, dist_nm;
  if (KWIK) {
    // geo.kwikqdrdist_matrix [i, j]: cavelat at lata[j] + latb[i] (geo.py:355)
    double dist_m;
    kwik_entry(r.lat, r.lon, c.lat, c.lon, c.olat + r.ilat, qdr, dist_m);
    dist_nm = dist_m / kNM;
  } else {
    // geo.qdrdist_matrix (geo.py:118-160)
    qdrdist_entry<SC>(r.lat, r.lon, r.sinlat, r.coslat, r.hemA, c.lat, c.lon, c.sinlat, c.coslat, c.hemA,
                  c.eps, qdr, dist_nm);
  }

  // ---- StateBasedCD.detect (StateBasedCD.py:22-83), off-diagonal entry
  const double dist = dist_nm * kNM + 0.0;
  const double qdrrad = qdr * kD2R;
  double sq, cq;
  sin_cos<SC>(qdrrad, &sq, &cq);
  const double dx = dist * sq;
  const double dy = dist * cq;
  const double du = c.u - r.u;  // own.u[j] - int.u[i]
  const double dv = c.v - r.v;
  double dv2 = du * du + dv * dv;
  dv2 = (fabs(dv2) < 1e-6) ? 1e-6 : dv2;
  const double vrel = sqrt(dv2);
  const double tcpa = -(du * dx + dv * dy) / dv2 + 0.0;
  const double dcpa2 = dist * dist - tcpa * tcpa * dv2;
  const double R2 = rpz * rpz;
  const bool swhorconf = dcpa2 < R2;
  const double dxinhor = sqrt(np_max(0., R2 - dcpa2));
  const double dtinhor = dxinhor / vrel;
  const double tinhor = swhorconf ? tcpa - dtinhor : 1e8;
  const double touthor = swhorconf ? tcpa + dtinhor : -1e8;
  const double dalt = c.alt - r.alt + 0.0;  // own.alt[j] - int.alt[i]
  double dvs = c.vs - r.vs;
  dvs = (fabs(dvs) < 1e-6) ? 1e-6 : dvs;
  const double tcrosshi = (dalt + hpz) / -dvs;
  const double tcrosslo = (dalt - hpz) / -dvs;
  const double tinver = np_min(tcrosshi, tcrosslo);
  const double toutver = np_max(tcrosshi, tcrosslo);
  const double tinconf = np_max(tinver, tinhor);
  const double toutconf = np_min(toutver, touthor);
  o.conf = swhorconf && (tinconf <= toutconf) && (toutconf > 0.0) && (tinconf < tla);
  o.los = (dist < rpz) && (fabs(dalt) < hpz);  // StateBasedCD.py:94
  o.qdr = qdr;
  o.dist = dist;
  o.tcpa = tcpa;
  o.tin = tinconf;
  o.dcpa = sqrt(np_max(dcpa2, 0.0));
  return o;
}

// The outputs of one evaluated candidate with row buckets (B > 0; K1b and the
// fused pass below): a conflict's 48-B record (word 0 = the column's sorted
// position, so K2's fused MVP reads the intruder's state without an id2h
// lookup) and the pair's (column, candidate) entry in its row's conflict /
// LoS bucket, at the slot the row count's atomic returns (a full bucket raises
// k2_demand: the detect is retried with wider buckets)
__device__ __forceinline__ void exact_bucket(const PairResult &o, int row, unsigned oj, unsigned py,
                                             unsigned long long id, int nrows, int B, double *__restrict__ cpay,
                                             unsigned *__restrict__ rowcnt, uint2 *__restrict__ kb,
                                             Counters *__restrict__ cnt) {
  if (o.conf) {
    // the detect's "any conflict" word (the lean K2's MVP gate): the first of the wave's lanes here stores it
    if (__lane_id() == (unsigned)__ffsll((long long)__ballot(1)) - 1u) cnt->any_conf = 1ull;
    double *rec = cpay + id * kPayStride;
    rec[0] = __longlong_as_double((long long)py);
    rec[1] = o.qdr;
    rec[2] = o.dist;
    rec[3] = o.tcpa;
    rec[4] = o.tin;
    rec[5] = o.dcpa;
    const unsigned s = atomicAdd(&rowcnt[row], 1u);
    if (s < (unsigned)B) kb[(size_t)row * B + s] = make_uint2(oj, (unsigned)id);
    else atomicMax(&cnt->k2_demand, (unsigned long long)s + 1);
  }
  if (o.los) {
    const unsigned s = atomicAdd(&rowcnt[nrows + 1 + row], 1u);
    if (s < (unsigned)B) kb[((size_t)nrows + row) * B + s] = make_uint2(oj, (unsigned)id);
    else atomicMax(&cnt->k2_demand, (unsigned long long)s + 1);
  }
}

// One candidate p = (row, sorted column) at slot id: K1b's work for it.
__device__ __forceinline__ void fuse_exact_one(const ExactFuse &xf, uint2 p, unsigned long long id,
                                               Counters *__restrict__ cnt) {
  const unsigned oi = xf.perm_r ? xf.perm_r[p.x] : (unsigned)xf.rb + p.x, oj = xf.perm_c[p.y];
  if (xf.perm_r ? oi == oj : oi == p.y) return;  // an aircraft against itself (never a pair)
  const PairResult o = eval_pair<false, false>(xf.R[p.x], xf.C[p.y], xf.rpz, xf.hpz, xf.tla);  // (sin_cos)
  exact_bucket(o, (int)oi - xf.rb, oj, p.y, id, xf.nrows, xf.B, xf.cpay, xf.rowcnt, xf.kb, cnt);
}

}  // namespace bsa
