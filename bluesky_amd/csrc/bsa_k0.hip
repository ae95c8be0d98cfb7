// StateBased conflict detection, K0 (pipeline: bsa_cd.hip, DESIGN.md section
// 3): spatial order, records, tile boxes, the tile-pair list and the
// per-detect state's zeroing, with their launchers.
#include <hipcub/hipcub.hpp>

#include "bsa_box.h"
#include "bsa_detect.h"
#include "bsa_geo_math.h"
#include "bsa_halo.h"
#include "bsa_internal.h"
#include "bsa_prep.h"
#include "bsa_wave.h"

#pragma clang fp contract(off)

namespace bsa {

// math helpers (np_max / np_min / np_rem / rwgs84) and the qdrdist entries: bsa_geo_math.h

// ------------------------------------------------------------------ K0a keys
__device__ __forceinline__ unsigned expand10(unsigned v) {
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
// Spatial order key: 3-D Hilbert index (10 bits per axis, Skilling's
// transpose form) of the unit position vector.  Consecutive keys are always
// adjacent cells (no Z-order jumps), so the 64-row groups and 8-column
// sub-groups cut from the sorted order have tighter boxes: ~15% fewer stage-1
// pair tests than Morton order at the 100k box (tools/cull_sim.py).  Any order
// gives identical results; only the culling efficiency depends on it.
__device__ __forceinline__ unsigned curve_key(const double p[3]) {
  unsigned X[3];
  for (int k = 0; k < 3; ++k) {
    if (!(p[k] == p[k]) || isinf(p[k])) return 0xffffffffu;
    int q = (int)((p[k] + 1.0) * 512.0);
    X[k] = (unsigned)(q < 0 ? 0 : (q > 1023 ? 1023 : q));
  }
  // axes -> transposed Hilbert index
  for (unsigned Q = 1u << 9; Q > 1u; Q >>= 1) {
    const unsigned P = Q - 1u;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (X[i] & Q) {
        X[0] ^= P;
      } else {
        const unsigned t = (X[0] ^ X[i]) & P;
        X[0] ^= t;
        X[i] ^= t;
      }
    }
  }
  X[1] ^= X[0];
  X[2] ^= X[1];
  unsigned t = 0;
  for (unsigned Q = 1u << 9; Q > 1u; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1u;
  X[0] ^= t;
  X[1] ^= t;
  X[2] ^= t;
  return (expand10(X[0]) << 2) | (expand10(X[1]) << 1) | expand10(X[2]);
}

// f > 0 (midpoint stage 1): key of the stage-1 point m = p + f (u e + v n)
// (make_pf_mid), so that sorted groups stay compact around the points the
// boxes bound; any order gives identical results
__global__ __launch_bounds__(256) void k_keys(int cnt, int base, const double *__restrict__ lat,
                                              const double *__restrict__ lon, const double *__restrict__ trk,
                                              const double *__restrict__ gs, double f,
                                              unsigned *__restrict__ key,
                                              unsigned *__restrict__ idx) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const int o = base + k;
  const double la = lat[o] * kD2R, lo = lon[o] * kD2R;
  double cl, sl, co, so;
  sincos(la, &sl, &cl);
  sincos(lo, &so, &co);
  double p[3] = {cl * co, cl * so, sl};
  if (f > 0.0) {
    const double t = trk[o] * kD2R, g = gs[o];
    double st, ct;
    sincos(t, &st, &ct);
    const double u = g * st, v = g * ct;
    const double m[3] = {p[0] + f * (-u * so - v * sl * co), p[1] + f * (u * co - v * sl * so), p[2] + f * (v * cl)};
    if (isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]))
      for (int q = 0; q < 3; ++q) p[q] = m[q];
  }
  key[k] = curve_key(p);
  idx[k] = (unsigned)o;
}

// Row records, sorted position k -> original row perm[k]: own[i] geometry,
// intruder[i] velocity / altitude (StateBasedCD.py:39-40,65-69 orientation).
__global__ __launch_bounds__(256) void k_prep_rows(int cnt, const unsigned *__restrict__ perm,
                                                   SoA6 own, SoA6 intr, double rpz, double hpz,
                                                   double tla, RowRec *__restrict__ R,
                                                   PFRec *__restrict__ PR, PFVel *__restrict__ PV,
                                                   float4 *__restrict__ PP, int mid, uint8_t *__restrict__ rowbad,
                                                   int rb) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const int o = (int)perm[k];
  const double tlap = tla > 0.0 ? tla : 0.0;
  const double la = own.lat[o], lo = own.lon[o];
  const double rad = la * kD2R;
  double sinl, cosl;
  sincos(rad, &sinl, &cosl);
  const double trk = intr.trk[o] * kD2R;
  const double gs = intr.gs[o];
  RowRec r;
  r.lat = la;
  r.lon = lo;
  r.sinlat = sinl;
  r.coslat = cosl;
  r.hemA = fabs(la) * (rwgs84_sc(sinl, cosl) + kWGS84_A);  // geo.py:127
  double st, ct;
  sincos(trk, &st, &ct);
  r.u = gs * st;                                 // StateBasedCD.py:36-37
  r.v = gs * ct;
  r.alt = intr.alt[o];
  r.vs = intr.vs[o];
  r.pad0 = 0.0;
  r.ilat = intr.lat[o];
  for (int q = 0; q < 5; ++q) r.pad[q] = 0.0;
  R[k] = r;
  const double lor = lo * kD2R;
  double coslo, sinlo;
  sincos(lor, &sinlo, &coslo);
  const double px = cosl * coslo, py = cosl * sinlo, pz = sinl;
  const PFRec p = mid ? make_pf_mid(px, py, pz, sinl, cosl, coslo, sinlo, r.u, r.v, gs, r.alt, r.vs, rpz, hpz, tlap)
                      : make_pf(px, py, pz, reach_h(rpz, gs, tlap), r.alt, reach_v(hpz, r.vs, r.alt, tlap));
  PP[k] = make_float4((float)px, (float)py, (float)pz, 0.f);
  PFVel v;
  v.u = (float)r.u;
  v.v = (float)r.v;
  v.vs = (float)r.vs;
  // within ~0.6 deg of a pole (or |lat| > 90: the refine's local east / north
  // basis is ill-conditioned), or a non-finite position: never refine
  v.flags = (!(cosl > 1e-2) || !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) ? 1u : 0u;
  // every tcpa of the row, hence its tcpamax, is NaN (K2; rows in index order)
  rowbad[o - rb] = (isfinite(la) && isfinite(lo) && isfinite(r.u) && isfinite(r.v)) ? 0 : 1;
  PR[k] = p;
  PV[k] = v;
}

// Column records: intruder[j] geometry, own[j] velocity / altitude.
// Workgroup = kTile lanes (one tile of sorted records).  rec = 0 (the
// resident sim's home order): the fp64 records are not stored -- K1b builds
// the few it needs from the state arrays with col_record itself.
// presorted: the state arrays are already in sorted (home) order, perm only
// names the aircraft (the resident sim): record k reads index k, coalesced.
// Tiles: workgroup b prepares tile tile_base + b, or tile_list[b] (a halo
// tile list of the row-sharded step, -1 = unused slot).
// (the waves-per-EU floors below keep the occupancy these kernels had before
// the library's max-ilp scheduling, Makefile: it would trade it for ILP)
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(6))) void k_prep_cols(int cnt, const unsigned *__restrict__ perm, int presorted, int rec,
                                                     SoA6 own, SoA6 intr, int distinct, int shared,
                                                     double rpz, double hpz, double tla,
                                                     ColRec *__restrict__ C, PFRec *__restrict__ PC,
                                                     PFVel *__restrict__ PV, float4 *__restrict__ PP, int mid,
                                                     ReuseParams rz, FusedBoxes fb, ZeroArgs zs, int tile_base,
                                                     const int *__restrict__ tile_list, HaloUnpack hu,
                                                     Counters *__restrict__ hcnt, TprCheck tck, NfArgs nf, int nown) {
  __shared__ TileBox fgb[kTile / 64];
  // K0z (fused): nothing here reads that state
  if (zs.cnt) zero_state(zs, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  // workgroups [0, nown): tiles tile_base + b; the rest: slots b - nown of
  // tile_list (the halo K0b's received tiles; one launch with the own tiles
  // when the host kept the plan, HK)
  const int b = (int)blockIdx.x;
  const bool mine = b < nown;
  const int slot = b - nown;
  int tile = mine ? tile_base + b : (hu.count && slot >= (int)*hu.count ? -1 : tile_list[slot]);
  // halo exchange: this slot's received tile rows first (each thread writes
  // the row it prepares below), checked against this rank's plan
  if (!mine && hu.rbuf) tile = halo_unpack_tile(hu, slot, tile, hcnt);
  if (tile < 0) return;  // (the whole workgroup: no barrier is skipped by part of it)
  const int k = tile * kTile + (int)threadIdx.x;
  bool over = false;       // reuse: this aircraft overran a budget
  float use_h = 0.f, use_v = 0.f;
  PFRec pk{}, pb{};        // this lane's record (the fused boxes take it from registers), its build's
  const bool check = tck.snap && mine;  // (the own tiles' records: the halo tiles' are their owners' to check)
  if (check && k < cnt) pb = tck.snap[k];
  if (k < cnt) {
    const int o = presorted ? k : (int)perm[k];
    const double tlap = tla > 0.0 ? tla : 0.0;
    const ColRec c = col_record(own, intr, o);
    if (rec) C[k] = c;
    if (nf.word && !col_tcpa_finite(c)) *nf.word = nf.epoch;
    const double lo = c.lon, sinl = c.sinlat, cosl = c.coslat, gs = own.gs[o], olat = c.olat;
    const double lor = lo * kD2R;
    // (own.lat[j] == 0) leaves the different-hemisphere radius unbounded below
    // when own != intruder (geo.py:128): never prune such a column horizontally
    // nor refine it.
    const bool quirk = distinct && olat == 0.0;
    double coslo, sinlo;
    sincos(lor, &sinlo, &coslo);
    const double px = cosl * coslo, py = cosl * sinlo, pz = sinl;
    float sv = 0.f, sadd = 0.f;
    if (rz.build) {  // reuse (shared records only): budget check against the last build
      double svn = rz.sv_default;
      if (rz.valid) {
        const Snap b = rz.build[k];
        const double dx = px - b.x, dy = py - b.y, dz = pz - b.z;
        const double dch = sqrt(dx * dx + dy * dy + dz * dz);
        const double rho = fmin(sqrt(px * px + py * py), sqrt(b.x * b.x + b.y * b.y));
        // |dE| + |dN| <= (pi/2) |dr| (1 + 2 / rho): the refine basis turns with the row
        const double L = 1.0 + 1.5708 * kRefineChord * (1.0 + 2.0 / rho);
        const double du = c.u - b.u, dv = c.v - b.v;
        const double dh = (dch * 6378137.0 * L + sqrt(du * du + dv * dv) * tlap) * 1.001 + 1e-3;
        const double dvv = (fabs(c.alt - b.alt) + fabs(c.vs - b.vs) * tlap) * 1.001 + 1e-3;
        over = !(dh <= rz.sh) || !(dvv <= (double)b.sv);  // (NaN -> rebuild)
        use_h = (float)fmin(dh / rz.sh, 1e30);
        use_v = (float)fmin(dvv / (double)b.sv, 1e30);
        if (!(use_h >= 0.f)) use_h = 1e30f;
        if (!(use_v >= 0.f)) use_v = 1e30f;
        // next budget: this aircraft's vertical drift rate over ktarget detects
        const double age = (double)rz.ctl[1] + 1.0;
        svn = fmin(rz.sv_max, fmax(rz.sv_min, 2.0 * (dvv / age) * rz.ktarget));
      }
      sv = (float)svn;
      Snap sn;
      sn.x = px;
      sn.y = py;
      sn.z = pz;
      sn.u = c.u;
      sn.v = c.v;
      sn.alt = c.alt;
      sn.vs = c.vs;
      sn.sv = sv;
      sn.pad = 0.f;
      rz.cur[k] = sn;
      sadd = rz.sh_chord;
    }
    // (midpoint mode is never combined with reuse: the host passes mid = 0 then)
    PFRec p = mid ? make_pf_mid(px, py, pz, sinl, cosl, coslo, sinlo, c.u, c.v, gs, c.alt, c.vs, rpz, hpz, tlap)
                  : make_pf(px, py, pz, reach_h(rpz, gs, tlap) + sadd, c.alt,
                            reach_v(hpz, c.vs, c.alt, tlap) + (double)sv, sv);
    if (quirk) p.s = INFINITY;
    PP[k] = make_float4((float)px, (float)py, (float)pz, 0.f);
    PFVel v;
    v.u = (float)c.u;
    v.v = (float)c.v;
    v.vs = (float)c.vs;
    v.flags = (quirk || !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) ? 1u : 0u;
    // shared records also serve as rows: add the rows' pole flag (k_prep_rows)
    if (shared && !(cosl > 1e-2)) v.flags = 1u;
    PC[k] = p;
    PV[k] = v;
    pk = p;
  }
  if (rz.build) {  // one store per wave, no atomics
    const unsigned long long ob = __ballot(over);
    for (int o = 32; o > 0; o >>= 1) {
      use_h = fmaxf(use_h, __shfl_xor(use_h, o));
      use_v = fmaxf(use_v, __shfl_xor(use_v, o));
    }
    if ((threadIdx.x & 63) == 0) {
      if (ob) rz.ctl[0] = 1u;
      const int wv = k >> 6;
      rz.use[2 * wv] = use_h;
      rz.use[2 * wv + 1] = use_v;
    }
  }
  if (check) {  // plan reuse: one flag store per wave whose records left their budgets
    const bool out = k < cnt && !pf_within(pk, pb, tck.dx, tck.ds, tck.dv);
    if (__ballot(out) && (threadIdx.x & 63) == 0) *tck.flag = 1u;
    if (tck.pred) {  // HK: ... or f x the budgets (a rebuild two detects on)
      const bool near = k < cnt && !pf_within(pk, pb, tck.f * tck.dx, tck.f * tck.ds, tck.f * tck.dv);
      if (__ballot(near) && (threadIdx.x & 63) == 0) *tck.pred = 1ull;
    }
  }
  // K0c (fused): this thread wrote PC[k] above, every thread reaches the barrier
  if (fb.gbox) tile_boxes_v(cnt, tile, pk, fgb, fb.sbox, fb.gbox, fb.tbox);
  if (fb.blk && threadIdx.x == 0) fb.blk[tile - fb.blk_base] = fb.tbox[tile];  // (written by this thread)
}

// ------------------------------------------------------------------ K0c tile boxes
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(8))) void k_boxes(int cnt, const PFRec *__restrict__ P,
                                                 TileBox *__restrict__ sbox, TileBox *__restrict__ gbox,
                                                 TileBox *__restrict__ tbox, const unsigned *__restrict__ build,
                                                 Counters *__restrict__ reset) {
  __shared__ TileBox gb[kGroupsPerTile];
  if (build && !build[0]) return;  // reused candidate list: no sweep this detect
  if (reset && blockIdx.x == 0) {  // reuse build: start from an empty candidate list
    constexpr int kWords = (int)(sizeof(Counters) / 8);
    for (int k = threadIdx.x; k < kWords; k += blockDim.x)
      if (list_word(k)) reinterpret_cast<unsigned long long *>(reset)[k] = 0;
  }
  tile_boxes(cnt, blockIdx.x, P, gb, sbox, gbox, tbox);
}

// ------------------------------------------------------------------ K0d tile pairs

// K0d: the kept tile pairs, listed in two classes: pairs whose boxes overlap
// ("near": a row tile against itself and its neighbours, the costly items)
// from the front of the list, the others from its back (cap - 1 - k), so the
// sweep dequeues the near pairs first -- longest items first keeps the tail of
// the dynamic schedule short (measured -5 us at box100k).
// Two-level: a workgroup takes one SUPER row (kSuper row tiles), tests its
// union box against every super column's (kSuper column tiles) and only
// expands the kept super pairs into tile pairs: at 1M aircraft ~1 % of the
// (N/512)^2 tile pairs survive, so testing them all (3.8 M box pairs) cost
// 42 us.  A union box is a superset of its tiles' boxes and
// boxes_may_interact is monotone in the extents, so no kept tile pair is
// lost.  One returning atomic per class and expansion round of the
// workgroup (a returning atomic on one word saturates at ~88 per us,
// MI355X_MICROARCH 'dequeue').
constexpr int kTPThreads = 1024;
constexpr int kSuper = 8;  // tiles per super tile (each side)
// present (halo mode, nullable): column tiles whose data this rank holds --
// its own [p0, p1) and the halo tiles it received.  A kept pair with any
// other column tile means the halo plan disagreed with this test (it cannot:
// the plan runs the same boxes_may_interact on the same boxes): it is flagged
// (cnt->halo_miss, the step fails loudly), never silently dropped or swept.
// K0d's test of one (row tile rt, column tile ct) pair: its class (near: the
// boxes overlap, far: they only may interact) and the mask of the row tile's
// 64-row slices whose boxes may reach the column tile (sg: the slice boxes)
__device__ __forceinline__ unsigned tp_classify(const TileBox &a, const TileBox *sg, const TileBox &b, int rt, int ct,
                                                int nrows, int noprune, const uint8_t *__restrict__ present, int p0,
                                                int p1, Counters *__restrict__ cnt, bool &kn, bool &kf, int sym) {
  unsigned sm = 0;
  // symmetric sweep (DetectPlan::sym; row tile t is column tile t): the pair
  // (ct, rt) covers this one, its items refined in both orientations
  if (sym && ct < rt) return 0u;
  if ((noprune || boxes_may_interact(a, b)) && present && !(ct >= p0 && ct < p1) && !present[ct]) {
    cnt->halo_miss = 1;
  } else if (noprune || boxes_may_interact(a, b)) {
    const bool near = gap(a.lo[0], a.hi[0], b.lo[0], b.hi[0]) == 0.f &&
                      gap(a.lo[1], a.hi[1], b.lo[1], b.hi[1]) == 0.f &&
                      gap(a.lo[2], a.hi[2], b.lo[2], b.hi[2]) == 0.f;
    kn = near;
    kf = !near;
    for (int q = 0; q < kSlicesPerTile; ++q)
      if (rt * kTile + q * kGroup < nrows && (noprune || boxes_may_interact(sg[q], b))) sm |= 1u << q;
  }
  return sm;
}

// K0d's list append of one round (every lane of the NT-lane workgroup calls
// it): the items (slices) of each class and the tile pairs themselves, one
// returning atomic per class (near ones from the front of the list, the
// others from its back)
template <int NT>
__device__ __forceinline__ void tp_emit(bool kn, bool kf, unsigned sm, int rt, int ct, uint2 *__restrict__ out,
                                        unsigned long long cap, Counters *__restrict__ cnt,
                                        unsigned long long *__restrict__ icnt, unsigned (*wpre)[NT / 64],
                                        unsigned long long *bbase, int sym) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned ni = (unsigned)__popc(sm);
  const unsigned xn = wave_incl_scan(kn ? ni : 0u), xf = wave_incl_scan(kf ? ni : 0u);
  const unsigned tw = (unsigned)__popcll(__ballot(kn)) | (unsigned)__popcll(__ballot(kf)) << 16;
  if (lane == 63) {
    wpre[0][w] = xn;
    wpre[1][w] = xf;
    wpre[3][w] = tw;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned run = 0, tiles = 0;
    for (int q = 0; q < NT / 64; ++q) {
      const unsigned v = wpre[threadIdx.x][q];
      wpre[threadIdx.x][q] = run;
      run += v;
      tiles += (wpre[3][q] >> (16 * threadIdx.x)) & 0xffffu;
    }
    bbase[threadIdx.x] = run ? atomicAdd(&icnt[1 + threadIdx.x], (unsigned long long)run) : 0ull;
    if (tiles) {
      atomicAdd(&cnt->tiles, (unsigned long long)tiles);
      if (threadIdx.x == 0) atomicAdd(&cnt->tiles_near, (unsigned long long)tiles);
    }
  }
  __syncthreads();
  if (ni) {  // item = (row tile | slice << 22 | flags, column tile); near ones from the front
    // mirrored (kItemMirror): an off-diagonal pair of a symmetric list -- the
    // sweep refines its stage-1 survivors as (row, column) and as (column, row)
    // triangular (kItemTri, level 2): a diagonal pair -- the sweep skips the
    // column sub-groups below the slice's own and mirrors the ones above
    const unsigned mir = sym && rt != ct ? kItemMirror : (sym >= 2 && rt == ct ? kItemTri : 0u);
    unsigned long long k = (kn ? bbase[0] + wpre[0][w] + xn : bbase[1] + wpre[1][w] + xf) - ni;
    for (unsigned m = sm; m; m &= m - 1u, ++k) {
      const uint2 v = make_uint2((unsigned)rt | (unsigned)__builtin_ctz(m) << 22 | mir, (unsigned)ct);
      out[kn ? k : cap - 1 - k] = v;
    }
  }
}

__global__ __launch_bounds__(kTPThreads) void k_tilepairs(int nrt, int nct, int nrows, const TileBox *__restrict__ rb,
                                                          const TileBox *__restrict__ rg,
                                                          const TileBox *__restrict__ cb, int noprune,
                                                          uint2 *__restrict__ out, unsigned long long cap,
                                                          Counters *__restrict__ cnt,
                                                          unsigned long long *__restrict__ icnt,
                                                          const unsigned *__restrict__ build,
                                                          const uint8_t *__restrict__ present, int p0, int p1,
                                                          int sym) {
  if (build && !build[0]) return;
  __shared__ TileBox srt[kSuper];                    // this super row's tile boxes
  __shared__ TileBox sgb[kSuper * kSlicesPerTile];   // ... and its 64-row slices' boxes
  __shared__ unsigned keep[kTPThreads];      // kept super columns of the chunk
  __shared__ unsigned wpre[4][kTPThreads / 64];
  __shared__ unsigned long long bbase[2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int rt0 = blockIdx.x * kSuper, nr = min(kSuper, nrt - rt0);
  if (threadIdx.x < nr) srt[threadIdx.x] = rb[rt0 + threadIdx.x];
  if (threadIdx.x < nr * kSlicesPerTile && rt0 * kTile + (int)threadIdx.x * kGroup < nrows)
    sgb[threadIdx.x] = rg[rt0 * kSlicesPerTile + threadIdx.x];
  __syncthreads();
  TileBox sr = srt[0];
  for (int i = 1; i < nr; ++i) sr = box_union(sr, srt[i]);
  const int nsc = (nct + kSuper - 1) / kSuper;
  for (int c0 = 0; c0 < nsc; c0 += kTPThreads) {
    // super columns c0 + threadIdx.x: union box, tested against the super row
    const int sc = c0 + threadIdx.x;
    bool kp = false;
    if (sc < nsc) {
      const int ct0 = sc * kSuper, nc = min(kSuper, nct - ct0);
      TileBox u = cb[ct0];
      for (int j = 1; j < nc; ++j) u = box_union(u, cb[ct0 + j]);
      kp = (noprune || boxes_may_interact(sr, u)) && !(sym && ct0 + nc <= rt0);  // (sym: no tile pair with rt <= ct in it)
    }
    const unsigned x = wave_incl_scan(kp ? 1u : 0u);
    if (lane == 63) wpre[2][w] = x;
    __syncthreads();
    unsigned before = 0, K = 0;
    for (int q = 0; q < kTPThreads / 64; ++q) {
      before += q < w ? wpre[2][q] : 0u;
      K += wpre[2][q];
    }
    if (kp) keep[before + x - 1] = (unsigned)sc;
    __syncthreads();
    // expansion: K super columns x (nr row tiles x kSuper column tiles)
    const unsigned ne = K * kSuper * kSuper;
    for (unsigned e0 = 0; e0 < ne; e0 += kTPThreads) {
      const unsigned e = e0 + threadIdx.x;
      bool kn = false, kf = false;
      int rt = 0, ct = 0;
      unsigned sm = 0;  // slices of row tile rt whose boxes may interact with column tile ct
      if (e < ne) {
        const unsigned sc2 = keep[e / (kSuper * kSuper)], r = e % (kSuper * kSuper);
        const int i = (int)(r / kSuper);
        rt = rt0 + i;
        ct = (int)sc2 * kSuper + (int)(r % kSuper);
        if (i < nr && ct < nct) sm = tp_classify(srt[i], &sgb[i * kSlicesPerTile], cb[ct], rt, ct, nrows, noprune,
                                                 present, p0, p1, cnt, kn, kf, sym);
      }
      tp_emit<kTPThreads>(kn, kf, sm, rt, ct, out, cap, cnt, icnt, wpre, bbase, sym);
      __syncthreads();  // wpre / bbase are rewritten by the next round
    }
  }
}

// K0d without the super level, for few column tiles (the 100k box: 196):
// one workgroup per row tile, one lane per column tile -- the super pass's
// union loads, its scan and its barrier were a third of K0d's chain there
constexpr int kTPDirectThreads = 256;
// Halo mode (hl != NULL): the columns are this rank's own tiles [p0, p1) and
// the received halo tiles hl[0, nhl) (-1: an unused slot; *nhl_dev bounds the
// list when set), not all nct tiles -- one rank of 8 at 1M holds ~300 of the
// 1954 tiles.  Every other tile is still tested against the row tile, without
// an append: a kept pair with a tile the halo plan did not deliver sets
// Counters::halo_miss (the step fails loudly), as the full sweep did.
__global__ __launch_bounds__(kTPDirectThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_tilepairs_direct(
    int nrt, int nct, int nrows, const TileBox *__restrict__ rb, const TileBox *__restrict__ rg,
    const TileBox *__restrict__ cb, int noprune, uint2 *__restrict__ out, unsigned long long cap,
    Counters *__restrict__ cnt, unsigned long long *__restrict__ icnt, const unsigned *__restrict__ build,
    const uint8_t *__restrict__ present, int p0, int p1, const TileBox *__restrict__ gbc,
    const int *__restrict__ hl, int nhl, const unsigned *__restrict__ nhl_dev, TprArgs tp, int sym) {
  if (tp.myflag && blockIdx.x == 0 && threadIdx.x == 0) *tp.myflag = 0u;  // (k_halo_plan's blocks all read it)
  if (build && !build[0]) return;
  // tile-pair list reuse: no build this detect -> the kept
  // list's item counts into the dequeue words, nothing else
  const bool grow = tp.ctl != nullptr;
  if (grow && !(tp.force || tp.ctl[0] != 0ull)) {
    if (blockIdx.x == 0 && threadIdx.x < 2) icnt[1 + threadIdx.x] = tp.ctl[1 + threadIdx.x];
    return;
  }
  __shared__ TileBox sgb[kSlicesPerTile];
  __shared__ unsigned wpre[4][kTPDirectThreads / 64];
  __shared__ unsigned long long bbase[2];
  const int rt = blockIdx.x;
  // gbc (the resident step's prepped detect, no K0z launch): the tile boxes
  // from the group boxes, as tile_from_groups would have written them (the
  // rows are the columns then, so the row groups are the column groups)
  auto tile_of = [&](int t) {
    const int ng = (nrows + kGroup - 1) / kGroup;  // (all rows detected: nrows = n)
    TileBox g[kGroupsPerTile];
#pragma unroll
    for (int q = 0; q < kGroupsPerTile; ++q) g[q] = gbc[min(t * kGroupsPerTile + q, ng - 1)];  // loads together
    TileBox u = t * kGroupsPerTile < ng ? g[0] : empty_box();
#pragma unroll
    for (int q = 1; q < kGroupsPerTile; ++q) u = box_union(u, t * kGroupsPerTile + q < ng ? g[q] : empty_box());
    return u;
  };
  // column k of the sweep: tile k (all tiles), or own tile p0 + k / halo tile hl[k - (p1 - p0)]
  const int nown = p1 - p0;
  const int ncols = hl ? nown + (nhl_dev ? min(nhl, (int)*nhl_dev) : nhl) : nct;
  auto col_of = [&](int k) { return k >= ncols ? -1 : (!hl ? k : (k < nown ? p0 + k : hl[k - nown])); };
  // every box load issued before the first barrier (one round trip)
  int ct = col_of((int)threadIdx.x);
  TileBox bc = gbc ? tile_of(max(ct, 0)) : cb[max(ct, 0)];
  if (threadIdx.x < kSlicesPerTile && rt * kTile + (int)threadIdx.x * kGroup < nrows)
    sgb[threadIdx.x] = rg[rt * kSlicesPerTile + threadIdx.x];
  TileBox a = gbc ? empty_box() : rb[rt];
  if (grow) {  // a build: the snapshot of this row tile's records (rows = columns here)
    for (int k = rt * kTile + (int)threadIdx.x; k < min(nrows, (rt + 1) * kTile); k += kTPDirectThreads)
      tp.snap[k] = tp.pc[k];
  }
  __syncthreads();
  if (gbc) {  // the row tile's groups are its slices (rows = columns): tile_from_groups' union from LDS
    a = sgb[0];
    for (int q = 1; q < kSlicesPerTile; ++q) a = box_union(a, rt * kTile + q * kGroup < nrows ? sgb[q] : empty_box());
  }
  if (grow) {  // the list outlives this detect: every box grown by the drift budgets
    a = box_grow(a, tp.dx, tp.ds, tp.dv);
    bc = box_grow(bc, tp.dx, tp.ds, tp.dv);
    __syncthreads();  // (every lane has read sgb above)
    if (threadIdx.x < kSlicesPerTile) sgb[threadIdx.x] = box_grow(sgb[threadIdx.x], tp.dx, tp.ds, tp.dv);
    __syncthreads();
  }
  for (int c0 = 0; c0 < ncols; c0 += kTPDirectThreads) {
    if (c0 > 0) {
      ct = col_of(c0 + (int)threadIdx.x);
      if (ct >= 0) bc = gbc ? tile_of(ct) : cb[ct];
      if (grow) bc = box_grow(bc, tp.dx, tp.ds, tp.dv);
    }
    bool kn = false, kf = false;
    unsigned sm = 0;
    if (ct >= 0) sm = tp_classify(a, sgb, bc, rt, ct, nrows, noprune, present, p0, p1, cnt, kn, kf, sym);
    tp_emit<kTPDirectThreads>(kn, kf, sm, rt, ct, out, cap, cnt, icnt, wpre, bbase, sym);
    __syncthreads();  // wpre / bbase are rewritten by the next round
  }
  if (hl) {  // the tiles this rank does not hold: none may be reachable (no appends, no barriers;
             // 4 tiles' loads per lane issued together, not one dependent round trip per tile)
    bool miss = false;
    for (int t0 = (int)threadIdx.x; t0 < nct; t0 += 4 * kTPDirectThreads) {
      TileBox b[4];
      uint8_t pr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = min(t0 + u * kTPDirectThreads, nct - 1);
        b[u] = cb[t];
        pr[u] = present[t];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * kTPDirectThreads;
        miss |= t < nct && !(t >= p0 && t < p1) && !pr[u] && (noprune || boxes_may_interact(a, b[u]));
      }
    }
    if (miss) cnt->halo_miss = 1;
  }
}

// Zero the per-detect state: counters (but `tiles` unless full; with keep,
// nothing of the candidate list: its counts, tiles and groups), the dequeue
// shards and the per-row outputs / counts.  Grid-stride, one word per lane
// (zero_state, shared with the fused K0z+K0b path of k_prep_cols).
// tbox (nullable): the tile boxes of cnt records from their group boxes (the
// records and group boxes were written by the resident step's K4').
__global__ __launch_bounds__(256) void k_zero(int nrows, int full, int keep, unsigned *__restrict__ rctl,
                                              int rforce, Counters *__restrict__ cnt,
                                              unsigned long long *__restrict__ work,
                                              unsigned char *__restrict__ inconf,
                                              unsigned long long *__restrict__ tcpamax,
                                              unsigned *__restrict__ rowcnt, int tcnt,
                                              const TileBox *__restrict__ gbox, TileBox *__restrict__ tbox) {
  if (rctl && blockIdx.x == 0 && threadIdx.x == 0) {  // reuse: build this detect? (force: age 0)
    rctl[0] = rforce ? 1u : 0u;
    if (rforce) rctl[1] = 0u;
  }
  if (tbox)
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < (tcnt + kTile - 1) / kTile; t += gridDim.x * blockDim.x)
      tile_from_groups(tcnt, t, gbox, tbox);
  zero_state(ZeroArgs{nrows, full, keep, cnt, work, inconf, tcpamax, rowcnt, {}, {}},
             blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// ------------------------------------------------------------------ host side
// spatial sort of cnt positions starting at original index base -> perm
int spatial_order(Ctx *c, int cnt, int base, const double *lat, const double *lon, const double *trk,
                         const double *gs, double f, DevBuf &key, DevBuf &idx, DevBuf &key2, DevBuf &perm) {
  if (!ensure(c, key, (size_t)cnt * 4, "keys") || !ensure(c, idx, (size_t)cnt * 4, "key idx") ||
      !ensure(c, key2, (size_t)cnt * 4, "sorted keys") || !ensure(c, perm, (size_t)cnt * 4, "perm"))
    return -1;
  hipLaunchKernelGGL(k_keys, dim3(blocks_for(cnt, 256)), dim3(256), 0, c->stream, cnt, base, lat, lon, trk, gs,
                     f, (unsigned *)key.p, (unsigned *)idx.p);
  BSA_HIP(c, hipGetLastError());
  size_t tmp = 0;
  BSA_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (unsigned *)key.p, (unsigned *)key2.p,
                                                (unsigned *)idx.p, (unsigned *)perm.p, cnt, 0, 30,
                                                c->stream));
  if (!ensure(c, c->sort_tmp, std::max<size_t>(tmp, 16), "sort scratch")) return -1;
  tmp = c->sort_tmp.bytes;
  BSA_HIP(c, hipcub::DeviceRadixSort::SortPairs(c->sort_tmp.p, tmp, (unsigned *)key.p,
                                                (unsigned *)key2.p, (unsigned *)idx.p,
                                                (unsigned *)perm.p, cnt, 0, 30, c->stream));
  return 0;
}

// Home order of the resident sim (bsa_sim_init): the spatial order of the
// traffic in own[] (aircraft-index order) at the look-ahead midpoints the
// detect's stage 1 uses -> h2id (home position -> aircraft index).  Every rank
// computes the same permutation from the same state (deterministic sort).
int home_order(Ctx *c, double tla, std::vector<unsigned> &h2id) {
  const int64_t n = c->n;
  const double kf = 0.5 * (tla > 0.0 ? tla : 0.0) / 6371000.0;
  DevBuf key, idx, key2, perm;
  struct Rel {
    DevBuf *b[4];
    ~Rel() {
      for (auto *x : b) release(*x);
    }
  } rel{{&key, &idx, &key2, &perm}};
  if (spatial_order(c, (int)n, 0, (const double *)c->own[0].p, (const double *)c->own[1].p,
                    (const double *)c->own[2].p, (const double *)c->own[3].p, kf, key, idx, key2, perm))
    return -1;
  h2id.assign((size_t)n, 0u);
  BSA_HIP(c, hipMemcpyAsync(h2id.data(), perm.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the launchers (bsa_detect.h; PrepColsLaunch: bsa_cd_args.h)
int launch_prep_cols(Ctx *c, hipStream_t stream, unsigned grid, const PrepColsLaunch &a) {
  hipLaunchKernelGGL(k_prep_cols, dim3(grid), dim3(kTile), 0, stream, a.n, a.perm, a.presorted, a.rec, a.own, a.intr,
                     a.distinct, a.shared, a.rpz, a.hpz, a.tla, (ColRec *)c->colrec.p, (PFRec *)c->pfcol.p,
                     (PFVel *)c->pfvcol.p, (float4 *)c->pfpcol.p, a.mid, a.rz, a.fb, a.zs, a.tile_base, a.tile_list,
                     a.hu, a.hcnt, a.tck, a.nf, a.nown < 0 ? (int)grid : a.nown);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

bool ensure_col_prep(Ctx *c, int64_t n, bool rec) {
  return (!rec || ensure(c, c->colrec, n * sizeof(ColRec), "column records")) &&
         ensure(c, c->pfcol, n * sizeof(PFRec), "prefilter columns") &&
         ensure(c, c->pfvcol, n * sizeof(PFVel), "prefilter column velocities") &&
         ensure(c, c->pfpcol, n * sizeof(float4), "prefilter column positions") &&
         ensure(c, c->tbox_c, ((n + kTile - 1) / kTile) * sizeof(TileBox), "column tile boxes") &&
         ensure(c, c->gbox_c, ((n + kGroup - 1) / kGroup) * sizeof(TileBox), "column group boxes") &&
         ensure(c, c->sbox_c, ((n + kSub - 1) / kSub) * sizeof(TileBox), "column sub-group boxes");
}

int prep_all_tiles(Ctx *c, double rpz, double hpz, double tla, unsigned long long nf_epoch) {
  const int64_t n = c->n;
  if (n <= 0) return 0;
  const int nct = (int)((n + kTile - 1) / kTile);
  if (!ensure_col_prep(c, n, true)) return -1;
  // home order, no stored fp64 records, every tile with its fused boxes
  PrepColsLaunch a;
  a.n = (int)n;
  a.perm = (const unsigned *)c->h2id.p;
  a.own = a.intr = soa(c->own);
  a.rpz = rpz;
  a.hpz = hpz;
  a.tla = tla;
  a.mid = stage1_mid(0, false, 0);
  a.nf = NfArgs{nf_epoch ? (unsigned long long *)c->nonfin.p : nullptr, nf_epoch, nullptr};
  a.fb = FusedBoxes{(TileBox *)c->sbox_c.p, (TileBox *)c->gbox_c.p, (TileBox *)c->tbox_c.p, nullptr, 0};
  return launch_prep_cols(c, c->stream, (unsigned)nct, a);
}

// K0b of rows that are not columns (own != intruder, or a row range)
int launch_prep_rows(const DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  hipLaunchKernelGGL(k_prep_rows, dim3(blocks_for(p.nrows, 256)), dim3(256), 0, c->stream, (int)p.nrows, R.perm_r,
                     R.own, R.intr, p.rpz, p.hpz, p.tla, (RowRec *)c->rowrec.p, (PFRec *)c->pfrow.p,
                     (PFVel *)c->pfvrow.p, (float4 *)c->pfprow.p, p.mid, (uint8_t *)c->rownf.p, (int)p.rb);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// K0c as its own launch: the rows' group / tile boxes, or (cols) the columns'
// with their sub-group boxes and the reused candidate list's reset
int launch_boxes(const DetectRun &R, bool cols) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  if (cols)
    hipLaunchKernelGGL(k_boxes, dim3(p.nct), dim3(kTile), 0, c->stream, (int)p.n, (const PFRec *)c->pfcol.p,
                       (TileBox *)c->sbox_c.p, (TileBox *)c->gbox_c.p, (TileBox *)c->tbox_c.p, R.build, R.dcnt);
  else
    hipLaunchKernelGGL(k_boxes, dim3(p.nrt), dim3(kTile), 0, c->stream, (int)p.nrows, R.pfrow, (TileBox *)nullptr,
                       (TileBox *)c->gbox_r.p, (TileBox *)c->tbox_r.p, R.build, (Counters *)nullptr);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// K0d, direct form (few column tiles, or the halo tile list) and two-level form
int launch_tilepairs_direct(const DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  hipLaunchKernelGGL(k_tilepairs_direct, dim3((unsigned)p.nrt), dim3(kTPDirectThreads), 0, c->stream, p.nrt, p.nct,
                     (int)p.nrows, R.tbox_r, R.gbox_r, (const TileBox *)c->tbox_c.p, p.noprune,
                     (uint2 *)c->tilepairs.p, p.icap, R.dcnt, (unsigned long long *)c->workq.p, R.build,
                     p.halo ? halo_present(c) : nullptr, p.a0, p.a1,
                     p.nozero ? (const TileBox *)c->gbox_c.p : (const TileBox *)nullptr,
                     p.tp_list ? (const int *)c->h_hl.p : (const int *)nullptr, (int)c->halo_hl,
                     p.tp_list ? halo_list_count(c) : (const unsigned *)nullptr, R.tp, p.sym);
  BSA_HIP(c, hipGetLastError());
  return 0;
}
int launch_tilepairs(const DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  hipLaunchKernelGGL(k_tilepairs, dim3((unsigned)((p.nrt + kSuper - 1) / kSuper)), dim3(kTPThreads), 0, c->stream,
                     p.nrt, p.nct, (int)p.nrows, R.tbox_r, R.gbox_r, (const TileBox *)c->tbox_c.p, p.noprune,
                     (uint2 *)c->tilepairs.p, p.icap, R.dcnt, (unsigned long long *)c->workq.p, R.build,
                     p.halo ? halo_present(c) : nullptr, p.a0, p.a1, p.sym);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// K0z: zero the per-detect state (launched once the reuse decision is known)
int DetectRun::zero(bool keep, unsigned *rctl, int rforce, bool tiles) const {
  const int64_t m = std::max<int64_t>(2 * (p.nrows + 1), 256);
  hipLaunchKernelGGL(k_zero, dim3((unsigned)std::min<int64_t>(blocks_for(m, 256 * 4), 256)), dim3(256), 0,
                     c->stream, (int)p.nrows, 1, keep ? 1 : 0, rctl, rforce, dcnt,
                     (unsigned long long *)c->workq.p, (unsigned char *)c->inconf.p,
                     (unsigned long long *)c->tcpamax.p, (unsigned *)c->rowcnt.p, (int)p.n,
                     (const TileBox *)c->gbox_c.p, tiles ? (TileBox *)c->tbox_c.p : (TileBox *)nullptr);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

}  // namespace bsa
