// Route edits on the device: ADDWPT / DELWPT / DIRECT as a
// batch of records on the route table.  The host groups the batch by aircraft,
// checks every record against the route the earlier ones leave and places each
// edited route behind the table's tail (bsa_route_math.h); k_route_edit, one
// wave per edited route, copies the route there, applies its records in order
// and after each recomputes the flight plan (Route.calcfp: legs by lanes, the
// backward VNAV pass in one lane) and runs Route.direct (bsa_fms_math.h, the
// one bsa_fms_recover uses).  Dead rows are compacted in aircraft order with
// the single-pass scan once they outnumber the live ones.
#include "bsa_fms_math.h"
#include "bsa_route_math.h"

#pragma clang fp contract(off)

namespace bsa {

struct EditGroup {
  int h;          // the aircraft's position in the FMS arrays
  int rec0, cnt;  // its records, grouped order
  int dst;        // first row of its new place
  int n0;         // waypoints before the batch
};

struct RowRegs {
  double2 v[4];
  uint8_t t;
};
__device__ __forceinline__ RowRegs row_load(const double *rows, const uint8_t *types, size_t r) {
  const double2 *p = (const double2 *)(rows + r * fms::kRouteCols);
  return {{p[0], p[1], p[2], p[3]}, types[r]};
}
__device__ __forceinline__ void row_store(double *rows, uint8_t *types, size_t r, const RowRegs &x) {
  double2 *p = (double2 *)(rows + r * fms::kRouteCols);
  p[0] = x.v[0], p[1] = x.v[1], p[2] = x.v[2], p[3] = x.v[3];
  types[r] = x.t;
}

// Route.calcfp of the n rows at `route` (route.py:983-1041) and the nextqdr
// column: chunks of 64 waypoints from the last one down.  Lane i takes leg
// i -> i + 1 (geo.qdrdist: wpdirfrom[i] = nextqdr[i], wpdistto[i + 1]); lane 0
// then walks the chunk's VNAV pass over LDS in the reference's order of
// additions, carrying (toalt, xtoalt) to the next chunk.
__device__ __forceinline__ void flight_plan(double *route, const uint8_t *types, int n) {
  __shared__ double s_alt[64], s_dist[64], s_toalt[64], s_xtoalt[64];
  __shared__ int s_type[64];
  const int lane = threadIdx.x;
  route::Vnav v;
  for (int i1 = n; i1 > 0; i1 -= 64) {
    const int i0 = i1 > 64 ? i1 - 64 : 0;
    const int i = i0 + lane;
    const bool act = i < i1;
    if (act) {
      double *row = route + (size_t)i * fms::kRouteCols;
      double qdr = -999., dist = 0.;
      if (i + 1 < n) fms::qdrdist(row[0], row[1], row[fms::kRouteCols], row[fms::kRouteCols + 1], qdr, dist);
      row[7] = qdr;
      s_alt[lane] = row[2], s_dist[lane] = dist, s_type[lane] = types[i];
    }
    __syncthreads();
    if (lane == 0) route::vnav_pass(v, i0, i1, n, s_alt, s_type, s_dist, s_toalt, s_xtoalt);
    __syncthreads();
    if (act) {
      double *row = route + (size_t)i * fms::kRouteCols;
      row[4] = s_xtoalt[lane], row[5] = s_toalt[lane];
    }
    __syncthreads();
  }
}

// One wave per edited route.  Every loop bound is wave-uniform; the rows a
// chunk moves are read by all lanes before any lane writes (the barrier), and
// chunks go top-down for an insert, bottom-up for a delete, so no row is
// overwritten before it is read.  The group's place [dst, dst + most rows the
// route holds on the way) lies behind the table's tail, sized by the host.
__global__ __launch_bounds__(64) void k_route_edit(int ng, const EditGroup *__restrict__ grp,
                                                   const bsa_route_edit_rec *__restrict__ rec, double *rows,
                                                   uint8_t *types, int *rt_off, int *rt_n, FmsArrays a) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= ng) return;
  const EditGroup G = grp[g];
  const int k = G.h;
  int n = G.n0;
  {
    const size_t src = (size_t)rt_off[k];
    for (int i = lane; i < n; i += 64) row_store(rows, types, (size_t)G.dst + i, row_load(rows, types, src + i));
  }
  double *route = rows + (size_t)G.dst * fms::kRouteCols;
  uint8_t *rtype = types + G.dst;
  fms::Lane L{};
  if (lane == 0) {   // what Route.direct reads or writes (recover_lane's set) and actwp.next_qdr
    L.lat = a.tr[0][k], L.lon = a.tr[1][k], L.alt = a.tr[2][k], L.tas = a.tr[3][k];
    L.gs = a.tr[4][k], L.trk = a.tr[5][k], L.bank = a.tr[7][k];
    L.wlat = a.st[0][k], L.wlon = a.st[1][k], L.nextaltco = a.st[2][k], L.xtoalt = a.st[3][k];
    L.spd = a.st[4][k], L.vs = a.st[5][k], L.turndist = a.st[6][k], L.flyby = a.st[7][k];
    L.next_qdr = a.st[8][k], L.dist2vs = a.st[9][k], L.selspd = a.st[12][k];
    L.swlnav = a.fl[0][k] != 0, L.swvnav = a.fl[1][k] != 0;
    L.ap_alt = a.tg[2][k];
    L.iactwp = a.iactwp[k];
  }
  __syncthreads();
  for (int q = 0; q < G.cnt; ++q) {
    const bsa_route_edit_rec r = rec[G.rec0 + q];
    const int pos = r.pos;
    if (r.op == BSA_ROUTE_INSERT) {
      for (int hi = n; hi > pos; hi -= 64) {
        const int lo = hi - 64 > pos ? hi - 64 : pos;
        const int i = lo + lane;
        RowRegs x{};
        if (i < hi) x = row_load(route, rtype, (size_t)i);
        __syncthreads();
        if (i < hi) row_store(route, rtype, (size_t)i + 1, x);
        __syncthreads();
      }
      n += 1;
    } else if (r.op == BSA_ROUTE_DELETE) {
      for (int lo = pos + 1; lo < n; lo += 64) {
        const int i = lo + lane;
        RowRegs x{};
        if (i < n) x = row_load(route, rtype, (size_t)i);
        __syncthreads();
        if (i < n) row_store(route, rtype, (size_t)i - 1, x);
        __syncthreads();
      }
      n -= 1;
    }
    if ((r.op == BSA_ROUTE_INSERT || r.op == BSA_ROUTE_OVERWRITE) && lane == 0) {
      RowRegs x;
      x.v[0] = make_double2(route::wrap_lat(r.lat), route::wrap_lon(r.lon)), x.v[1] = make_double2(r.alt, r.spd);
      x.v[2] = make_double2(0., 0.), x.v[3] = make_double2(r.flyby ? 1. : 0., 0.);
      x.t = (uint8_t)r.wptype;
      row_store(route, rtype, (size_t)pos, x);
    }
    __syncthreads();
    if (r.op != BSA_ROUTE_DIRECT) flight_plan(route, rtype, n);
    if (lane == 0) {
      if (r.op == BSA_ROUTE_DIRECT) {
        fms::direct(L, route, n, pos);
      } else {
        L.iactwp = route::iactwp_after(r.op, pos, r.bump_active, L.iactwp, n);
        if (r.op == BSA_ROUTE_DELETE) {
          if (n == 0) L.swlnav = false;   // no LNAV without a route (fms_check_routes)
        } else {
          L.next_qdr = (-1 < L.iactwp && L.iactwp < n - 1) ? route[(size_t)L.iactwp * fms::kRouteCols + 7] : -999.;
          if (0 <= L.iactwp && L.iactwp < n) fms::direct(L, route, n, L.iactwp);
        }
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    a.st[0][k] = L.wlat, a.st[1][k] = L.wlon, a.st[2][k] = L.nextaltco, a.st[3][k] = L.xtoalt;
    a.st[4][k] = L.spd, a.st[5][k] = L.vs, a.st[6][k] = L.turndist, a.st[7][k] = L.flyby;
    a.st[8][k] = L.next_qdr, a.st[9][k] = L.dist2vs, a.st[12][k] = L.selspd;
    a.fl[0][k] = L.swlnav ? 1 : 0;
    a.tg[2][k] = L.ap_alt;
    a.iactwp[k] = L.iactwp;
    rt_off[k] = G.dst;
    rt_n[k] = n;
  }
}

// ---- small helpers of the host side: the edited aircraft's counts, the live rows
__global__ __launch_bounds__(256) void k_rt_gather(int ng, const int *__restrict__ h, const int *__restrict__ rt_n,
                                                   int *__restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < ng) out[g] = rt_n[h[g]];
}
__global__ __launch_bounds__(256) void k_rt_sum(int n, const int *__restrict__ rt_n, unsigned long long *__restrict__ sum) {
  unsigned long long s = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += (unsigned)rt_n[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(sum, s);
}

// ---- compaction in aircraft order: counts by aircraft, their exclusive scan,
// one thread per fp64 of the new table (the aircraft by binary search in the
// new offsets), then the offsets repointed
__global__ __launch_bounds__(256) void k_rt_counts(int n, const unsigned *__restrict__ id2h, const int *__restrict__ rt_n,
                                                   unsigned *__restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cnt[i] = (unsigned)rt_n[id2h ? id2h[i] : (unsigned)i];
}
__global__ __launch_bounds__(256) void k_rt_copy(long long total, int n, const unsigned *__restrict__ noff,
                                                 const unsigned *__restrict__ id2h, const int *__restrict__ rt_off,
                                                 const double *__restrict__ src, const uint8_t *__restrict__ stype,
                                                 double *__restrict__ dst, uint8_t *__restrict__ dtype) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long row = e >> 3;
  if (row >= total) return;
  const int col = (int)(e & 7);
  int lo = 0, hi = n;   // the last aircraft whose new offset is <= row: its route holds the row
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long long)noff[mid] <= row) lo = mid;
    else hi = mid;
  }
  const size_t from = (size_t)rt_off[id2h ? id2h[lo] : (unsigned)lo] + (size_t)(row - (long long)noff[lo]);
  dst[(size_t)row * 8 + col] = src[from * 8 + col];
  if (col == 0) dtype[row] = stype[from];
}
__global__ __launch_bounds__(256) void k_rt_repoint(int n, const unsigned *__restrict__ id2h,
                                                    const unsigned *__restrict__ noff, int *__restrict__ rt_off) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rt_off[id2h ? id2h[i] : (unsigned)i] = (int)noff[i];
}

static dim3 blocks(int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

// The table a call works on: device pointers and, for the resident sim, the buffers that grow
struct RouteDev {
  double *rows;
  uint8_t *types;
  int *off, *n;              // by position in the FMS arrays
  const unsigned *id2h;      // aircraft index -> position, NULL = identity
  int64_t naircraft, tail;   // rows in use (live + dead)
};

// Compacts the table of d in aircraft order into (drows, dtypes) (room for the live rows; the caller sized them
// from *live of an earlier call, or passes NULL to only count).  ws: 2 x naircraft words; on return its first
// naircraft words hold the counts and the next the new offsets, both in aircraft order.  repoint: d.off follows
static int compact(Ctx *c, const RouteDev &d, unsigned *ws, double *drows, uint8_t *dtypes, bool repoint, int64_t *live) {
  const int n = (int)d.naircraft;
  *live = 0;
  if (n == 0) return 0;
  unsigned *cnt = ws, *noff = ws + n;
  hipLaunchKernelGGL(k_rt_counts, blocks(n, 256), dim3(256), 0, c->stream, n, d.id2h, (const int *)d.n, cnt);
  BSA_HIP(c, hipGetLastError());
  if (scan_excl(c, cnt, noff, n)) return -1;
  unsigned last[2];
  BSA_HIP(c, hipMemcpyAsync(&last[0], cnt + n - 1, 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(&last[1], noff + n - 1, 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  *live = (int64_t)last[0] + (int64_t)last[1];
  if (!drows) return 0;
  if (*live) {
    hipLaunchKernelGGL(k_rt_copy, blocks(*live * 8, 256), dim3(256), 0, c->stream, (long long)*live, n,
                       (const unsigned *)noff, d.id2h, (const int *)d.off, (const double *)d.rows,
                       (const uint8_t *)d.types, drows, dtypes);
    BSA_HIP(c, hipGetLastError());
  }
  if (repoint) {
    hipLaunchKernelGGL(k_rt_repoint, blocks(n, 256), dim3(256), 0, c->stream, n, d.id2h, (const unsigned *)noff, d.off);
    BSA_HIP(c, hipGetLastError());
  }
  return 0;
}

// A refusal: the message for bsa_last_error, the code for the caller
template <typename... A>
static int refuse(Ctx *c, int code, const char *fmt, A... args) {
  fail(c, fmt, args...);
  return code;
}

// The batch grouped and checked against the routes' counts n0[g] (one per group, in the groups' order)
struct EditPlan {
  std::vector<int32_t> order, gstart;
  std::vector<EditGroup> grp;
  std::vector<bsa_route_edit_rec> recs;  // grouped order
  int64_t ng = 0, need = 0, written = 0, delta = 0;  // rows of the new places; new lengths; live rows gained
};
static int plan_ids(Ctx *c, const char *who, int64_t n, int64_t m, const bsa_route_edit_rec *rec, EditPlan &p) {
  for (int64_t q = 0; q < m; ++q)
    if (rec[q].aircraft < 0 || rec[q].aircraft >= n)
      return refuse(c, BSA_ROUTE_ERR_AIRCRAFT, "%s: record %lld: aircraft %d outside [0, %lld)", who, (long long)q,
                    rec[q].aircraft, (long long)n);
  p.ng = route::group(m, rec, p.order, p.gstart);
  return 0;
}
static int plan_rows(Ctx *c, const char *who, const bsa_route_edit_rec *rec, const int32_t *n0, int64_t tail, EditPlan &p) {
  p.grp.resize((size_t)p.ng);
  p.recs.resize(p.order.size());
  for (size_t q = 0; q < p.order.size(); ++q) p.recs[q] = rec[p.order[q]];
  p.need = p.written = p.delta = 0;
  for (int64_t g = 0; g < p.ng; ++g) {
    const int32_t *ord = p.order.data() + p.gstart[(size_t)g];
    const int cnt = p.gstart[(size_t)g + 1] - p.gstart[(size_t)g];
    int nf = 0, nmax = 0, bad = 0;
    const int e = route::plan(rec, ord, cnt, n0[g], &nf, &nmax, &bad);
    if (e != BSA_ROUTE_OK) {
      const bsa_route_edit_rec &r = rec[ord[bad]];
      return refuse(c, e, "%s: record %d (aircraft %d, op %d, pos %d, waypoint type %d) refused with code %d", who,
                    ord[bad], r.aircraft, r.op, r.pos, r.wptype, e);
    }
    if (tail + p.need + nmax > 0x7fffffff / 8) return fail(c, "%s: the route table would pass 2^31 / 8 rows", who);
    p.grp[(size_t)g] = EditGroup{0, p.gstart[(size_t)g], cnt, (int)(tail + p.need), n0[g]};
    p.need += nmax, p.written += nf, p.delta += nf - n0[g];
  }
  return 0;
}

// Uploads the plan and runs k_route_edit; synchronises (the plan's vectors are pageable)
static int launch(Ctx *c, DevBuf &stage, const EditPlan &p, const RouteDev &d, const FmsArrays &a) {
  if (p.ng == 0) return 0;
  const size_t gb = ((size_t)p.ng * sizeof(EditGroup) + 255) / 256 * 256, rb = p.recs.size() * sizeof(bsa_route_edit_rec);
  if (!ensure(c, stage, gb + rb + 256, "route edit staging")) return -1;
  BSA_HIP(c, hipMemcpyAsync(stage.p, p.grp.data(), (size_t)p.ng * sizeof(EditGroup), hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync((char *)stage.p + gb, p.recs.data(), rb, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_route_edit, dim3((unsigned)p.ng), dim3(64), 0, c->stream, (int)p.ng, (const EditGroup *)stage.p,
                     (const bsa_route_edit_rec *)((const char *)stage.p + gb), d.rows, d.types, d.off, d.n, a);
  BSA_HIP(c, hipGetLastError());
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The resident table: types for every row in use (rows the table got from bsa_sim_set_fms / create are type 0)
static int sim_types(Ctx *c, int64_t rows) {
  if (!ensure_keep(c, c->s_fmstype, (size_t)rows + 64, "route waypoint types")) return -1;
  if (c->fms_ntypes < c->fms_nrows) {
    BSA_HIP(c, hipMemsetAsync((char *)c->s_fmstype.p + c->fms_ntypes, 0, (size_t)(c->fms_nrows - c->fms_ntypes), c->stream));
    c->fms_ntypes = c->fms_nrows;
  }
  return 0;
}
static RouteDev sim_table(Ctx *c) {
  const size_t n = (size_t)c->n;
  return RouteDev{(double *)c->s_fmsrows.p, (uint8_t *)c->s_fmstype.p, (int *)c->s_fmsi.p + n, (int *)c->s_fmsi.p + 2 * n,
                  (const unsigned *)c->id2h.p, c->n, c->fms_nrows};
}
static int sim_live(Ctx *c, int64_t *live) {
  *live = 0;
  if (c->n == 0) return 0;
  if (!ensure(c, c->rt_ws, 2 * (size_t)c->n * 4 + 64, "route scan words")) return -1;
  unsigned long long *sum = (unsigned long long *)c->rt_ws.p, h = 0;
  BSA_HIP(c, hipMemsetAsync(sum, 0, 8, c->stream));
  hipLaunchKernelGGL(k_rt_sum, dim3((unsigned)std::min<int64_t>((c->n + 255) / 256, 1024)), dim3(256), 0, c->stream, (int)c->n,
                     (const int *)c->s_fmsi.p + 2 * (size_t)c->n, sum);
  BSA_HIP(c, hipGetLastError());
  BSA_HIP(c, hipMemcpyAsync(&h, sum, 8, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  *live = (int64_t)h;
  return 0;
}
static int sim_ready(Ctx *c, const char *who) {
  if (!c->sim_ready) return fail(c, "%s before bsa_sim_init", who);
  if (!c->sim_fms) return fail(c, "%s: no route table: bsa_sim_set_fms is off", who);
  if (c->nranks > 1)
    return refuse(c, BSA_ROUTE_ERR_RANKS, "%s with autopilot guidance on several ranks: bsa_sim_set_fms(NULL), edit on the host, set it again", who);
  return 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" int bsa_sim_route_edit(bsa_ctx *cc, int64_t m, const bsa_route_edit_rec *rec) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (int e = bsa::sim_ready(c, "bsa_sim_route_edit")) return e;
  if (m < 0 || m > 0x7fffffff / 64 || (m > 0 && !rec)) return bsa::fail(c, "bsa_sim_route_edit: bad batch");
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::EditPlan p;
  if (int e = bsa::plan_ids(c, "bsa_sim_route_edit", c->n, m, rec, p)) return e;
  if (m == 0) {
    c->rt_written = 0;
    return 0;
  }
  // the edited routes' lengths, by position in the FMS arrays
  std::vector<int32_t> hpos((size_t)p.ng), n0((size_t)p.ng);
  for (int64_t g = 0; g < p.ng; ++g) hpos[(size_t)g] = (int32_t)c->id2h_h[(size_t)rec[p.order[(size_t)p.gstart[(size_t)g]]].aircraft];
  const size_t gb = ((size_t)p.ng * 4 + 255) / 256 * 256;
  if (!bsa::ensure(c, c->rt_stage, 2 * gb + 256, "route edit staging")) return -1;
  BSA_HIP(c, hipMemcpyAsync(c->rt_stage.p, hpos.data(), (size_t)p.ng * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(bsa::k_rt_gather, bsa::blocks(p.ng, 256), dim3(256), 0, c->stream, (int)p.ng, (const int *)c->rt_stage.p,
                     (const int *)c->s_fmsi.p + 2 * (size_t)c->n, (int *)((char *)c->rt_stage.p + gb));
  BSA_HIP(c, hipGetLastError());
  BSA_HIP(c, hipMemcpyAsync(n0.data(), (char *)c->rt_stage.p + gb, (size_t)p.ng * 4, hipMemcpyDeviceToHost, c->stream));
  int64_t live = 0;
  if (bsa::sim_live(c, &live)) return -1;  // synchronises
  if (int e = bsa::plan_rows(c, "bsa_sim_route_edit", rec, n0.data(), c->fms_nrows, p)) return e;
  for (int64_t g = 0; g < p.ng; ++g) p.grp[(size_t)g].h = hpos[(size_t)g];
  // nothing was written so far.  The table grows as bsa_sim_create_with grows it
  const int64_t tail = c->fms_nrows + p.need;
  if (!bsa::ensure_keep(c, c->s_fmsrows, (size_t)tail * 64 + 64, "route table") || bsa::sim_types(c, tail)) return -1;
  const bsa::RouteDev d = bsa::sim_table(c);
  if (bsa::launch(c, c->rt_stage, p, d, bsa::fms_sim_arrays(c))) return -1;
  c->fms_nrows = c->fms_ntypes = tail;
  c->rt_written = p.written;
  live += p.delta;
  if (tail - live > live) {   // dead rows outnumber the live ones: compact in aircraft order
    if (!bsa::ensure(c, c->s_fmsrows2, (size_t)live * 64 + 64, "route table (compacted)") ||
        !bsa::ensure(c, c->s_fmstype2, (size_t)live + 64, "route waypoint types (compacted)"))
      return -1;
    int64_t got = 0;
    if (bsa::compact(c, bsa::sim_table(c), (unsigned *)c->rt_ws.p + 2, (double *)c->s_fmsrows2.p, (uint8_t *)c->s_fmstype2.p,
                     true, &got))
      return -1;
    BSA_HIP(c, hipStreamSynchronize(c->stream));
    if (got != live) return bsa::fail(c, "bsa_sim_route_edit: compaction counted %lld live rows, expected %lld", (long long)got, (long long)live);
    std::swap(c->s_fmsrows, c->s_fmsrows2);
    std::swap(c->s_fmstype, c->s_fmstype2);
    c->fms_nrows = c->fms_ntypes = live;
    c->rt_compactions += 1;
  }
  bsa::invalidate(c, bsa::Change::RouteEdit);
  return 0;
}

extern "C" int bsa_sim_route_rows(bsa_ctx *cc, int64_t *live) {
  Ctx *c = (Ctx *)cc;
  if (!c || !live) return -1;
  if (int e = bsa::sim_ready(c, "bsa_sim_route_rows")) return e;
  BSA_HIP(c, hipSetDevice(c->device));
  return bsa::sim_live(c, live);
}

extern "C" int bsa_sim_route_stats(bsa_ctx *cc, int64_t *live, int64_t *dead, int64_t *written, int64_t *compactions) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (int e = bsa::sim_ready(c, "bsa_sim_route_stats")) return e;
  BSA_HIP(c, hipSetDevice(c->device));
  int64_t l = 0;
  if (bsa::sim_live(c, &l)) return -1;
  if (live) *live = l;
  if (dead) *dead = c->fms_nrows - l;
  if (written) *written = c->rt_written;
  if (compactions) *compactions = c->rt_compactions;
  return 0;
}

extern "C" int bsa_sim_read_routes(bsa_ctx *cc, int64_t cap_rows, double *rows, uint8_t *wptype, int32_t *rt_off,
                                   int32_t *rt_n, int64_t *nrows) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (int e = bsa::sim_ready(c, "bsa_sim_read_routes")) return e;
  if (!rt_off || !rt_n || !nrows || cap_rows < 0 || (cap_rows > 0 && !rows)) return bsa::fail(c, "bsa_sim_read_routes: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  const int64_t n = c->n;
  *nrows = 0;
  if (n == 0) return 0;
  int64_t live = 0;
  if (bsa::sim_live(c, &live)) return -1;
  if (live > cap_rows) return bsa::fail(c, "bsa_sim_read_routes: %lld live rows, room for %lld", (long long)live, (long long)cap_rows);
  if (bsa::sim_types(c, c->fms_nrows)) return -1;
  // compacted into the staging area; the sim's table and offsets stay
  const size_t rb = ((size_t)live * 64 + 255) / 256 * 256;
  if (!bsa::ensure(c, c->rt_stage, rb + (size_t)live + 256, "route read staging")) return -1;
  unsigned *ws = (unsigned *)c->rt_ws.p + 2;
  int64_t got = 0;
  if (bsa::compact(c, bsa::sim_table(c), ws, (double *)c->rt_stage.p, (uint8_t *)c->rt_stage.p + rb, false, &got)) return -1;
  if (live) BSA_HIP(c, hipMemcpyAsync(rows, c->rt_stage.p, (size_t)live * 64, hipMemcpyDeviceToHost, c->stream));
  if (live && wptype) BSA_HIP(c, hipMemcpyAsync(wptype, (char *)c->rt_stage.p + rb, (size_t)live, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(rt_n, ws, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(rt_off, ws + n, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  *nrows = live;
  return 0;
}

extern "C" int bsa_route_edit(bsa_ctx *cc, int64_t n, int64_t nrows, const double *route_rows, const uint8_t *wptype,
                              const int32_t *rt_off, const int32_t *rt_n, int32_t *iactwp, const double *lat,
                              const double *lon, const double *alt, const double *tas, const double *gs,
                              const double *trk, const double *bank, const bsa_fms_state *st, double *ap_alt, int64_t m,
                              const bsa_route_edit_rec *rec, int64_t cap_rows, double *out_rows, uint8_t *out_wptype,
                              int32_t *out_off, int32_t *out_n, int64_t *out_nrows) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  const char *who = "bsa_route_edit";
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "%s: bad n", who);
  if (nrows < 0 || nrows > 0x7fffffff / 16) return bsa::fail(c, "%s: bad route row count", who);
  if (m < 0 || m > 0x7fffffff / 64 || (m > 0 && !rec)) return bsa::fail(c, "%s: bad batch", who);
  if (!st) return bsa::fail(c, "%s: NULL state", who);
  const double *tr[7] = {lat, lon, alt, tas, gs, trk, bank};
  const bsa::FmsFields ff = bsa::fms_fields(*st);
  for (auto q : tr)
    if (!q) return bsa::fail(c, "%s: NULL array", who);
  for (auto q : ff.reals)
    if (!q) return bsa::fail(c, "%s: NULL array", who);
  for (auto q : ff.flags)
    if (!q) return bsa::fail(c, "%s: NULL array", who);
  if (!rt_off || !rt_n || !iactwp || !ap_alt || (nrows > 0 && !route_rows) || !out_off || !out_n || !out_nrows ||
      (cap_rows > 0 && !out_rows))
    return bsa::fail(c, "%s: NULL array", who);
  // the table as the edit kernel reads it; iactwp may be -1 on a route that was never activated
  int64_t live = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t off = rt_off[k], cnt = rt_n[k];
    if (off < 0 || cnt < 0 || off + cnt > nrows)
      return bsa::fail(c, "%s: aircraft %lld: route rows [%lld, %lld) outside the table's %lld", who, (long long)k,
                       (long long)off, (long long)(off + cnt), (long long)nrows);
    if (iactwp[k] < -1 || (iactwp[k] >= cnt && !(cnt == 0 && iactwp[k] == 0)))
      return bsa::fail(c, "%s: aircraft %lld: active waypoint %d outside [-1, %lld)", who, (long long)k, iactwp[k], (long long)cnt);
    live += cnt;
  }
  bsa::EditPlan p;
  if (int e = bsa::plan_ids(c, who, n, m, rec, p)) return e;
  std::vector<int32_t> n0((size_t)p.ng);
  for (int64_t g = 0; g < p.ng; ++g) n0[(size_t)g] = rt_n[rec[p.order[(size_t)p.gstart[(size_t)g]]].aircraft];
  if (int e = bsa::plan_rows(c, who, rec, n0.data(), nrows, p)) return e;
  for (int64_t g = 0; g < p.ng; ++g) p.grp[(size_t)g].h = rec[p.order[(size_t)p.gstart[(size_t)g]]].aircraft;
  const int64_t tail = nrows + p.need, live_after = live + p.delta;
  if (live_after > cap_rows) return bsa::fail(c, "%s: %lld rows after the edit, room for %lld", who, (long long)live_after, (long long)cap_rows);
  *out_nrows = 0;
  if (n == 0) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  // one device block: 7 + 15 + 1 fp64 arrays, 3 int32 + 2 scan arrays, 4 uint8, the table with its new places and
  // types, the compacted table and types
  const size_t N8 = ((size_t)n * 8 + 255) / 256 * 256, N4 = ((size_t)n * 4 + 255) / 256 * 256,
               N1 = ((size_t)n + 255) / 256 * 256;
  const size_t RB = ((size_t)tail * 64 + 255) / 256 * 256, TB = ((size_t)tail + 255) / 256 * 256;
  const size_t CB = ((size_t)live_after * 64 + 255) / 256 * 256, CT = ((size_t)live_after + 255) / 256 * 256;
  constexpr int kD = 7 + bsa::kFmsReals + 1;
  bsa::DevBuf buf, stage;
  struct Rel {
    bsa::DevBuf *a, *b;
    ~Rel() { bsa::release(*a), bsa::release(*b); }
  } rel{&buf, &stage};
  if (!bsa::ensure(c, buf, kD * N8 + 5 * N4 + 4 * N1 + RB + TB + CB + CT + 256, "route edit arrays")) return -1;
  char *base = (char *)buf.p;
  bsa::FmsArrays a{};
  double *d8[kD];
  for (int q = 0; q < kD; ++q) d8[q] = (double *)(base + (size_t)q * N8);
  int *d4[5];
  for (int q = 0; q < 5; ++q) d4[q] = (int *)(base + kD * N8 + (size_t)q * N4);
  uint8_t *d1[4];
  for (int q = 0; q < 4; ++q) d1[q] = (uint8_t *)(base + kD * N8 + 5 * N4 + (size_t)q * N1);
  char *tb = base + kD * N8 + 5 * N4 + 4 * N1;
  double *drows = (double *)tb, *crows = (double *)(tb + RB + TB);
  uint8_t *dtypes = (uint8_t *)(tb + RB), *ctypes = (uint8_t *)(tb + RB + TB + CB);
  const int slot[7] = {0, 1, 2, 3, 4, 5, 7};   // FmsArrays::tr without traf.ax
  for (int q = 0; q < 7; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[q], tr[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.tr[slot[q]] = d8[q];
  }
  for (int q = 0; q < bsa::kFmsReals; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[7 + q], ff.reals[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.st[q] = d8[7 + q];
  }
  double *dapalt = d8[7 + bsa::kFmsReals];
  BSA_HIP(c, hipMemcpyAsync(dapalt, ap_alt, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  a.tg[2] = dapalt;
  const int32_t *h4[3] = {iactwp, rt_off, rt_n};
  for (int q = 0; q < 3; ++q) BSA_HIP(c, hipMemcpyAsync(d4[q], h4[q], (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  for (int q = 0; q < 4; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d1[q], ff.flags[q], (size_t)n, hipMemcpyHostToDevice, c->stream));
    a.fl[q] = d1[q];
  }
  if (nrows) BSA_HIP(c, hipMemcpyAsync(drows, route_rows, (size_t)nrows * 64, hipMemcpyHostToDevice, c->stream));
  if (wptype && nrows) BSA_HIP(c, hipMemcpyAsync(dtypes, wptype, (size_t)nrows, hipMemcpyHostToDevice, c->stream));
  else BSA_HIP(c, hipMemsetAsync(dtypes, 0, TB, c->stream));
  a.iactwp = d4[0];
  a.rt_off = d4[1], a.rt_n = d4[2], a.rows = drows;
  const bsa::RouteDev d{drows, dtypes, d4[1], d4[2], nullptr, n, tail};
  if (bsa::launch(c, stage, p, d, a)) return -1;
  int64_t got = 0;
  if (bsa::compact(c, d, (unsigned *)d4[3], crows, ctypes, false, &got)) return -1;
  if (got != live_after) return bsa::fail(c, "%s: %lld rows after the edit, expected %lld", who, (long long)got, (long long)live_after);
  for (int q = 0; q < bsa::kFmsMutable; ++q)
    BSA_HIP(c, hipMemcpyAsync(ff.reals[q], d8[7 + q], (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(ap_alt, dapalt, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  for (int q = 0; q < 2; ++q) BSA_HIP(c, hipMemcpyAsync(ff.flags[q], d1[q], (size_t)n, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(iactwp, d4[0], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (got) BSA_HIP(c, hipMemcpyAsync(out_rows, crows, (size_t)got * 64, hipMemcpyDeviceToHost, c->stream));
  if (got && out_wptype) BSA_HIP(c, hipMemcpyAsync(out_wptype, ctypes, (size_t)got, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(out_n, d4[3], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(out_off, (unsigned *)d4[3] + n, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  *out_nrows = got;
  return 0;
}
