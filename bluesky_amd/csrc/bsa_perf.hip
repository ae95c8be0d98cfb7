// OpenAP drag / thrust / fuel flow (the second half of OpenAP.update,
// perfoap.py:133-173): the standalone kernel over host arrays
// (bsa_openap_forces) and the resident step's own launch (k_sim_forces,
// bsa_sim_set_forces), one lane per aircraft.  A kernel of its own, not more
// registers in K4': the fused K2 + K4' kernel is latency-bound at about two
// waves per SIMD.
//
// The per-type parameters (a few KB) are staged in LDS by every workgroup --
// 16 doubles of the force table + the lift type of the 24-column table per
// type -- so a lane's row read is an LDS read, not a 16-double gather from HBM.
#include <vector>

#include "bsa_perf_math.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

struct ForceIn {
  const double *tas, *vs, *alt, *mass;
  const int *type;
  const uint8_t *phase;    // explicit flight phase, or NULL: kin::openap_phase of the lift type, vs, alt
  const double *ptab, *ftab;  // 24-column type table, force table
  const perf::ForceConst *fc;
  int ntypes;
};
struct ForceOut {
  double *cd0, *drag, *tr, *thrust, *ff, *bank;  // bank: in (the previous perf.bank) and out
};

__global__ void k_force_consts(perf::ForceConst *out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = perf::force_consts();
}

extern __shared__ double s_ftab[];  // ntypes x perf::kStageCols

__device__ __forceinline__ void stage_table(const ForceIn &in) {
  for (int i = threadIdx.x; i < in.ntypes * perf::kStageCols; i += blockDim.x) {
    const int t = i / perf::kStageCols, q = i - t * perf::kStageCols;
    s_ftab[i] = q < perf::kForceCols ? in.ftab[t * perf::kForceCols + q] : in.ptab[t * kin::kPerfCols + 22];
  }
  __syncthreads();
}

__device__ __forceinline__ perf::Forces forces_row(const ForceIn &in, int k, double bank) {
  const double *r = s_ftab + in.type[k] * perf::kStageCols;
  const double lift = r[perf::kForceCols];
  const double vs = in.vs[k], alt = in.alt[k];
  const int ph = in.phase ? (int)in.phase[k] : kin::openap_phase(lift, vs, alt);
  return perf::forces(r, lift, ph, in.mass[k], in.tas[k], vs, alt, bank, *in.fc);
}

__device__ __forceinline__ void store_row(const ForceOut &o, int k, const perf::Forces &f) {
  o.cd0[k] = f.cd0;
  o.drag[k] = f.drag;
  o.tr[k] = f.thrustratio;
  o.thrust[k] = f.thrust;
  o.ff[k] = f.fuelflow;
  o.bank[k] = f.bank;
}

// the standalone producer: aircraft [0, n)
__global__ __launch_bounds__(256) void k_openap_forces(int n, ForceIn in, ForceOut out) {
  stage_table(in);
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  store_row(out, k, forces_row(in, k, out.bank[k]));
}

// The resident step's launch, first on the step's stream: rows [rb, re) of the
// PRE-step state (OpenAP.update runs before the pilot and the kinematics,
// traffic.py:397-404).  Behind the batch's sticky abort word it changes
// nothing, like every kernel that writes persistent state.  commit: the fuel
// of the step before (pending) is a completed step's -- add it to fuel_used;
// then pending becomes this step's fuelflow x simdt.
__global__ __launch_bounds__(256) void k_sim_forces(int rb, int re, ForceIn in, ForceOut out,
                                                    double *__restrict__ fuel_used, double *__restrict__ pending,
                                                    const unsigned *__restrict__ sticky, double simdt, int commit) {
  if (*sticky != 0u) return;
  stage_table(in);
  const int k = rb + blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= re) return;
  if (commit) fuel_used[k] = fuel_used[k] + pending[k];
  const perf::Forces f = forces_row(in, k, out.bank[k]);
  store_row(out, k, f);
  pending[k] = f.fuelflow * simdt;
}

int forces_consts(Ctx *c) {
  if (c->f_const.p) return 0;
  if (!ensure(c, c->f_const, sizeof(perf::ForceConst), "OpenAP thrust constants")) return -1;
  hipLaunchKernelGGL(k_force_consts, dim3(1), dim3(64), 0, c->stream, (perf::ForceConst *)c->f_const.p);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

static size_t stage_bytes(int64_t ntypes) { return (size_t)ntypes * perf::kStageCols * sizeof(double); }

int forces_sim_launch(Ctx *c, bool commit) {
  const int64_t rb = c->sim_rb, re = c->sim_re, n = c->n;
  if (re <= rb) return 0;
  ForceIn in{(const double *)c->s_tas.p, (const double *)c->own[5].p, (const double *)c->own[4].p,
             (const double *)c->s_fmass.p, (const int *)c->s_ptype.p, nullptr, (const double *)c->s_ptab.p,
             (const double *)c->s_ftab.p, (const perf::ForceConst *)c->f_const.p, (int)c->sim_ntypes};
  double *o = (double *)c->s_fout.p;
  ForceOut out{o, o + n, o + 2 * n, o + 3 * n, o + 4 * n, o + 5 * n};
  hipLaunchKernelGGL(k_sim_forces, dim3((unsigned)((re - rb + 255) / 256)), dim3(256), stage_bytes(c->sim_ntypes),
                     c->stream, (int)rb, (int)re, in, out, (double *)c->s_fused.p, (double *)c->s_fpend.p,
                     (const unsigned *)((const char *)c->sim_ctl.p + kSimCtlSticky), c->simp.simdt, commit ? 1 : 0);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

void forces_off(Ctx *c) { c->sim_forces = false; }

// bsa_sim_create_with's hook (bsa_internal.h): the mass; the outputs and the fuel accumulators stay at the zeros
int forces_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x) {
  if (!c->sim_forces) return 0;
  BSA_HIP(c, hipMemcpyAsync((double *)c->s_fmass.p + n, x.mass, (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
  return 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" int bsa_sim_set_forces(bsa_ctx *cc, int64_t ntypes, const double *ftable, const double *mass) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_forces before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  if (!ftable) {
    bsa::forces_off(c);
    return 0;
  }
  if (!c->sim_perf) return bsa::fail(c, "bsa_sim_set_forces needs the type table and index of bsa_sim_set_perf");
  if (!mass) return bsa::fail(c, "bsa_sim_set_forces: NULL mass");
  if (ntypes != c->sim_ntypes)
    return bsa::fail(c, "bsa_sim_set_forces: %lld force-table rows for the %lld types of bsa_sim_set_perf",
                     (long long)ntypes, (long long)c->sim_ntypes);
  if (ntypes > bsa::perf::kForceTypesMax)
    return bsa::fail(c, "bsa_sim_set_forces: %lld types, at most %d", (long long)ntypes, bsa::perf::kForceTypesMax);
  // thr0 = engnum x engthrust divides the thrust ratio of every fixed wing
  std::vector<double> tab24((size_t)ntypes * bsa::kin::kPerfCols);
  BSA_HIP(c, hipMemcpyAsync(tab24.data(), c->s_ptab.p, tab24.size() * 8, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  for (int64_t t = 0; t < ntypes; ++t) {
    const double thr0 = ftable[t * bsa::perf::kForceCols + 1] * ftable[t * bsa::perf::kForceCols + 2];
    if (tab24[(size_t)t * bsa::kin::kPerfCols + 22] == 1.0 && !std::isfinite(thr0))
      return bsa::fail(c, "type %lld: engnum x engthrust is not finite", (long long)t);
  }
  const int64_t n = c->n;
  const size_t N8 = (size_t)n * 8;
  if (!bsa::ensure(c, c->s_ftab, (size_t)ntypes * bsa::perf::kForceCols * 8, "OpenAP force table") ||
      !bsa::ensure(c, c->s_fmass, N8, "mass") || !bsa::ensure(c, c->s_fout, 6 * N8, "OpenAP forces") ||
      !bsa::ensure(c, c->s_fused, N8, "fuel used") || !bsa::ensure(c, c->s_fpend, N8, "pending fuel"))
    return -1;
  if (bsa::forces_consts(c)) return -1;
  BSA_HIP(c, hipMemcpyAsync(c->s_ftab.p, ftable, (size_t)ntypes * bsa::perf::kForceCols * 8, hipMemcpyHostToDevice,
                            c->stream));
  bsa::HomeBatch up(c, true);
  if (up.add(c->s_fmass.p, mass, nullptr, 8) || up.run()) return -1;
  // switching on: outputs (perf.bank among them) and the fuel accumulators start at 0
  BSA_HIP(c, hipMemsetAsync(c->s_fout.p, 0, 6 * N8, c->stream));
  BSA_HIP(c, hipMemsetAsync(c->s_fused.p, 0, N8, c->stream));
  BSA_HIP(c, hipMemsetAsync(c->s_fpend.p, 0, N8, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  c->sim_forces = true;
  return 0;
}

extern "C" int bsa_sim_read_forces(bsa_ctx *cc, double *cd0, double *drag, double *thrustratio, double *thrust,
                                   double *fuelflow, double *bank, double *fuel_used) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read_forces before bsa_sim_init");
  if (!c->sim_forces) return bsa::fail(c, "no forces: bsa_sim_set_forces is off");
  BSA_HIP(c, hipSetDevice(c->device));
  const int64_t n = c->n, rb = c->sim_rb, re = c->sim_re;
  bsa::HomeBatch down(c, false, rb, re);
  double *dst[6] = {cd0, drag, thrustratio, thrust, fuelflow, bank};
  for (int k = 0; k < 6; ++k)
    if (dst[k] && down.add((const double *)c->s_fout.p + (size_t)k * n, nullptr, dst[k], 8)) return -1;
  // fuel burnt: the committed steps + the last completed step's share, added
  // here as the next step's launch will add it (one fp64 add: the same bits)
  std::vector<double> pend(fuel_used ? (size_t)n : 0, 0.0);
  if (fuel_used && (down.add(c->s_fused.p, nullptr, fuel_used, 8) || down.add(c->s_fpend.p, nullptr, pend.data(), 8)))
    return -1;
  if (down.run()) return -1;
  for (int64_t h = rb; fuel_used && h < re; ++h) {
    const unsigned i = c->h2id_h[(size_t)h];
    fuel_used[i] = fuel_used[i] + pend[i];
  }
  return 0;
}

extern "C" int bsa_openap_forces(bsa_ctx *cc, int64_t n, int64_t ntypes, const double *table, const double *ftable,
                                 const int32_t *type_idx, const uint8_t *phase, const double *mass, const double *tas,
                                 const double *vs, const double *alt, double *cd0, double *drag, double *thrustratio,
                                 double *thrust, double *fuelflow, double *bank) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_openap_forces: bad n");
  if (ntypes < 1 || ntypes > bsa::perf::kForceTypesMax)
    return bsa::fail(c, "bsa_openap_forces: %lld types (1 .. %d)", (long long)ntypes, bsa::perf::kForceTypesMax);
  const void *need[] = {table, ftable, type_idx, mass, tas, vs, alt, cd0, drag, thrustratio, thrust, fuelflow, bank};
  for (auto q : need)
    if (!q) return bsa::fail(c, "bsa_openap_forces: NULL array");
  // every index, lift type and phase is checked here: the kernel reads the staged table unguarded
  for (int64_t t = 0; t < ntypes; ++t) {
    const double lt = table[t * bsa::kin::kPerfCols + 22];
    if (lt != 0.0 && lt != 1.0 && lt != 2.0) return bsa::fail(c, "type %lld: lifttype must be 0, 1 or 2", (long long)t);
  }
  for (int64_t k = 0; k < n; ++k) {
    if (type_idx[k] < 0 || type_idx[k] >= ntypes)
      return bsa::fail(c, "aircraft %lld: type index %d outside [0, %lld)", (long long)k, type_idx[k], (long long)ntypes);
    if (phase && phase[k] > 8) return bsa::fail(c, "aircraft %lld: flight phase %d outside 0..8", (long long)k, (int)phase[k]);
  }
  if (n == 0) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  if (bsa::forces_consts(c)) return -1;
  // one device block: 4 inputs + 6 outputs (fp64), the type index, the phase, the two tables
  const size_t N8 = ((size_t)n * 8 + 255) / 256 * 256, N4 = ((size_t)n * 4 + 255) / 256 * 256,
               N1 = ((size_t)n + 255) / 256 * 256;
  const size_t tb = (size_t)ntypes * bsa::kin::kPerfCols * 8, fb = (size_t)ntypes * bsa::perf::kForceCols * 8;
  bsa::DevBuf buf;
  struct Rel {
    bsa::DevBuf *b;
    ~Rel() { bsa::release(*b); }
  } rel{&buf};
  if (!bsa::ensure(c, buf, 10 * N8 + N4 + N1 + tb + fb, "OpenAP forces staging")) return -1;
  char *base = (char *)buf.p;
  double *d8[10];
  for (int q = 0; q < 10; ++q) d8[q] = (double *)(base + (size_t)q * N8);
  int *dtype = (int *)(base + 10 * N8);
  uint8_t *dph = (uint8_t *)(base + 10 * N8 + N4);
  double *dtab = (double *)(base + 10 * N8 + N4 + N1), *dftab = (double *)(base + 10 * N8 + N4 + N1 + tb);
  const double *hin[5] = {tas, vs, alt, mass, bank};
  const int slot[5] = {0, 1, 2, 3, 9};
  for (int q = 0; q < 5; ++q)
    BSA_HIP(c, hipMemcpyAsync(d8[slot[q]], hin[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(dtype, type_idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if (phase) BSA_HIP(c, hipMemcpyAsync(dph, phase, (size_t)n, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(dtab, table, tb, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(dftab, ftable, fb, hipMemcpyHostToDevice, c->stream));
  bsa::ForceIn in{d8[0], d8[1], d8[2], d8[3], dtype, phase ? dph : nullptr, dtab, dftab,
                  (const bsa::perf::ForceConst *)c->f_const.p, (int)ntypes};
  bsa::ForceOut out{d8[4], d8[5], d8[6], d8[7], d8[8], d8[9]};
  hipLaunchKernelGGL(bsa::k_openap_forces, dim3((unsigned)((n + 255) / 256)), dim3(256), bsa::stage_bytes(ntypes),
                     c->stream, (int)n, in, out);
  BSA_HIP(c, hipGetLastError());
  double *hout[6] = {cd0, drag, thrustratio, thrust, fuelflow, bank};
  for (int q = 0; q < 6; ++q)
    BSA_HIP(c, hipMemcpyAsync(hout[q], d8[4 + q], (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}
