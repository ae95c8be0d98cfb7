// The 3-D wind field (winddim 3): Windfield.getdata with altitude profiles
// (bluesky/traffic/windfield.py:158-202) per aircraft, a kernel of its own in
// front of the kinematic kernels (math: kin::windfield_3d, bsa_kin_math.h).
//
// k_wind3d writes each aircraft's (vnorth, veast) at its pre-step position and
// altitude; k_kinematics, K4' and K2 + K4' then read the two values like a
// per-aircraft constant wind (WindField::vn / ve), so none of them carries the
// O(nvec) loop or its registers.  One lane per aircraft: per
// point one fp64 cos, one divide and two 16-byte table reads; the point
// coordinates are wave-uniform reads.  Fields of up to kWindCachePts points keep
// their weights in LDS between the sum pass and the product pass (one column
// per lane, conflict-free) instead of evaluating the cos twice.
// bsa_wind_getdata is the same evaluation (and the 1-D / 2-D one) at
// host-given positions.
#include <vector>

#include "bsa_kin_math.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kWindBlock = 256;
constexpr int kWindCachePts = 16;  // 16 x 256 lanes x 8 B = 32 KiB of LDS per workgroup

// a lane's column of the workgroup's weight cache
struct WindLdsCache {
  static constexpr int kMax = kWindCachePts;
  double *col;
  __device__ __forceinline__ void put(int k, double v) const { col[k * kWindBlock] = v; }
  __device__ __forceinline__ double get(int k) const { return col[k * kWindBlock]; }
};

// rows [rb, re) of lat / lon / alt -> the same rows of vn / ve
template <bool CACHE>
__global__ __launch_bounds__(kWindBlock) void k_wind3d(int rb, int re, const double *__restrict__ lat,
                                                         const double *__restrict__ lon,
                                                         const double *__restrict__ alt, WindField3D w,
                                                         double *__restrict__ vn, double *__restrict__ ve) {
  const int k = rb + blockIdx.x * kWindBlock + threadIdx.x;
  if (k >= re) return;
  double n, e;
  if (CACHE) {
    __shared__ double sw[kWindCachePts * kWindBlock];
    kin::windfield_3d(w, lat[k], lon[k], alt[k], WindLdsCache{sw + threadIdx.x}, n, e);
  } else {
    kin::windfield_3d(w, lat[k], lon[k], alt[k], kin::WindNoCache{}, n, e);
  }
  vn[k] = n;
  ve[k] = e;
}

// Windfield.getdata without altitude profiles at n positions: winddim 1 the
// field's first point (windfield.py:150-152), winddim 2 the 2-D field
__global__ __launch_bounds__(kWindBlock) void k_wind_getdata(int n, int winddim, const double *__restrict__ lat,
                                                               const double *__restrict__ lon, WindField wf,
                                                               double *__restrict__ vn, double *__restrict__ ve) {
  const int k = blockIdx.x * kWindBlock + threadIdx.x;
  if (k >= n) return;
  double a = wf.vn[0], b = wf.ve[0];
  if (winddim == 2) kin::windfield_2d(wf, lat[k], lon[k], a, b);
  vn[k] = a;
  ve[k] = b;
}

static WindField3D wind_field3d(const Ctx *c) {
  WindField3D w;
  const double *p = (const double *)c->wfield3.p;
  w.nvec = (int)c->wf3_nvec;
  w.nalt = (int)c->wf3_nalt;
  w.altstep = c->wf3_altstep;
  w.lat = p;
  w.lon = p + c->wf3_nvec;
  w.tab = (const double2 *)(p + 2 * c->wf3_nvec);
  return w;
}

WindField wind_field_pa(const Ctx *c) {
  WindField w{};
  w.vn = (const double *)c->wind_pa.p;
  w.ve = w.vn ? w.vn + c->wind_pa_n : nullptr;
  return w;
}

// BSA_WIND3D_CACHE=0: every field recomputes its weights (A/B; same bits)
static bool wind_cache_on() {
  static const bool on = [] {
    const char *e = getenv("BSA_WIND3D_CACHE");
    return !(e && e[0] == '0');
  }();
  return on;
}

int wind3d_launch(Ctx *c, int64_t rb, int64_t re, int64_t n, const double *lat, const double *lon,
                  const double *alt) {
  if (c->wf3_nvec < 1) return fail(c, "winddim 3 needs a 3-D wind field (bsa_set_windfield3d)");
  if (rb < 0 || re > n || n > 0x7fffffff) return fail(c, "internal: wind rows [%lld, %lld) of %lld", (long long)rb,
                                                      (long long)re, (long long)n);
  if (!ensure(c, c->wind_pa, (size_t)n * 16, "per-aircraft wind")) return -1;
  c->wind_pa_n = n;
  if (re <= rb) return 0;
  double *vn = (double *)c->wind_pa.p, *ve = vn + n;
  const bool cache = wind_cache_on() && c->wf3_nvec <= kWindCachePts;
  const auto K = cache ? k_wind3d<true> : k_wind3d<false>;
  hipLaunchKernelGGL(K, dim3((unsigned)((re - rb + kWindBlock - 1) / kWindBlock)), dim3(kWindBlock), 0, c->stream,
                     (int)rb, (int)re, lat, lon, alt, wind_field3d(c), vn, ve);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

}  // namespace bsa

extern "C" int bsa_set_windfield3d(bsa_ctx *cc, int64_t nvec, int64_t nalt, double altstep, const double *lat,
                                   const double *lon, const double *vnorth, const double *veast) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (nvec < 0 || nvec > (1 << 20)) return bsa::fail(c, "bad wind field size %lld", (long long)nvec);
  BSA_HIP(c, hipSetDevice(c->device));
  // the field is not a CD input: no kept detect state depends on it (bsa_kept.h)
  bsa::invalidate(c, bsa::Change::WindField);
  if (nvec == 0) {
    c->wf3_nvec = 0;
    return 0;
  }
  if (nalt < 2 || nalt > 65536 || nalt * nvec > (int64_t(1) << 26))
    return bsa::fail(c, "bsa_set_windfield3d: bad table size (%lld levels x %lld points)", (long long)nalt,
                     (long long)nvec);
  if (!(altstep > 0.0) || !(altstep < 1e300)) return bsa::fail(c, "bsa_set_windfield3d: altstep must be > 0");
  if (!lat || !lon || !vnorth || !veast) return bsa::fail(c, "bsa_set_windfield3d: NULL array");
  const size_t cells = (size_t)nalt * nvec;
  // the steps enqueued so far read the old field; ensure() synchronises only when it reallocates
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  c->wf3_nvec = 0;
  if (!bsa::ensure(c, c->wfield3, (2 * (size_t)nvec + 2 * cells) * 8, "3-D wind field")) return -1;
  std::vector<double> h(2 * (size_t)nvec + 2 * cells);
  std::copy(lat, lat + nvec, h.begin());
  std::copy(lon, lon + nvec, h.begin() + nvec);
  double *tab = h.data() + 2 * nvec;
  for (size_t q = 0; q < cells; ++q) {
    tab[2 * q] = vnorth[q];
    tab[2 * q + 1] = veast[q];
  }
  BSA_HIP(c, hipMemcpy(c->wfield3.p, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  c->wf3_nvec = nvec;
  c->wf3_nalt = nalt;
  c->wf3_altstep = altstep;
  return 0;
}

extern "C" int bsa_wind_getdata(bsa_ctx *cc, int winddim, int64_t n, const double *lat, const double *lon,
                                const double *alt, double *vn_out, double *ve_out) {
  bsa::Ctx *c = (bsa::Ctx *)cc;
  if (!c) return -1;
  if (winddim < 1 || winddim > 3) return bsa::fail(c, "bsa_wind_getdata: winddim %d not supported (1, 2 or 3)", winddim);
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bad n");
  if (winddim == 3 && c->wf3_nvec < 1)
    return bsa::fail(c, "winddim 3 needs a 3-D wind field (bsa_set_windfield3d)");
  if (winddim < 3 && c->wf_nvec < 1)
    return bsa::fail(c, "winddim %d needs a wind field (bsa_set_windfield)", winddim);
  if (n == 0) return 0;
  if (!lat || !lon || (winddim == 3 && !alt) || !vn_out || !ve_out)
    return bsa::fail(c, "bsa_wind_getdata: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N8 = (size_t)n * 8;
  if (!bsa::ensure(c, c->wind_stage, 3 * N8, "wind positions")) return -1;
  double *d = (double *)c->wind_stage.p;
  hipStream_t s = c->stream;
  BSA_HIP(c, hipMemcpyAsync(d, lat, N8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d + n, lon, N8, hipMemcpyHostToDevice, s));
  if (winddim == 3) {
    BSA_HIP(c, hipMemcpyAsync(d + 2 * n, alt, N8, hipMemcpyHostToDevice, s));
    if (bsa::wind3d_launch(c, 0, n, n, d, d + n, d + 2 * n)) return -1;
  } else {
    if (!bsa::ensure(c, c->wind_pa, (size_t)n * 16, "per-aircraft wind")) return -1;
    c->wind_pa_n = n;
    double *vn = (double *)c->wind_pa.p;
    hipLaunchKernelGGL(bsa::k_wind_getdata, dim3((unsigned)((n + bsa::kWindBlock - 1) / bsa::kWindBlock)),
                       dim3(bsa::kWindBlock), 0, s, (int)n, winddim, (const double *)d, (const double *)(d + n),
                       bsa::wind_field(c), vn, vn + n);
    BSA_HIP(c, hipGetLastError());
  }
  const double *vn = (const double *)c->wind_pa.p;
  BSA_HIP(c, hipMemcpyAsync(vn_out, vn, N8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipMemcpyAsync(ve_out, vn + n, N8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  return 0;
}
