// The two drivers that move lists of the resident sim's per-aircraft arrays
// (bsa_xfer.h): HomeBatch (host index order <-> device home
// order through the pinned stage) and gather_rows (every rank's rows to every
// rank).  Neither runs inside a step.
#include <algorithm>

#include "bsa_xfer.h"

namespace bsa {

__global__ __launch_bounds__(256) void k_home_xfer(int hb, int he, int mode, ArrayBatch a, StageOffsets off,
                                                   const unsigned *__restrict__ h2id,
                                                   unsigned char *__restrict__ stage) {
  const int h = hb + blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= he) return;
  const unsigned i = mode == kXferDownPacked ? (unsigned)(h - hb) : h2id[h];
  for (int q = 0; q < a.n; ++q) {
    if (mode == kXferUp) copy_elem(a.esz[q], a.p[q], h, stage + off.b[q], i);
    else copy_elem(a.esz[q], stage + off.b[q], i, a.p[q], h);
  }
}

// host: dst[ids[r]] = src[r] (a rank's packed rows into the caller's index-order array)
static void scatter_rows(int esz, void *dst, const void *src, const unsigned *ids, int64_t rows) {
  for (int64_t r = 0; r < rows; ++r) copy_elem(esz, dst, ids[r], src, (size_t)r);
}

HomeBatch::HomeBatch(Ctx *cc, bool upload, int64_t hb_, int64_t he_) : c(cc), hb(hb_), he(he_ < 0 ? cc->n : he_) {
  mode = upload ? kXferUp : hb == 0 && he == c->n ? kXferDown : kXferDownPacked;
}

int HomeBatch::add(const void *dev_, const void *hsrc_, void *hdst_, int esz) {
  if (dev.n == kBatchMax && run()) return -1;
  const int q = dev.n++;
  dev.p[q] = const_cast<void *>(dev_);
  dev.esz[q] = esz;
  off.b[q] = bytes;
  hsrc[q] = hsrc_;
  hdst[q] = hdst_;
  bytes += ((size_t)std::max<int64_t>(he - hb, 0) * esz + 255) / 256 * 256;
  return 0;
}

int HomeBatch::run() {
  const int64_t rows = he - hb;
  const bool up = mode == kXferUp;
  const ArrayBatch a = dev;
  const size_t total = bytes;
  dev.n = 0;  // (the batch is empty again, whatever happens below)
  bytes = 0;
  if (a.n == 0 || rows <= 0) return 0;  // (a rank without rows: nothing to launch)
  if (!ensure(c, c->xfer_stage, total, "transfer staging")) return -1;
  unsigned char *st = (unsigned char *)c->xfer_stage.p;
  // the host side through the pinned staging: one parallel host copy and
  // ONE DMA of the whole batch (pin_stage, bsa_ctx.hip)
  unsigned char *pin = pin_stage(c, total);
  if (!pin) return -1;
  HostCopy jobs[kBatchMax];
  if (up) {
    for (int q = 0; q < a.n; ++q) jobs[q] = HostCopy{pin + off.b[q], hsrc[q], (size_t)rows * a.esz[q]};
    host_copy(jobs, a.n);
    BSA_HIP(c, hipMemcpyAsync(st, pin, total, hipMemcpyHostToDevice, c->stream));
  }
  hipLaunchKernelGGL(k_home_xfer, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, (int)hb, (int)he, mode,
                     a, off, (const unsigned *)c->h2id.p, st);
  BSA_HIP(c, hipGetLastError());
  if (!up) BSA_HIP(c, hipMemcpyAsync(pin, st, total, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  if (mode == kXferDown) {
    for (int q = 0; q < a.n; ++q) jobs[q] = HostCopy{hdst[q], pin + off.b[q], (size_t)rows * a.esz[q]};
    host_copy(jobs, a.n);
  } else if (mode == kXferDownPacked) {
    const unsigned *ids = c->h2id_h.data() + hb;
    for (int q = 0; q < a.n; ++q) scatter_rows(a.esz[q], hdst[q], pin + off.b[q], ids, rows);
  }
  return 0;
}

// this rank's rows [rb, re) of every array into its block (array k at rpr x
// (sum of the earlier arrays' element sizes)); the rows of the block past re
// stay unwritten: k_rows_unpack reads a block's rows below n only
__global__ __launch_bounds__(256) void k_rows_pack(int rb, int re, int rpr, ArrayBatch b, char *__restrict__ send) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rpr || rb + r >= re) return;
  size_t off = 0;
  for (int k = 0; k < b.n; ++k) {
    copy_elem(b.esz[k], send + off, r, b.p[k], rb + r);
    off += (size_t)rpr * b.esz[k];
  }
}

__global__ __launch_bounds__(256) void k_rows_unpack(int n, int rpr, int me, int rowbytes, ArrayBatch b,
                                                     const char *__restrict__ recv) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= n) return;
  const int q = h / rpr, r = h - q * rpr;
  if (q == me) return;
  const char *blk = recv + (size_t)q * rpr * rowbytes;
  size_t off = 0;
  for (int k = 0; k < b.n; ++k) {
    copy_elem(b.esz[k], b.p[k], h, blk + off, r);
    off += (size_t)rpr * b.esz[k];
  }
}

int gather_rows(Ctx *c, const std::vector<ArrayRef> &arrs, bool sync) {
  const int64_t n = c->n, rpr = c->sim_rpr;
  for (size_t k0 = 0; k0 < arrs.size(); k0 += kBatchMax) {
    ArrayBatch b{};
    int rowbytes = 0;
    for (size_t k = k0; k < arrs.size() && b.n < kBatchMax; ++k) {
      b.p[b.n] = arrs[k].p;
      b.esz[b.n++] = arrs[k].esz;
      rowbytes += arrs[k].esz;
    }
    const size_t blk = (size_t)rpr * rowbytes;
    if (!ensure(c, c->g_send, blk, "gather send") || !ensure(c, c->g_recv, blk * c->nranks, "gather recv")) return -1;
    hipLaunchKernelGGL(k_rows_pack, dim3((unsigned)((rpr + 255) / 256)), dim3(256), 0, c->stream, (int)c->sim_rb,
                       (int)c->sim_re, (int)rpr, b, (char *)c->g_send.p);
    BSA_HIP(c, hipGetLastError());
    if (comm_allgather(c, c->g_send.p, c->g_recv.p, blk)) return -1;
    hipLaunchKernelGGL(k_rows_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (int)n, (int)rpr,
                       c->rank, rowbytes, b, (const char *)c->g_recv.p);
    BSA_HIP(c, hipGetLastError());
  }
  if (sync) BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace bsa
