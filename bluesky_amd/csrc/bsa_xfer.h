// Moving lists of the resident sim's per-aircraft arrays: one
// descriptor (ArrayBatch: up to kBatchMax arrays of element size 1, 4 or 8),
// one element copy (copy_elem) and the two drivers defined in bsa_xfer.hip --
// HomeBatch between the host's aircraft-index order and the device's home
// order, gather_rows between the ranks.  bsa_traffic.hip's k_compact takes the
// same descriptor and copy.
#pragma once
#include "bsa_internal.h"

namespace bsa {

constexpr int kBatchMax = 32;  // (bsa_sim_read_fms moves 25 arrays in one batch)
struct ArrayBatch {
  void *p[kBatchMax];
  int esz[kBatchMax];  // 1, 4 or 8
  int n;
};

// dst[di] = src[si], elements of esz bytes: the only size switch of the movers
__host__ __device__ __forceinline__ void copy_elem(int esz, void *dst, size_t di, const void *src, size_t si) {
  if (esz == 8) ((unsigned long long *)dst)[di] = ((const unsigned long long *)src)[si];
  else if (esz == 4) ((unsigned *)dst)[di] = ((const unsigned *)src)[si];
  else ((unsigned char *)dst)[di] = ((const unsigned char *)src)[si];
}

// Home order (host side): arrays cross the ABI in aircraft-index order and live
// on the device in home order (Ctx::h2id_h).  HomeBatch is the one way between
// the two: the arrays of a batch cross PCIe through the pinned stage in ONE
// DMA, ONE kernel moves every field between the device arrays and the staging
// area, one stream synchronisation per batch (a host permutation loop and a
// synchronisation per array cost the ASAS drop-in ~0.2 ms per array at 100k
// aircraft).  Upload and download of all rows: index order in the staging
// area, stage[h2id[h]] <-> dev[h].  Download of a rank's rows [hb, he): packed,
// stage[h - hb] = dev[h]; the host then writes host[h2id[h]] for these rows and
// no other entry.  A batch that is full runs before the next array is added; a
// rank without rows launches nothing
enum XferMode { kXferUp, kXferDown, kXferDownPacked };
struct StageOffsets {
  unsigned long long b[kBatchMax];  // byte offset of each array in the staging area
};
struct HomeBatch {
  Ctx *c;
  int64_t hb, he;  // home rows (an upload: all)
  int mode;
  ArrayBatch dev{};
  StageOffsets off{};
  const void *hsrc[kBatchMax] = {};
  void *hdst[kBatchMax] = {};
  size_t bytes = 0;
  HomeBatch(Ctx *cc, bool upload, int64_t hb_ = 0, int64_t he_ = -1);
  // upload: device array dev <- host src (index order); download: host dst <- dev
  int add(const void *dev_, const void *hsrc_, void *hdst_, int esz);
  int run();
};

// One all-gather (RCCL or the in-process group) of every rank's rows
// [sim_rb, sim_re) of the listed full-n device arrays, staged in Ctx::g_send /
// g_recv, kBatchMax arrays per collective.  sync: the stream is synchronised
// before returning; else the caller's next synchronisation covers it
struct ArrayRef {
  void *p;
  int esz;
};
int gather_rows(Ctx *c, const std::vector<ArrayRef> &arrs, bool sync);

}  // namespace bsa
