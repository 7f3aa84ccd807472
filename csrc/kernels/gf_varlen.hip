// Variable-length batched encode / in-place repair on gfx950: `batch` stripes of one code per launch,
// each with a row length OF ITS OWN (objects of mixed sizes) and an erasure pattern of its own.
//
// Per stripe b, over byte columns [0, len[b]):
//     out_i[c] = XOR_j L_q[i][j](in_j[c])      i < e_q, j < k,  q = pat[b]
// which is gf_repair.hip's math on gf_repair.hip's code (gfrs/repair_device.h and
// gfrs/repair_group_body.h: the five-word v_perm
// records, so GF(2^8) coefficients and the GF(16) nibble maps; the lane walks output tiles of
// MT = min(4, m_pad) rows over a static ring of 4 input rows consumed in pairs; non-temporal loads
// and stores; the ragged tail of a row one byte per lane in the same launch; a byte-per-lane form
// for a launch with any row that is not 16-byte aligned; no LDS, no atomics, every address formed in
// 64 bits). An encode is the one-pattern case: in = the natives, out = the parity rows, tables of E.
//
// What is new is the grid. gf_repair.hip launches (column blocks, stripe): with mixed lengths that
// is batch x blocks(longest) workgroups of which most exit at once. Here the grid is 1-D over a
// flattened work list of (stripe, column block) pairs: stripe b contributes
//     nb[b] = ceil((len[b] / 16 + len[b] % 16) / 256)   blocks in the vector form (one lane per
//                                                       16-byte group, one per ragged tail byte),
//     nb[b] = ceil(len[b] / 256)                        in the byte form,
// none when len[b] == 0, and the record (varlen_layout, gfrs/desc.h) carries
//     blk_stripe[nblk]  int32: the stripe of work item w,
//     first_blk[batch]  int64: the exclusive prefix sum of nb,
//     len[batch]        int64.
// A workgroup reads b = blk_stripe[w] through the constant address space and moves it into an SGPR
// (sgpr_int); a workgroup never spans two stripes, so everything per stripe (row pointers, pattern,
// table block, length) is wave-uniform and read with scalar loads. Its column block is
// cb = w - first_blk[b]; from there it does what the repair kernel does on column block cb. When the
// grid was capped the kernel strides, w += gridDim.x, and redoes the lookup per item.
//
// The per-block map was chosen over a binary search of the prefix sums: a search is about log2(batch)
// DEPENDENT scalar loads per 4 KiB block of work, the map is one load, costs 4 bytes per 4 KiB of
// chunk columns and is built on the host by one repeat over the stripes. Neither variant has been
// measured against the other.
//
// The grid being flat there is no 65,535-stripe grid.y split: any batch runs as one launch, up to
// nblk < 2^31 work items.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gfrs/desc.h"
#include "gfrs/kernels.h"
#include "gfrs/perm_device.h"
#include "gfrs/repair_device.h"

namespace gfrs {
namespace {

using namespace repairdev;

struct VarlenView {
  RepairView r;           // (the pointers of stripe 0)
  cptr<int64_t> len;      // [batch]
  cptr<int64_t> first;    // [batch]
  cptr<int32_t> blk;      // [nblk]
};

struct Item {
  RepairView v;         // the stripe's own pointers
  cptr<uint32_t> tb;    // its pattern's table block
  int64_t len, cb;      // its length and the item's column block
};

// Work item w: the stripe from the block map, moved into an SGPR; its pointers, pattern, table block
// and length by scalar loads; all offsets formed in 64 bits. Called at the top of the item loop,
// where the wave has reconverged (w and the trip count are wave-uniform).
__device__ __forceinline__ Item item(const VarlenView& a, int k, int m_pad, int64_t w) {
  const uint64_t b = uint32_t(sgpr_int(a.blk[w]));
  Item it;
  it.v = {a.r.in + b * uint64_t(k), a.r.out + b * uint64_t(m_pad), a.r.pat, a.r.tab};
  const int q = sgpr_int(a.r.pat[b]);
  it.tb = a.r.tab + uint64_t(uint32_t(q)) * uint64_t(k) * uint64_t(m_pad) * uint64_t(kPermStride);
  it.len = a.len[b];
  it.cb = w - a.first[b];
  return it;
}

// Vector form: lanes [0, ngroups) of a stripe own a 16-byte group each, lanes [ngroups, ngroups +
// tail) one byte of its ragged tail; a lane past them (the last block of a stripe) does nothing.
template <int MT>
__global__ __launch_bounds__(kBlock) void gf_varlen_vec_kernel(VarlenView a, int k, int m_pad, int64_t nblk) {
  for (int64_t w = blockIdx.x; w < nblk; w += gridDim.x) {
    const Item it = item(a, k, m_pad, w);
    const int64_t ngroups = it.len / 16;
    const int64_t tail = it.len % 16;
    const int64_t g = it.cb * kBlock + threadIdx.x;
    if (g >= ngroups) {
      if (g - ngroups < tail) repair_byte(it.v, it.tb, k, m_pad, ngroups * 16 + (g - ngroups));
      continue;
    }
    const RepairView& v = it.v;
    const auto tb = it.tb;
#include "gfrs/repair_group_body.h"
  }
}

// Byte form: one lane per byte column, rows of any alignment.
__global__ __launch_bounds__(kBlock) void gf_varlen_byte_kernel(VarlenView a, int k, int m_pad, int64_t nblk) {
  for (int64_t w = blockIdx.x; w < nblk; w += gridDim.x) {
    const Item it = item(a, k, m_pad, w);
    const int64_t c = it.cb * kBlock + threadIdx.x;
    if (c < it.len) repair_byte(it.v, it.tb, k, m_pad, c);
  }
}

// as gf_repair.hip: at most 2^32 - 1 work-items along x, the kernels stride
constexpr int64_t kMaxGridBlocks = int64_t(UINT32_MAX) / kBlock / 8 * 8;

}  // namespace

hipError_t launch_gf_varlen(const void* desc, int k, int m_pad, int batch, int npat, int64_t nblk, bool force_bytewise,
                            int max_blocks, hipStream_t stream) {
  if (!desc || batch < 1 || npat < 1 || k < 1 || k > 256 || m_pad < 1 || m_pad > 256 ||
      m_pad % tile_for(m_pad) != 0 || nblk < 0 || nblk > int64_t(INT32_MAX) || max_blocks < 0)
    return hipErrorInvalidValue;
  if (nblk == 0) return hipSuccess;
  const VarlenLayout l = varlen_layout(k, m_pad, batch, npat, nblk);
  const char* base = static_cast<const char*>(desc);
  const VarlenView a{{(cptr<uint64_t>)(base + l.in_off), (cptr<uint64_t>)(base + l.out_off),
                      (cptr<int32_t>)(base + l.pat_off), (cptr<uint32_t>)(base + l.tab_off)},
                     (cptr<int64_t>)(base + l.len_off),
                     (cptr<int64_t>)(base + l.first_off),
                     (cptr<int32_t>)(base + l.blk_off)};
  const unsigned grid = unsigned(std::min(nblk, max_blocks ? int64_t(max_blocks) : kMaxGridBlocks));
  if (force_bytewise)
    gf_varlen_byte_kernel<<<grid, kBlock, 0, stream>>>(a, k, m_pad, nblk);
  else if (m_pad == 1)
    gf_varlen_vec_kernel<1><<<grid, kBlock, 0, stream>>>(a, k, m_pad, nblk);
  else if (m_pad == 2)
    gf_varlen_vec_kernel<2><<<grid, kBlock, 0, stream>>>(a, k, m_pad, nblk);
  else
    gf_varlen_vec_kernel<4><<<grid, kBlock, 0, stream>>>(a, k, m_pad, nblk);
  return hipGetLastError();
}

}  // namespace gfrs
