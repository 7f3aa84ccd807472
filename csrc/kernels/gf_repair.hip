// Batched in-place repair on gfx950: `batch` stripes of one shape per launch, each with an erasure
// pattern OF ITS OWN (objects placed over different node sets lose different chunk ids).
//
// Per stripe b, over byte columns [0, ncols):
//     out_i[c] = XOR_j L_q[i][j](in_j[c])      i < e_q, j < k,  q = pat[b]
// in_j are the stripe's k survivor rows, out_i the rows it rewrites, L_q[i][j] the byte map of
// coeff_q[i][j] = (G[erased_q] . inv(G[survivors_q]))[i][j] in the five-word v_perm records of
// gf_gemm.hip, so GF(2^8) coefficients and the GF(16) nibble maps run on the same code. The record is
// repair_batch_layout(k, m_pad, batch, npat) (gfrs/desc.h): the host has resolved the chunk ids into
// row addresses, the kernel reads only pat[b].
//
// What is new against the other batched kernels is that the coefficient tables differ per stripe: a
// repair matrix depends on the whole pattern, so ids into one shared block (gf_update.hip) cannot
// express it. grid.y = stripe, so a wave never spans two stripes and pat[b] is wave-uniform: it is
// read through the constant address space and moved into an SGPR at the top of the kernel
// (sgpr_int), the pattern's table block tab + pat * k * m_pad * kPermStride is formed in 64 bits,
// and from there every table word is a scalar load as in the shared-table kernels.
//
// Vector form: a lane owns one 16-byte group of every row of its stripe. Loads and stores are
// non-temporal; kRing input rows are kept in flight by a static register ring (gf_gemm_vec_kernel's),
// rows consumed in pairs (mac_pair). The output tile is MT = min(4, m_pad) rows. For m_pad > MT the
// LANE walks the tiles, re-reading its own 16 bytes of the k inputs per tile; tiles are not dealt to
// blocks (map_block). Either is race-free here (within a stripe the rows read and the rows written
// are disjoint sets); the walk is chosen because stripes of one launch have different numbers of
// erasures: a tile whose out pointers are all 0 is skipped by one scalar branch, where dealt tiles
// would launch batch x ntiles blocks of which most exit at once when only a few stripes of the batch
// lost more than 4 chunks, and because grid.y already supplies the parallelism that dealing tiles
// buys a single stripe. The second tile's input reads come from the L2 the first tile filled.
// Lanes [ngroups, ngroups + tail) take one byte of the ragged tail each, in the same launch.
//
// Byte form: one lane per byte column, rows of any alignment; taken when any row of any stripe of the
// launch is not 16-byte aligned. No LDS, no atomics; every address is formed in 64 bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gfrs/desc.h"
#include "gfrs/kernels.h"
#include "gfrs/perm_device.h"
#include "gfrs/repair_device.h"

namespace gfrs {
namespace {

using namespace repairdev;  // RepairView, kRing, repair_byte (shared with gf_varlen.hip)

// Stripe b = blockIdx.y: its own k input and m_pad output pointers, and the table block of its
// pattern (returned), all offsets formed in 64 bits and the pattern id moved into an SGPR. Called at
// the top of a kernel, before any divergent branch.
__device__ __forceinline__ cptr<uint32_t> stripe(RepairView& v, int k, int m_pad) {
  const uint64_t b = blockIdx.y;
  v.in += b * uint64_t(k);
  v.out += b * uint64_t(m_pad);
  const int q = sgpr_int(v.pat[b]);
  return v.tab + uint64_t(uint32_t(q)) * uint64_t(k) * uint64_t(m_pad) * uint64_t(kPermStride);
}

// Vector form. MT = output rows per tile = min(4, m_pad), so m_pad is a multiple of MT and every
// tile row has a table column (rows past a pattern's e hold zero maps and a 0 out pointer). Lanes
// [0, ngroups) own a 16-byte group each, lanes [ngroups, ngroups + tail) one byte of the ragged tail;
// the grid strides over the column blocks when it was capped.
template <int MT>
__global__ __launch_bounds__(kBlock) void gf_repair_vec_kernel(RepairView v, int k, int m_pad, int64_t ngroups,
                                                               int tail, int64_t nblk) {
  const auto tb = stripe(v, k, m_pad);
  for (int64_t cb = blockIdx.x; cb < nblk; cb += gridDim.x) {
    const int64_t g = cb * kBlock + threadIdx.x;
    if (g >= ngroups) {
      if (g - ngroups < tail) repair_byte(v, tb, k, m_pad, ngroups * 16 + (g - ngroups));
      continue;
    }
#include "gfrs/repair_group_body.h"
  }
}

// Byte form: one lane per byte column, rows of any alignment.
__global__ __launch_bounds__(kBlock) void gf_repair_byte_kernel(RepairView v, int k, int m_pad, int64_t ncols,
                                                                int64_t nblk) {
  const auto tb = stripe(v, k, m_pad);
  for (int64_t cb = blockIdx.x; cb < nblk; cb += gridDim.x) {
    const int64_t c = cb * kBlock + threadIdx.x;
    if (c < ncols) repair_byte(v, tb, k, m_pad, c);
  }
}

// ---- launch -----------------------------------------------------------------------------------
// as gf_update.hip's make_grid: at most 2^32 - 1 work-items along x, the kernels stride
constexpr int64_t kMaxGridBlocks = int64_t(UINT32_MAX) / kBlock / 8 * 8;
struct Grid {
  int64_t nblk;
  unsigned blocks;
};
inline Grid make_grid(int64_t items) {
  Grid g{};
  g.nblk = (items + kBlock - 1) / kBlock;
  g.blocks = static_cast<unsigned>(std::min(g.nblk, kMaxGridBlocks));
  return g;
}

// One launch over `batch` stripes (grid.y); `v` holds the pointers of the first of them.
hipError_t repair_launch(const RepairView& v, int k, int m_pad, unsigned batch, int64_t ncols, bool force_bytewise,
                         hipStream_t stream) {
  if (force_bytewise) {
    const Grid g = make_grid(ncols);
    gf_repair_byte_kernel<<<dim3(g.blocks, batch), kBlock, 0, stream>>>(v, k, m_pad, ncols, g.nblk);
    return hipGetLastError();
  }
  const int64_t ngroups = ncols / 16;
  const int tail = int(ncols % 16);
  const Grid g = make_grid(ngroups + tail);  // one extra lane per ragged tail byte
  const dim3 grid(g.blocks, batch);
  if (m_pad == 1)
    gf_repair_vec_kernel<1><<<grid, kBlock, 0, stream>>>(v, k, m_pad, ngroups, tail, g.nblk);
  else if (m_pad == 2)
    gf_repair_vec_kernel<2><<<grid, kBlock, 0, stream>>>(v, k, m_pad, ngroups, tail, g.nblk);
  else
    gf_repair_vec_kernel<4><<<grid, kBlock, 0, stream>>>(v, k, m_pad, ngroups, tail, g.nblk);
  return hipGetLastError();
}

constexpr int kMaxGridY = 65535;  // stripes per launch, as launch_gf_update_batched

}  // namespace

hipError_t launch_gf_repair_batched(const void* desc, int k, int m_pad, int batch, int npat, int64_t ncols,
                                    bool force_bytewise, hipStream_t stream) {
  if (!desc || batch < 1 || npat < 1 || k < 1 || k > 256 || m_pad < 1 || m_pad > 256 ||
      m_pad % tile_for(m_pad) != 0 || ncols < 0)
    return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const RepairBatchLayout l = repair_batch_layout(k, m_pad, batch, npat);
  const char* base = static_cast<const char*>(desc);
  const RepairView v0{(cptr<uint64_t>)(base + l.in_off), (cptr<uint64_t>)(base + l.out_off),
                      (cptr<int32_t>)(base + l.pat_off), (cptr<uint32_t>)(base + l.tab_off)};
  hipError_t e = hipSuccess;
  for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridY) {
    RepairView v = v0;  // (the table block is shared by the launches)
    v.in += size_t(b0) * size_t(k);
    v.out += size_t(b0) * size_t(m_pad);
    v.pat += size_t(b0);
    e = repair_launch(v, k, m_pad, unsigned(std::min(batch - b0, kMaxGridY)), ncols, force_bytewise, stream);
  }
  return e;
}

}  // namespace gfrs
