// What the kernels over a scrub descriptor share (gf_scrub.hip, gf_correct.hip, gf_checked.hip): the
// per-lane syndrome of a column unit, the hot pass's fold of row bits into the mask and its grid,
// the workgroup span, the tile dispatch and the argument rules of their launchers. Include from a
// .hip file only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "gfrs/desc.h"
#include "gfrs/perm_device.h"

namespace gfrs {
namespace scrubdev {

using namespace permdev;

// Syndrome accumulators of one lane's column unit: T = uint8_t (one byte column, any alignment;
// only the low byte of each accumulator is meaningful) or uint32_t (four columns, 4-byte aligned).
// The row loads are issued 8 at a time before any is used, as gf_gemm.hip's tail_byte does.
template <int MT, typename T>
__device__ __forceinline__ void syn_cols(const DescView& d, int n, int m_pad, int i0, int64_t off,
                                         uint32_t (&acc)[MT]) {
  constexpr int kB = 8;
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = 0;
  for (int j0 = 0; j0 < n; j0 += kB) {
    T x[kB];
#pragma unroll
    for (int u = 0; u < kB; ++u) x[u] = j0 + u < n ? *(gptr<const T>)(d.in[j0 + u] + uint64_t(off)) : T(0);
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      const int j = j0 + u;
      if (j < n) {
        const Sel s = make_sel(x[u]);
        const auto t = d.tab + (size_t(j) * m_pad + i0) * kPermStride;
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = mac_map(acc[i], t + i * kPermStride, s);
      }
    }
  }
}

// ---- the hot pass: row bits of a lane's accumulators into the mask (gf_scrub.hip, gf_checked.hip) ----
template <int MT>
__device__ __forceinline__ uint32_t group_bits(const uint32_t (&acc)[MT][4]) {
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) bits |= uint32_t((acc[i][0] | acc[i][1] | acc[i][2] | acc[i][3]) != 0) << i;
  return bits;
}

// OR of the wave's row bits into mask word `blk` (wave-uniform): one ballot when the wave is clean,
// else one per row and a single atomicOr from lane 0. Called with the whole wave converged.
template <int MT>
__device__ __forceinline__ void wave_or(uint32_t rowbits, int shift, int* mask, int64_t blk) {
  if (__builtin_amdgcn_ballot_w64(rowbits != 0) == 0) return;
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < MT; ++i)
    if (__builtin_amdgcn_ballot_w64(((rowbits >> i) & 1u) != 0) != 0) bits |= 1u << i;
  if ((threadIdx.x & 63u) == 0) atomicOr(mask + blk, int(bits << shift));
}

// The mask word of a wave of 16-byte-group lanes whose first lane owns group g0: every group of the
// wave lies in one 4096-byte span (a workgroup's 256 groups), which block_bytes >= 4096 never
// splits, and the ragged tail bytes (lanes ngroups .. ngroups + tail - 1) sit right after group
// ngroups - 1, in the span of group `ngroups`.
__device__ __forceinline__ int64_t wave_block(int64_t g0, int64_t ngroups, int bshift) {
  return ((g0 < ngroups ? g0 : ngroups) * 16) >> bshift;
}

struct Grid {
  int64_t nblk, ncb;
  unsigned blocks;
};

// as gf_gemm.hip's make_grid: at most 2^32 - 1 work-items along x, column blocks padded to a multiple
// of 8 for the XCD map (short grids unpadded)
constexpr int64_t kMaxGridBlocks = int64_t(UINT32_MAX) / kBlock;
inline Grid make_grid(int64_t items, int ntiles) {
  Grid g{};
  g.nblk = (items + kBlock - 1) / kBlock;
  g.ncb = std::min(g.nblk, kMaxGridBlocks / ntiles / 8 * 8);
  const int64_t ncb8 = g.ncb < 8 ? g.ncb : (g.ncb + 7) / 8 * 8;
  g.blocks = static_cast<unsigned>(ncb8 * ntiles);
  return g;
}

constexpr int kLocSpanShift = 14;  // a workgroup covers min(block_bytes, 16 KiB) columns
constexpr int kMaxGridY = 65535;   // stripes per launch, as launch_gf_gemm_batched

template <typename F>
hipError_t dispatch_tile(int t, F&& f) {
  switch (t) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}

inline int log2_exact(int64_t v) {
  int s = 0;
  while ((int64_t(1) << s) < v) ++s;
  return (int64_t(1) << s) == v ? s : -1;
}

inline bool scrub_args_ok(int n, int m_pad, int64_t ncols, int64_t block_bytes) {
  return n >= 1 && n <= 256 && m_pad >= 1 && m_pad % tile_for(m_pad) == 0 && ncols >= 0 && block_bytes >= 4096 &&
         log2_exact(block_bytes) > 0;
}

inline bool locate_args_ok(int n, int p, int64_t ncols, int64_t block_bytes) {
  if (p < 1 || p > 16 || p >= n || !scrub_args_ok(n, pad_m(p), ncols, block_bytes)) return false;
  const int span_shift = std::min(log2_exact(block_bytes), kLocSpanShift);
  return ((ncols + (int64_t(1) << span_shift) - 1) >> span_shift) <= int64_t(INT32_MAX);
}

}  // namespace scrubdev
}  // namespace gfrs
