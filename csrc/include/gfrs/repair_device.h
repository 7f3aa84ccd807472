// Device code shared by the batched repair kernels (gf_repair.hip: stripes of one shape, grid.y =
// stripe; gf_varlen.hip: stripes of differing lengths on a flat grid). Both apply one stripe's
// pattern tables to one column position of that stripe's rows; they differ only in how a workgroup
// finds its stripe and its column block. Here: the view, the row ring's depth and the byte column;
// the 16-byte group's tile walk is gfrs/repair_group_body.h, text that both kernels include in place.
// Included only by .hip translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gfrs/perm_device.h"

namespace gfrs {
namespace repairdev {

using namespace permdev;

// Input rows in flight per lane (16 VGPRs). A ring of 8 holds 90 / 98 / 114 VGPRs (5 / 4 / 4 waves per
// SIMD) against 58 / 66 / 85 (7 / 7 / 5) and was 12-17 % slower on every shape of profiles/repair.
constexpr int kRing = 4;

struct RepairView {
  cptr<uint64_t> in;   // [batch * k]
  cptr<uint64_t> out;  // [batch * m_pad]
  cptr<int32_t> pat;   // [batch]
  cptr<uint32_t> tab;  // [npat][k][m_pad] records
};

__device__ __forceinline__ uint8_t ldb(uint64_t base, int64_t off) {
  return __builtin_nontemporal_load((gptr<const uint8_t>)(base + uint64_t(off)));
}
__device__ __forceinline__ void stb(uint64_t base, int64_t off, uint8_t v) {
  __builtin_nontemporal_store(v, (gptr<uint8_t>)(base + uint64_t(off)));
}

// One byte column at row offset `off` (rows of any alignment): the ragged tail of the vector form
// and every lane of the byte form. `v` holds the pointers of the lane's own stripe, `tb` the table
// block of its pattern. The row bytes are loaded 8 at a time before any is used (as gf_gemm.hip's
// tail_byte); tiles of up to 4 outputs, a tile without an output row skipped.
__device__ __forceinline__ void repair_byte(const RepairView& v, cptr<uint32_t> tb, int k, int m_pad, int64_t off) {
  constexpr int kB = 8;
  for (int i0 = 0; i0 < m_pad; i0 += 4) {
    uint64_t op[4];
    uint32_t acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      op[i] = i0 + i < m_pad ? v.out[i0 + i] : 0;  // (0: a padding output, never touched)
      acc[i] = 0;
    }
    if (!(op[0] | op[1] | op[2] | op[3])) continue;
    for (int j0 = 0; j0 < k; j0 += kB) {
      uint32_t x[kB];
#pragma unroll
      for (int u = 0; u < kB; ++u) x[u] = j0 + u < k ? uint32_t(ldb(v.in[j0 + u], off)) : 0u;
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        const int j = j0 + u;
        if (j < k) {
          const Sel s = make_sel(x[u]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            // a slot past m_pad applies row m_pad - 1's map to an accumulator nobody stores
            const int ii = std::min(i0 + i, m_pad - 1);
            acc[i] = mac_map(acc[i], tb + (size_t(j) * m_pad + ii) * kPermStride, s);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (op[i]) stb(op[i], off, uint8_t(acc[i]));
  }
}

}  // namespace repairdev
}  // namespace gfrs
