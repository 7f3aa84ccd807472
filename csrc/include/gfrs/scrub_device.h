// What the cold-path kernels over a scrub descriptor share (gf_scrub.hip's locate, gf_correct.hip):
// the per-lane syndrome of a column unit, the workgroup span, the tile dispatch and the argument
// rules of their launchers. Include from a .hip file only.
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
