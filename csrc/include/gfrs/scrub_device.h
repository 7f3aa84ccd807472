// What the kernels over a scrub descriptor share (gf_scrub.hip, gf_correct.hip, gf_checked.hip): the
// per-lane syndrome of a column unit, the hot pass's fold of row bits into the mask and its grid,
// the cold pass's scaffold (stripe offsets, span, column sweep, count flush), the tile dispatch, the
// argument rules of their launchers and the slicing of a batch past the grid.y limit. The decoder of
// the cold passes that repair is in correct_device.h. Include from a .hip file only.
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

// bit i: syndrome row i0 + i is nonzero in this byte column
template <int MT>
__device__ __forceinline__ uint32_t syn_byte_bits(const DescView& d, int n, int m_pad, int i0, int64_t off) {
  uint32_t acc[MT];
  syn_cols<MT, uint8_t>(d, n, m_pad, i0, off, acc);
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) bits |= uint32_t((acc[i] & 0xFFu) != 0) << i;
  return bits;
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

// mask words of one stripe: one per block of 2^bshift columns
__host__ __device__ inline int64_t mask_words(int64_t ncols, int bshift) {
  return (ncols + (int64_t(1) << bshift) - 1) >> bshift;
}

// ---- the cold pass over dirty blocks (gf_locate_kernel, gf_correct_kernel, gf_checked_fix_kernel) ----
// One workgroup per span of min(block_bytes, 16 KiB) columns, grid.x = span.
struct Span {
  int64_t base, end;  // the workgroup's columns
  bool dirty;         // its mask word is nonzero
};

// Stripe b = blockIdx.y of a batched launch (its own n_in input and n_out output row pointers, mask
// row and nbins counts, every offset formed in 64 bits), then the workgroup's span. n_out = 0: the
// kernel stores no output rows and d.out stays as it is. `dirty` is uniform, so on !dirty the whole
// workgroup can leave, before any barrier.
template <bool BATCH>
__device__ __forceinline__ Span cold_span(DescView& d, int n_in, int n_out, const int*& mask,
                                          unsigned long long*& counts, int nbins, int64_t ncols, int bshift,
                                          int span_shift) {
  if constexpr (BATCH) {
    const uint64_t b = blockIdx.y;
    d.in += b * uint64_t(n_in);
    d.out += b * uint64_t(n_out);
    mask += b * uint64_t(mask_words(ncols, bshift));
    counts += b * uint64_t(nbins);
  }
  const int64_t base = int64_t(blockIdx.x) << span_shift;
  return {base, std::min(base + (int64_t(1) << span_shift), ncols), mask[base >> bshift] != 0};
}

// col(acc, q, c) for every column c of the span: its syndrome bytes are byte q of acc[0..MT-1] under
// the MT-row tables of `d` over n input rows. Four columns per lane, the ragged end of the span a
// byte at a time; `bytewise` (rows of any alignment): one column per lane throughout.
template <int MT, typename F>
__device__ __forceinline__ void sweep_span(const DescView& d, int n, const Span& s, bool bytewise, F&& col) {
  uint32_t acc[MT];
  if (!bytewise) {
    for (int64_t c = s.base + int64_t(threadIdx.x) * 4; c < s.end; c += kBlock * 4) {
      if (c + 4 <= s.end) {
        syn_cols<MT, uint32_t>(d, n, MT, 0, c, acc);
        for (int q = 0; q < 4; ++q) col(acc, q, c + q);
      } else {
        for (int64_t cc = c; cc < s.end; ++cc) {
          syn_cols<MT, uint8_t>(d, n, MT, 0, cc, acc);
          col(acc, 0, cc);
        }
      }
    }
  } else {
    for (int64_t c = s.base + threadIdx.x; c < s.end; c += kBlock) {
      syn_cols<MT, uint8_t>(d, n, MT, 0, c, acc);
      col(acc, 0, c);
    }
  }
}

// The workgroup's LDS histogram into the stripe's 64-bit counts: one atomic add per nonzero bin
__device__ __forceinline__ void flush_bins(const uint32_t* hist, int nbins, unsigned long long* counts) {
  __syncthreads();
  for (int t = threadIdx.x; t < nbins; t += kBlock) {
    const uint32_t v = hist[t];
    if (v) atomicAdd(counts + t, (unsigned long long)v);
  }
}

// ---- locate: the classifier of gf_locate_kernel and gf_varlen_locate_kernel ----
struct LocLds {
  uint8_t exp[1024];         // gf256.h layout: exp[510..1020] = 0
  uint16_t log[256];         // log[0] = 510
  uint16_t hlog[16 * 256];   // log H[i][j] at [i * n + j]
  uint16_t pinvlog[256];     // log of 1 / H[piv[j]][j]
  uint8_t piv[256];          // pivot (first nonzero) row of column j
  uint32_t hist[256 + 2];    // votes[n], unlocated, bad columns
};

// One byte column: s_i = byte q of acc[i]. Votes go to the LDS histogram, the two totals to the
// lane's own counters.
template <int MT>
__device__ __forceinline__ void classify(const LocLds& l, uint32_t* hist, const uint32_t (&acc)[MT], int q, int n,
                                         int p, bool locatable, uint32_t& bad, uint32_t& unl) {
  uint32_t sp[4] = {0u, 0u, 0u, 0u};  // the syndrome bytes, four rows per word
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const uint32_t s = (acc[i] >> (8 * q)) & 0xFFu;
    sp[i >> 2] |= s << (8 * (i & 3));
    nz |= uint32_t(s != 0) << i;
  }
  if (nz == 0) return;
  ++bad;
  if (!locatable) {
    ++unl;
    return;
  }
  const int k = n - p;
  if ((nz & (nz - 1)) == 0) {
    atomicAdd(&hist[k + (__ffs(int(nz)) - 1)], 1u);
    return;
  }
  for (int j = 0; j < k; ++j) {
    const int r = l.piv[j];
    const uint32_t w = r < 8 ? (r < 4 ? sp[0] : sp[1]) : (r < 12 ? sp[2] : sp[3]);
    const uint32_t sr = (w >> (8 * (r & 3))) & 0xFFu;
    if (sr == 0) continue;  // e would be 0
    int le = int(l.log[sr]) + int(l.pinvlog[j]);  // log e, e = s_r / H[r][j]
    if (le >= 255) le -= 255;
    bool match = true;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      if (i < p) {
        const uint32_t s = (sp[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        match = match && uint32_t(l.exp[le + int(l.hlog[i * n + j])]) == s;
      }
    }
    if (match) {
      atomicAdd(&hist[j], 1u);
      return;
    }
  }
  ++unl;
}

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

// ---- launchers ----

// A batch in slices of at most kMaxGridY stripes (grid.y): launch(d, stripes, mask, counts) gets the
// descriptor view, mask row and counts row of its first stripe. The strides are per stripe: input and
// output row pointers, mask words, count words (counts may be null, with a stride of 0). The first
// error ends it.
template <typename Mask, typename F>
hipError_t launch_slices(const DescView& d0, int batch, size_t in_stride, size_t out_stride, Mask* mask,
                         size_t mask_stride, uint64_t* counts, size_t count_stride, F&& launch) {
  hipError_t e = hipSuccess;
  for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridY) {
    DescView d = d0;
    d.in += size_t(b0) * in_stride;
    d.out += size_t(b0) * out_stride;
    e = launch(d, unsigned(std::min(batch - b0, kMaxGridY)), mask + size_t(b0) * mask_stride,
               counts + size_t(b0) * count_stride);
  }
  return e;
}

// One cold launch over `batch` stripes: kernel(mt, grid, span_shift) launches the family's kernel
// for the tile of pad_m(rows) check rows.
template <typename F>
hipError_t cold_launch(int rows, unsigned batch, int64_t ncols, int bshift, F&& kernel) {
  const int span_shift = std::min(bshift, kLocSpanShift);
  const int64_t nwg = (ncols + (int64_t(1) << span_shift) - 1) >> span_shift;
  return dispatch_tile(pad_m(rows), [&](auto mt) -> hipError_t {
    kernel(mt, dim3(unsigned(nwg), batch), span_shift);
    return hipGetLastError();
  });
}

}  // namespace scrubdev
}  // namespace gfrs
