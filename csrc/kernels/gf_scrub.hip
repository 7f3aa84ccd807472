// Scrub on gfx950: is an n-row stripe consistent, and if not, which chunk is wrong?
//
// With the parity-check matrix H = [E | I_p] (p x n) the syndrome of byte column c is
// s = H . stripe[:, c]: zero exactly when the column is consistent, and a multiple of column j of H
// when only chunk j is wrong there. Two kernels:
//   * gf_syndrome_*: the hot path. The same GF-GEMM as gf_gemm.hip (perm_device.h helpers,
//     non-temporal 16-byte loads, output tiles of up to 16 rows, the XCD tile map) over a descriptor
//     whose inputs are the n stripe rows and whose tables are H's, but no row is ever stored: every
//     lane folds its accumulators to one bit per syndrome row, a wave ORs them with ballots, and lane
//     0 issues one atomicOr into the int32 mask word of its column block, only when a bit is set.
//     A clean stripe reads its n rows and stores nothing (ReedSolomon.verify: k rows read, p
//     written, 2 p read back).
//   * gf_locate_kernel: the cold path. Workgroups whose mask word is zero exit at once; the others
//     recompute the syndrome of each byte column and classify it: one nonzero s_i blames parity
//     chunk k + i; several blame the native j with s == e . H[:, j], e = s_r / H[r][j], r = column
//     j's pivot row; anything else is unlocated. Counts go through an LDS histogram per workgroup
//     and one 64-bit atomic add per nonzero bin.
// Both have a batched form (template flag BATCH, grid.y = stripe) over a desc_layout(n, m_pad, batch)
// descriptor, for scrubbing many small stripes in one launch: stripe b reads its own row pointers and
// writes its own mask and counts rows; the tables of H are shared. The single-stripe launchers run
// the BATCH = false instantiations, which the flag leaves exactly as they were. The cold pass's
// scaffold (stripe offsets, span and early exit, column sweep, count flush) and the launchers' slicing
// of a batch past the grid.y limit are scrub_device.h's, shared with gf_correct.hip and gf_checked.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "gfrs/desc.h"
#include "gfrs/kernels.h"
#include "gfrs/perm_device.h"
#include "gfrs/scrub_device.h"
#include "gfrs/tune.h"

namespace gfrs {
namespace {

using namespace permdev;
using namespace scrubdev;

__constant__ Tables d_tab = make_tables();

// (syn_byte_bits, group_bits, wave_or and wave_block: scrub_device.h)

// Stripe b = blockIdx.y of a batched launch (gf_gemm.hip's stripe()): its own n row pointers and its
// own row of ceil(ncols / block_bytes) mask words, both offsets formed in 64 bits. A wave never spans
// two stripes, so everything wave_or and wave_block assume holds within each.
template <bool BATCH>
__device__ __forceinline__ void stripe(DescView& d, int n, int*& mask, int64_t ncols, int bshift) {
  if constexpr (BATCH) {
    const uint64_t b = blockIdx.y;
    d.in += b * uint64_t(n);
    mask += b * uint64_t((ncols + (int64_t(1) << bshift) - 1) >> bshift);
  }
}

// General form: any n, two rows in flight, grid-stride over column blocks (gf_gemm_vec_kernel with
// V = 1, PF = 2, non-temporal loads, no copies and no stores).
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_syndrome_vec_kernel(DescView d, int n, int m_pad, int ntiles,
                                                                 int64_t ngroups, int64_t nblk, int64_t ncb, int tail,
                                                                 int* mask, int bshift) {
  stripe<BATCH>(d, n, mask, ngroups * 16 + tail, bshift);
  const TileMap tm = map_block(ntiles);
  if (tm.cb0 >= ncb) return;
  const int i0 = tm.tile * MT;
  constexpr bool kPairs = MT <= 8;  // as gf_gemm_vec_kernel: the 16-row tile has no registers for pairs
  for (int64_t cb = tm.cb0; cb < nblk; cb += ncb) {
    const int64_t g = cb * kBlock + threadIdx.x;
    uint32_t rowbits = 0;
    if (g < ngroups) {
      const int64_t off = g * 16;
      uint32_t acc[MT][4];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[i][w] = 0;
      u32x4 r0 = ld16<true>(row_vec(d.in[0], off));
      u32x4 r1 = n > 1 ? ld16<true>(row_vec(d.in[1], off)) : u32x4{0u, 0u, 0u, 0u};
      for (int j = 0; j < n; j += 2) {
        const u32x4 x0 = r0, x1 = r1;
        if (j + 2 < n) r0 = ld16<true>(row_vec(d.in[j + 2], off));
        if (j + 3 < n) r1 = ld16<true>(row_vec(d.in[j + 3], off));
        const auto t0 = d.tab + (size_t(j) * m_pad + i0) * kPermStride;
        const auto t1 = t0 + size_t(m_pad) * kPermStride;
        if (kPairs && j + 1 < n) {
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const Sel s0 = make_sel(x0[w]);
            const Sel s1 = make_sel(x1[w]);
#pragma unroll
            for (int i = 0; i < MT; ++i)
              acc[i][w] = mac_pair(acc[i][w], t0 + i * kPermStride, s0, t1 + i * kPermStride, s1);
          }
        } else {
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const Sel s0 = make_sel(x0[w]);
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i][w] = mac_map(acc[i][w], t0 + i * kPermStride, s0);
          }
          if (j + 1 < n) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const Sel s1 = make_sel(x1[w]);
#pragma unroll
              for (int i = 0; i < MT; ++i) acc[i][w] = mac_map(acc[i][w], t1 + i * kPermStride, s1);
            }
          }
        }
      }
      rowbits = group_bits<MT>(acc);
    } else if (g - ngroups < tail) {
      rowbits = syn_byte_bits<MT>(d, n, m_pad, i0, ngroups * 16 + (g - ngroups));
    }
    wave_or<MT>(rowbits, i0 & 16, mask, wave_block(cb * kBlock + (threadIdx.x & ~63u), ngroups, bshift));
  }
}

// Rows-in-flight form (narrow codes, compile-time N, one tile): every lane issues the loads of all N
// rows of its group before the first multiply. It is gf_gemm_rows_lat_kernel without copies and
// stores: the table pointer is re-issued by an empty asm after each row pair's math, so each pair's
// scalar table loads wait only for the previous pair and nothing spills; one group per lane, no
// grid-stride loop (around a loop the loop-invariant table words would be hoisted and spilled).
// IDENT: the last MT columns of H are the identity (H = [E | I_p], p = MT), so parity row i is
// XORed into syndrome row i as it is instead of going through the tables of 0 and 1: the multiplies
// of an encode (k x p) are left, not n x p.
template <int MT, int N, bool IDENT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_syndrome_rows_kernel(DescView d, int n_tail, int m_pad, int ntiles,
                                                                  int64_t ngroups, int tail, int* mask, int bshift) {
  constexpr int K = IDENT ? N - MT : N;  // rows that are multiplied
  stripe<BATCH>(d, N, mask, ngroups * 16 + tail, bshift);
  const TileMap tm = map_block(ntiles);
  const int i0 = sgpr_int(tm.tile * MT);
  const int64_t g = tm.cb0 * kBlock + threadIdx.x;
  uint32_t rowbits = 0;
  if (g < ngroups) {
    const int64_t off = g * 16;
    u32x4 x[N];
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = ld16<true>(row_vec(d.in[j], off));
    uint32_t acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) acc[i][w] = 0;
    uint64_t tb = (uint64_t)d.tab;
#pragma unroll
    for (int j = 0; j < K; j += 2) {
      if (j > 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int w = 0; w < 4; ++w) asm volatile("" ::"v"(acc[i][w]));
      }
      asm volatile("" : "+s"(tb));
      asm volatile("" : "+v"(x[j]));
      if (j + 1 < K) asm volatile("" : "+v"(x[j + 1]));
      const auto t0 = (cptr<uint32_t>)tb + (size_t(j) * m_pad + i0) * kPermStride;
      if (j + 1 < K) {
        const auto t1 = t0 + size_t(m_pad) * kPermStride;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const Sel s0 = make_sel(x[j][w]);
          const Sel s1 = make_sel(x[j + 1][w]);
#pragma unroll
          for (int i = 0; i < MT; ++i)
            acc[i][w] = mac_pair(acc[i][w], t0 + i * kPermStride, s0, t1 + i * kPermStride, s1);
        }
      } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const Sel s = make_sel(x[j][w]);
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[i][w] = mac_map(acc[i][w], t0 + i * kPermStride, s);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (IDENT) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[i][w] ^= x[K + i][w];
    }
    rowbits = group_bits<MT>(acc);
  } else if (g - ngroups < tail) {
    // (n_tail == N, passed at run time: a compile-time N would unroll the tail's row loop too)
    rowbits = syn_byte_bits<MT>(d, n_tail, m_pad, i0, ngroups * 16 + (g - ngroups));
  }
  wave_or<MT>(rowbits, i0 & 16, mask, wave_block(tm.cb0 * kBlock + (threadIdx.x & ~63u), ngroups, bshift));
}

// Byte form: one lane per byte column, rows of any alignment. A wave's 64 columns share a mask word
// (block_bytes is a multiple of 64).
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_syndrome_byte_kernel(DescView d, int n, int m_pad, int ntiles,
                                                                  int64_t ncols, int64_t nblk, int64_t ncb, int* mask,
                                                                  int bshift) {
  stripe<BATCH>(d, n, mask, ncols, bshift);
  const TileMap tm = map_block(ntiles);
  if (tm.cb0 >= ncb) return;
  const int i0 = tm.tile * MT;
  for (int64_t cb = tm.cb0; cb < nblk; cb += ncb) {
    const int64_t c = cb * kBlock + threadIdx.x;
    const uint32_t rowbits = c < ncols ? syn_byte_bits<MT>(d, n, m_pad, i0, c) : 0u;
    const int64_t c0 = cb * kBlock + (threadIdx.x & ~63u);
    wave_or<MT>(rowbits, i0 & 16, mask, (c0 < ncols ? c0 : 0) >> bshift);
  }
}

// ---- locate -----------------------------------------------------------------------------------
// (LocLds and classify: scrub_device.h, shared with gf_varlen_scrub.hip)

// BATCH: grid.y = stripe; the stripe's own rows, mask row and n + 2 counts (histogram and totals
// are per stripe).
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_locate_kernel(DescView d, int n, int p, int64_t ncols, int bshift,
                                                           int span_shift, const int* mask, const uint8_t* loc,
                                                           int locatable, int bytewise, unsigned long long* counts) {
  const Span span = cold_span<BATCH>(d, n, 0, mask, counts, n + 2, ncols, bshift, span_shift);
  if (!span.dirty) return;
  __shared__ LocLds l;
  for (int t = threadIdx.x; t < 1024; t += kBlock) l.exp[t] = t < kExpLen ? d_tab.exp[t] : uint8_t(0);
  for (int t = threadIdx.x; t < 256; t += kBlock) l.log[t] = d_tab.log[t];
  for (int t = threadIdx.x; t < p * n; t += kBlock) l.hlog[t] = d_tab.log[loc[t]];
  for (int t = threadIdx.x; t < n; t += kBlock) {
    l.piv[t] = loc[p * n + t];
    l.pinvlog[t] = d_tab.log[loc[p * n + n + t]];
  }
  for (int t = threadIdx.x; t < n + 2; t += kBlock) l.hist[t] = 0;
  __syncthreads();

  uint32_t bad = 0, unl = 0;
  sweep_span<MT>(d, n, span, bytewise != 0, [&](const uint32_t (&acc)[MT], int q, int64_t) {
    classify<MT>(l, l.hist, acc, q, n, p, locatable != 0, bad, unl);
  });
  if (unl) atomicAdd(&l.hist[n], unl);
  if (bad) atomicAdd(&l.hist[n + 1], bad);
  flush_bins(l.hist, n + 2, counts);
}

// ---- launch -----------------------------------------------------------------------------------
// (Grid and make_grid: scrub_device.h)
//
// The rows-in-flight form is built for the (4, 6) and (10, 14) codes, one tile each; `ident` = the
// trailing identity columns of H, and with ident == MT the parity rows skip the multiplies.
// GFRS_TUNE=scrub_rows=0 keeps every launch on the general form, scrub_ident=0 multiplies the
// identity columns too (A/B measurements, profiles/scrub).
// In all of these BATCH picks the batched instantiation and `batch` is grid.y (1 when !BATCH).
template <int MT, int N, bool BATCH>
void launch_rows_n(const DescView& d, int m_pad, int ident, const Grid& g, unsigned batch, int64_t ngroups, int tail,
                   int* mask, int bshift, hipStream_t stream) {
  const dim3 grid(g.blocks, batch);
  if (ident == MT && tune_int("scrub_ident", 1) != 0)
    gf_syndrome_rows_kernel<MT, N, true, BATCH><<<grid, kBlock, 0, stream>>>(d, N, m_pad, 1, ngroups, tail, mask, bshift);
  else
    gf_syndrome_rows_kernel<MT, N, false, BATCH><<<grid, kBlock, 0, stream>>>(d, N, m_pad, 1, ngroups, tail, mask, bshift);
}

template <int MT, bool BATCH>
bool launch_rows(const DescView& d, int n, int m_pad, int ident, const Grid& g, unsigned batch, int64_t ngroups,
                 int tail, int* mask, int bshift, hipStream_t stream) {
  if (m_pad != MT || g.ncb < g.nblk || tune_int("scrub_rows", 1) == 0) return false;
  if constexpr (MT == 2) {
    if (n == 6) {
      launch_rows_n<2, 6, BATCH>(d, m_pad, ident, g, batch, ngroups, tail, mask, bshift, stream);
      return true;
    }
  }
  if constexpr (MT == 4) {
    if (n == 14) {
      launch_rows_n<4, 14, BATCH>(d, m_pad, ident, g, batch, ngroups, tail, mask, bshift, stream);
      return true;
    }
  }
  return false;
}

// One family for each pair of launchers (the single one is the BATCH = false instantiation on a
// batch of one): the mask or the counts cleared, then the batch in slices of grid.y stripes.
template <bool BATCH>
hipError_t syndrome_all(const void* desc, int n, int m_pad, int ident, int batch, int64_t ncols, bool force_bytewise,
                        int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  if (!scrub_args_ok(n, m_pad, ncols, block_bytes) || !mask || ident < 0 || ident > m_pad || ident >= n)
    return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const int bshift = log2_exact(block_bytes);
  const int64_t nmask = mask_words(ncols, bshift);
  const hipError_t e = hipMemsetAsync(mask, 0, size_t(batch) * size_t(nmask) * sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
  return launch_slices(
      view(desc, n, m_pad, batch), batch, n, 0, mask, nmask, nullptr, 0,
      [&](const DescView& d, unsigned stripes, int32_t* m, uint64_t*) {
        return dispatch_tile(tile_for(m_pad), [&](auto mt) -> hipError_t {
          constexpr int MT = decltype(mt)::value;
          const int ntiles = m_pad / MT;
          if (force_bytewise) {
            const Grid g = make_grid(ncols, ntiles);
            gf_syndrome_byte_kernel<MT, BATCH>
                <<<dim3(g.blocks, stripes), kBlock, 0, stream>>>(d, n, m_pad, ntiles, ncols, g.nblk, g.ncb, m, bshift);
            return hipGetLastError();
          }
          const int64_t ngroups = ncols / 16;
          const int tail = int(ncols % 16);
          const Grid g = make_grid(ngroups + tail, ntiles);  // one extra lane per ragged tail byte
          if (!launch_rows<MT, BATCH>(d, n, m_pad, ident, g, stripes, ngroups, tail, m, bshift, stream))
            gf_syndrome_vec_kernel<MT, BATCH><<<dim3(g.blocks, stripes), kBlock, 0, stream>>>(
                d, n, m_pad, ntiles, ngroups, g.nblk, g.ncb, tail, m, bshift);
          return hipGetLastError();
        });
      });
}

template <bool BATCH>
hipError_t locate_all(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                      int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable, uint64_t* counts,
                      hipStream_t stream) {
  if (!locate_args_ok(n, p, ncols, block_bytes) || !mask || !loc || !counts) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(counts, 0, size_t(batch) * size_t(n + 2) * sizeof(uint64_t), stream);
  if (e != hipSuccess || ncols == 0) return e;
  const int bshift = log2_exact(block_bytes);
  return launch_slices(
      view(desc, n, pad_m(p), batch), batch, n, 0, mask, mask_words(ncols, bshift), counts, n + 2,
      [&](const DescView& d, unsigned stripes, const int32_t* m, uint64_t* c) {
        return cold_launch(p, stripes, ncols, bshift, [&](auto mt, dim3 grid, int span_shift) {
          gf_locate_kernel<decltype(mt)::value, BATCH><<<grid, kBlock, 0, stream>>>(
              d, n, p, ncols, bshift, span_shift, m, loc, locatable ? 1 : 0, force_bytewise ? 1 : 0,
              reinterpret_cast<unsigned long long*>(c));
        });
      });
}

}  // namespace

hipError_t launch_gf_syndrome(const void* desc, int n, int m_pad, int ident, int64_t ncols, bool force_bytewise,
                              int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  return syndrome_all<false>(desc, n, m_pad, ident, 1, ncols, force_bytewise, block_bytes, mask, stream);
}

hipError_t launch_gf_syndrome_batched(const void* desc, int n, int m_pad, int ident, int batch, int64_t ncols,
                                      bool force_bytewise, int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  if (batch < 1 || !desc) return hipErrorInvalidValue;
  return syndrome_all<true>(desc, n, m_pad, ident, batch, ncols, force_bytewise, block_bytes, mask, stream);
}

hipError_t launch_gf_locate(const void* desc, int n, int p, int64_t ncols, bool force_bytewise, int64_t block_bytes,
                            const int32_t* mask, const uint8_t* loc, bool locatable, uint64_t* counts,
                            hipStream_t stream) {
  return locate_all<false>(desc, n, p, 1, ncols, force_bytewise, block_bytes, mask, loc, locatable, counts, stream);
}

hipError_t launch_gf_locate_batched(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                                    int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                    uint64_t* counts, hipStream_t stream) {
  if (batch < 1 || !desc) return hipErrorInvalidValue;
  return locate_all<true>(desc, n, p, batch, ncols, force_bytewise, block_bytes, mask, loc, locatable, counts, stream);
}

}  // namespace gfrs
