// Checked repair on gfx950: rebuild the erased rows of a degraded stripe and, in the same pass, check
// the survivors with the parity the erasures leave over; then correct what the check found.
//
// With e rows erased (X), the n - e survivors S ascending, K the first k of S and R the last
// r = p - e, T = inv(H[:, X + R]) . H has T[:, X + R] = I_p: rows 0..e-1 rebuild X from K (they are
// zero on R), rows e..p-1 re-encode survivor R[i] from K and XOR it in (they are zero on X): the
// [E | I] shape of gf_scrub.hip's IDENT path. The descriptor is desc_layout(ns, pad_m(p)) with the
// ns = n - e survivors as inputs (K, then R), the erased rows as outputs 0..e-1 (0 = not stored) and
// the tables of T[:, S]. The erased rows are never read. Two kernels:
//   * gf_checked_*: the hot pass, gf_syndrome_vec_kernel with stores. One tile of pad_m(p)
//     accumulators per 16-byte group, two rows in flight, non-temporal loads; the K rows go through
//     the tables, the R rows are XORed into their check accumulators as they are. Accumulators
//     0..e-1 are stored to the erased rows (16-byte non-temporal stores), accumulators e..p-1 are
//     folded to row bits and ORed into the mask word of the column block, never stored: a
//     consistent stripe moves n - e rows in and e rows out and nothing else.
//   * gf_checked_fix_kernel: the cold pass, gf_correct_kernel on the survivors. Workgroups whose
//     mask word is zero exit before any barrier; the others recompute each byte column and run
//     the decoder of gf_correct.hip (correct_device.h's decode_col, which states the rule) with the
//     r x ns check matrix T[e:, S]. A corrected survivor byte j gets ^= v, and every erased row i
//     then ^= v . T[i][j], so it holds the value rebuilt from the corrected survivors. An
//     uncorrectable column keeps its survivors and the hot pass's rebuild. Counts as
//     gf_correct.hip: fixed_bytes[ns] by survivor index, weight-1, weight-2, uncorrectable and bad
//     columns.
// BATCH: grid.y = stripe, one erasure pattern (one T) for the whole batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gfrs/correct_device.h"
#include "gfrs/desc.h"
#include "gfrs/gf256.h"
#include "gfrs/kernels.h"
#include "gfrs/perm_device.h"
#include "gfrs/scrub_device.h"

namespace gfrs {
namespace {

using namespace permdev;
using namespace scrubdev;

__constant__ Tables d_tab = make_tables();

// Stripe b = blockIdx.y of a batched launch: its own survivor and erased row pointers and mask row
template <int MT, bool BATCH>
__device__ __forceinline__ void stripe(DescView& d, int ns, int*& mask, int64_t ncols, int bshift) {
  if constexpr (BATCH) {
    const uint64_t b = blockIdx.y;
    d.in += b * uint64_t(ns);
    d.out += b * uint64_t(MT);
    mask += b * uint64_t((ncols + (int64_t(1) << bshift) - 1) >> bshift);
  }
}

// acc[ci] ^= x with ci wave-uniform: one v_bitop3 (a ^ (b & m)) per word under a scalar mask, so no
// accumulator is indexed at run time
template <int MT>
__device__ __forceinline__ void xor_row(uint32_t (&acc)[MT][4], const u32x4& x, int ci) {
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const uint32_t m = i == ci ? ~0u : 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) acc[i][w] = __builtin_amdgcn_bitop3_b32(acc[i][w], x[w], m, 0x78);
  }
}

// the check rows e..e+r-1 of a lane's row bits, as mask bits 0..r-1
__device__ __forceinline__ uint32_t check_bits(uint32_t bits, int e, int r) { return (bits >> e) & ((1u << r) - 1u); }

// One byte column, any alignment: every row through the tables (the R columns hold 0 and 1), the
// rebuilt bytes stored, the check bits returned
template <int MT>
__device__ __forceinline__ uint32_t checked_byte(const DescView& d, int ns, int e, int r, int64_t off) {
  uint32_t acc[MT];
  syn_cols<MT, uint8_t>(d, ns, MT, 0, off, acc);
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const uint64_t o = d.out[i];
    if (o) *(gptr<uint8_t>)(o + uint64_t(off)) = uint8_t(acc[i]);
    bits |= uint32_t((acc[i] & 0xFFu) != 0) << i;
  }
  return check_bits(bits, e, r);
}

// 16-byte groups, grid-stride over column blocks; the ragged tail bytes on extra lanes
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_checked_vec_kernel(DescView d, int ns, int e, int r, int64_t ngroups,
                                                                int64_t nblk, int64_t ncb, int tail, int* mask,
                                                                int bshift) {
  stripe<MT, BATCH>(d, ns, mask, ngroups * 16 + tail, bshift);
  const TileMap tm = map_block(1);
  if (tm.cb0 >= ncb) return;
  const int k = ns - r;
  constexpr bool kPairs = MT <= 8;  // as gf_syndrome_vec_kernel
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
      u32x4 r1 = ns > 1 ? ld16<true>(row_vec(d.in[1], off)) : u32x4{0u, 0u, 0u, 0u};
      for (int j = 0; j < ns; j += 2) {
        const u32x4 x0 = r0, x1 = r1;
        if (j + 2 < ns) r0 = ld16<true>(row_vec(d.in[j + 2], off));
        if (j + 3 < ns) r1 = ld16<true>(row_vec(d.in[j + 3], off));
        const auto t0 = d.tab + size_t(j) * MT * kPermStride;
        if (j + 1 < k) {  // two K rows
          const auto t1 = t0 + size_t(MT) * kPermStride;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const Sel s0 = make_sel(x0[w]);
            const Sel s1 = make_sel(x1[w]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
              if constexpr (kPairs)
                acc[i][w] = mac_pair(acc[i][w], t0 + i * kPermStride, s0, t1 + i * kPermStride, s1);
              else
                acc[i][w] = mac_map(mac_map(acc[i][w], t0 + i * kPermStride, s0), t1 + i * kPermStride, s1);
            }
          }
        } else {  // the last K row and an R row, or R rows: survivor j >= k is check row e + j - k
          if (j < k) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const Sel s0 = make_sel(x0[w]);
#pragma unroll
              for (int i = 0; i < MT; ++i) acc[i][w] = mac_map(acc[i][w], t0 + i * kPermStride, s0);
            }
          } else {
            xor_row<MT>(acc, x0, e + j - k);
          }
          if (j + 1 < ns) xor_row<MT>(acc, x1, e + j + 1 - k);
        }
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const uint64_t o = d.out[i];
        if (o) st16<true>(row_vec_w(o, off), u32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]});
      }
      rowbits = check_bits(group_bits<MT>(acc), e, r);
    } else if (g - ngroups < tail) {
      rowbits = checked_byte<MT>(d, ns, e, r, ngroups * 16 + (g - ngroups));
    }
    wave_or<MT>(rowbits, 0, mask, wave_block(cb * kBlock + (threadIdx.x & ~63u), ngroups, bshift));
  }
}

// Byte form: one lane per byte column, rows of any alignment
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_checked_byte_kernel(DescView d, int ns, int e, int r, int64_t ncols,
                                                                 int64_t nblk, int64_t ncb, int* mask, int bshift) {
  stripe<MT, BATCH>(d, ns, mask, ncols, bshift);
  const TileMap tm = map_block(1);
  if (tm.cb0 >= ncb) return;
  for (int64_t cb = tm.cb0; cb < nblk; cb += ncb) {
    const int64_t c = cb * kBlock + threadIdx.x;
    const uint32_t rowbits = c < ncols ? checked_byte<MT>(d, ns, e, r, c) : 0u;
    const int64_t c0 = cb * kBlock + (threadIdx.x & ~63u);
    wave_or<MT>(rowbits, 0, mask, (c0 < ncols ? c0 : 0) >> bshift);
  }
}

// ---- the cold pass ----------------------------------------------------------------------------
// A repair of survivor j's byte, carried into the erased rows: reb = T[:e, S] row-major (e x ns)
struct DegradedFix {
  const DescView& d;
  const CorLds& l;
  uint32_t* hist;
  const uint8_t* reb;
  int ns, e;
  int64_t col;
  __device__ __forceinline__ void patch(int j, uint32_t v) const {
    const auto ptr = (gptr<uint8_t>)(d.in[j] + uint64_t(col));
    *ptr = uint8_t(*ptr ^ v);
    for (int i = 0; i < e; ++i) {
      const uint32_t a = reb[i * ns + j];
      if (a == 0) continue;  // (an R survivor: the rebuild does not read it)
      const auto out = (gptr<uint8_t>)(d.out[i] + uint64_t(col));
      *out = uint8_t(*out ^ l.exp[int(l.log[v]) + int(l.log[a])]);  // v != 0: both logs below 255
    }
  }
  __device__ __forceinline__ void count(int j) const { atomicAdd(&hist[j], 1u); }
};

// One byte column `col`: the check syndrome u_t = byte q of acc[e + t]
template <int MT>
__device__ __forceinline__ Outcome fix_col(const CorLds& l, uint32_t* hist, const DescView& d, const uint8_t* reb,
                                        const uint32_t (&acc)[MT], int q, int64_t col, int ns, int e, int r,
                                        bool locatable, int max_errors) {
  Pack sp;
  bool any = false;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const uint32_t s = (acc[i] >> (8 * q)) & 0xFFu;
    if (i >= e && i < e + r) {
      pack_byte(sp, i - e, s);
      any = any || s != 0;
    }
  }
  if (!any) return kClean;
  return decode_col<MT>(l, sp, ns, r, locatable, max_errors, DegradedFix{d, l, hist, reb, ns, e, col});
}

template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_checked_fix_kernel(DescView d, int ns, int e, int r, int64_t ncols,
                                                                int bshift, int span_shift, const int* mask,
                                                                const uint8_t* loc, int locatable, int max_errors,
                                                                int bytewise, unsigned long long* counts) {
  const Span span = cold_span<BATCH>(d, ns, MT, mask, counts, ns + 4, ncols, bshift, span_shift);
  if (!span.dirty) return;
  __shared__ CorLds l;
  fill_cor_lds(l, d_tab, loc, ns, r);
  __syncthreads();

  const uint8_t* reb = loc + r * ns + 2 * ns;
  const bool loc_ok = locatable != 0;
  Tally tally;
  sweep_span<MT>(d, ns, span, bytewise != 0, [&](const uint32_t (&acc)[MT], int q, int64_t col) {
    tally.add(fix_col<MT>(l, l.hist, d, reb, acc, q, col, ns, e, r, loc_ok, max_errors));
  });
  tally.flush(l.hist, ns);
  flush_bins(l.hist, ns + 4, counts);
}

// ---- launch -----------------------------------------------------------------------------------
// ns survivors of which the last r are check rows (k = ns - r >= 1 of them rebuild), e erased rows,
// 1 <= e + r <= 16, and what the scrub launchers ask of the columns and the block
bool checked_args_ok(int ns, int e, int r, int64_t ncols, int64_t block_bytes) {
  if (e < 0 || r < 0 || e + r < 1 || e + r > 16 || ns > 256 || r >= ns) return false;
  if (!scrub_args_ok(ns, pad_m(e + r), ncols, block_bytes)) return false;
  const int span_shift = std::min(log2_exact(block_bytes), kLocSpanShift);
  return ((ncols + (int64_t(1) << span_shift) - 1) >> span_shift) <= int64_t(INT32_MAX);
}

bool fix_args_ok(int ns, int e, int r, int64_t ncols, int64_t block_bytes, int max_errors) {
  if (!checked_args_ok(ns, e, r, ncols, block_bytes) || r < 1) return false;
  return max_errors == 1 || (max_errors == 2 && r >= 4 && ns <= kCorrectMaxPairN);
}

// One family for each pair of launchers (the single one is the BATCH = false instantiation on a
// batch of one): the mask or the counts cleared, then the batch in slices of grid.y stripes.
template <bool BATCH>
hipError_t checked_all(const void* desc, int ns, int e, int r, int batch, int64_t ncols, bool force_bytewise,
                       int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  if (!desc || !checked_args_ok(ns, e, r, ncols, block_bytes) || !mask) return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const int bshift = log2_exact(block_bytes);
  const int64_t nmask = mask_words(ncols, bshift);
  const int mt = pad_m(e + r);
  const hipError_t err = hipMemsetAsync(mask, 0, size_t(batch) * size_t(nmask) * sizeof(int32_t), stream);
  if (err != hipSuccess) return err;
  return launch_slices(
      view(desc, ns, mt, batch), batch, ns, mt, mask, nmask, nullptr, 0,
      [&](const DescView& d, unsigned stripes, int32_t* m, uint64_t*) {
        return dispatch_tile(mt, [&](auto tile) -> hipError_t {
          constexpr int MT = decltype(tile)::value;
          if (force_bytewise) {
            const Grid g = make_grid(ncols, 1);
            gf_checked_byte_kernel<MT, BATCH>
                <<<dim3(g.blocks, stripes), kBlock, 0, stream>>>(d, ns, e, r, ncols, g.nblk, g.ncb, m, bshift);
            return hipGetLastError();
          }
          const int64_t ngroups = ncols / 16;
          const int tail = int(ncols % 16);
          const Grid g = make_grid(ngroups + tail, 1);  // one extra lane per ragged tail byte
          gf_checked_vec_kernel<MT, BATCH>
              <<<dim3(g.blocks, stripes), kBlock, 0, stream>>>(d, ns, e, r, ngroups, g.nblk, g.ncb, tail, m, bshift);
          return hipGetLastError();
        });
      });
}

template <bool BATCH>
hipError_t fix_all(const void* desc, int ns, int e, int r, int batch, int64_t ncols, bool force_bytewise,
                   int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                   uint64_t* counts, hipStream_t stream) {
  if (!desc || !fix_args_ok(ns, e, r, ncols, block_bytes, max_errors) || !mask || !loc || !counts)
    return hipErrorInvalidValue;
  const hipError_t err = hipMemsetAsync(counts, 0, size_t(batch) * size_t(ns + 4) * sizeof(uint64_t), stream);
  if (err != hipSuccess || ncols == 0) return err;
  const int bshift = log2_exact(block_bytes);
  return launch_slices(
      view(desc, ns, pad_m(e + r), batch), batch, ns, pad_m(e + r), mask, mask_words(ncols, bshift), counts,
      ns + 4, [&](const DescView& d, unsigned stripes, const int32_t* m, uint64_t* c) {
        return cold_launch(e + r, stripes, ncols, bshift, [&](auto mt, dim3 grid, int span_shift) {
          gf_checked_fix_kernel<decltype(mt)::value, BATCH><<<grid, kBlock, 0, stream>>>(
              d, ns, e, r, ncols, bshift, span_shift, m, loc, locatable ? 1 : 0, max_errors, force_bytewise ? 1 : 0,
              reinterpret_cast<unsigned long long*>(c));
        });
      });
}

}  // namespace

hipError_t launch_gf_checked(const void* desc, int ns, int e, int r, int64_t ncols, bool force_bytewise,
                             int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  return checked_all<false>(desc, ns, e, r, 1, ncols, force_bytewise, block_bytes, mask, stream);
}

hipError_t launch_gf_checked_batched(const void* desc, int ns, int e, int r, int batch, int64_t ncols,
                                     bool force_bytewise, int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  if (batch < 1) return hipErrorInvalidValue;
  return checked_all<true>(desc, ns, e, r, batch, ncols, force_bytewise, block_bytes, mask, stream);
}

hipError_t launch_gf_checked_fix(const void* desc, int ns, int e, int r, int64_t ncols, bool force_bytewise,
                                 int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                 int max_errors, uint64_t* counts, hipStream_t stream) {
  return fix_all<false>(desc, ns, e, r, 1, ncols, force_bytewise, block_bytes, mask, loc, locatable, max_errors, counts,
                        stream);
}

hipError_t launch_gf_checked_fix_batched(const void* desc, int ns, int e, int r, int batch, int64_t ncols,
                                         bool force_bytewise, int64_t block_bytes, const int32_t* mask,
                                         const uint8_t* loc, bool locatable, int max_errors, uint64_t* counts,
                                         hipStream_t stream) {
  if (batch < 1) return hipErrorInvalidValue;
  return fix_all<true>(desc, ns, e, r, batch, ncols, force_bytewise, block_bytes, mask, loc, locatable, max_errors,
                       counts, stream);
}

}  // namespace gfrs
