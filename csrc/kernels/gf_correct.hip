// Correct on gfx950: repair up to two wrong chunks per byte column of an n-row stripe, in place.
//
// The cold pass of a scrub (gf_scrub.hip's gf_locate_kernel, on scrub_device.h's scaffold) with a
// decoder in place of the vote. After the syndrome launch, workgroups whose mask word is zero exit at
// once; the others recompute the syndrome s = H . stripe[:, c] of each byte column and, for s != 0,
// apply the rule that correct_device.h states and implements (decode_col). This file holds how a
// repair is applied to a whole stripe, the kernel and its launchers.
// Fixes are ordinary per-lane byte stores into the stripe rows (columns are independent, so no two
// lanes touch one byte); nothing else of the rows is stored. Counts go through an LDS histogram per
// workgroup and one 64-bit atomic add per nonzero bin: fixed_bytes[n], weight-1 columns, weight-2
// columns, uncorrectable columns, bad columns. BATCH: grid.y = stripe, as in gf_scrub.hip.
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

// A repair of chunk j's byte in column `col` of the stripe: stripe[j][col] ^= e, loaded and stored by
// this lane alone, and one more fixed byte in chunk j's bin
struct PlainFix {
  const DescView& d;
  uint32_t* hist;
  int64_t col;
  __device__ __forceinline__ void patch(int j, uint32_t e) const {
    const auto ptr = (gptr<uint8_t>)(d.in[j] + uint64_t(col));
    *ptr = uint8_t(*ptr ^ e);
  }
  __device__ __forceinline__ void count(int j) const { atomicAdd(&hist[j], 1u); }
};

// One byte column `col`: s_i = byte q of acc[i].
template <int MT>
__device__ __forceinline__ Outcome correct_col(const CorLds& l, uint32_t* hist, const DescView& d,
                                            const uint32_t (&acc)[MT], int q, int64_t col, int n, int p,
                                            bool locatable, int max_errors) {
  Pack sp;  // the syndrome bytes
  bool any = false;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const uint32_t s = (acc[i] >> (8 * q)) & 0xFFu;
    pack_byte(sp, i, s);
    any = any || s != 0;
  }
  if (!any) return kClean;
  return decode_col<MT>(l, sp, n, p, locatable, max_errors, PlainFix{d, hist, col});
}

// BATCH: grid.y = stripe; the stripe's own rows, mask row and n + 4 counts.
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_correct_kernel(DescView d, int n, int p, int64_t ncols, int bshift,
                                                            int span_shift, const int* mask, const uint8_t* loc,
                                                            int locatable, int max_errors, int bytewise,
                                                            unsigned long long* counts) {
  const Span span = cold_span<BATCH>(d, n, 0, mask, counts, n + 4, ncols, bshift, span_shift);
  if (!span.dirty) return;
  __shared__ CorLds l;
  fill_cor_lds(l, d_tab, loc, n, p);
  __syncthreads();

  Tally tally;
  sweep_span<MT>(d, n, span, bytewise != 0, [&](const uint32_t (&acc)[MT], int q, int64_t col) {
    tally.add(correct_col<MT>(l, l.hist, d, acc, q, col, n, p, locatable != 0, max_errors));
  });
  tally.flush(l.hist, n);
  flush_bins(l.hist, n + 4, counts);
}

// what the locate launchers refuse, p < 2 (nothing can be corrected), and a pair search the kernel
// does not offer
bool correct_args_ok(int n, int p, int64_t ncols, int64_t block_bytes, int max_errors) {
  if (!locate_args_ok(n, p, ncols, block_bytes) || p < 2) return false;
  return max_errors == 1 || (max_errors == 2 && p >= 4 && n <= kCorrectMaxPairN);
}

// One family for both launchers: the counts cleared, then the batch in slices of grid.y stripes. The
// single launcher is the BATCH = false instantiation on a batch of one.
template <bool BATCH>
hipError_t correct_all(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                       int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                       uint64_t* counts, hipStream_t stream) {
  if (!desc || !correct_args_ok(n, p, ncols, block_bytes, max_errors) || !mask || !loc || !counts)
    return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(counts, 0, size_t(batch) * size_t(n + 4) * sizeof(uint64_t), stream);
  if (e != hipSuccess || ncols == 0) return e;
  const int bshift = log2_exact(block_bytes);
  return launch_slices(
      view(desc, n, pad_m(p), batch), batch, n, 0, mask, mask_words(ncols, bshift), counts, n + 4,
      [&](const DescView& d, unsigned stripes, const int32_t* m, uint64_t* c) {
        return cold_launch(p, stripes, ncols, bshift, [&](auto mt, dim3 grid, int span_shift) {
          gf_correct_kernel<decltype(mt)::value, BATCH><<<grid, kBlock, 0, stream>>>(
              d, n, p, ncols, bshift, span_shift, m, loc, locatable ? 1 : 0, max_errors, force_bytewise ? 1 : 0,
              reinterpret_cast<unsigned long long*>(c));
        });
      });
}

}  // namespace

hipError_t launch_gf_correct(const void* desc, int n, int p, int64_t ncols, bool force_bytewise, int64_t block_bytes,
                             const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                             uint64_t* counts, hipStream_t stream) {
  return correct_all<false>(desc, n, p, 1, ncols, force_bytewise, block_bytes, mask, loc, locatable, max_errors, counts,
                            stream);
}

hipError_t launch_gf_correct_batched(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                                     int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                     int max_errors, uint64_t* counts, hipStream_t stream) {
  if (batch < 1) return hipErrorInvalidValue;
  return correct_all<true>(desc, n, p, batch, ncols, force_bytewise, block_bytes, mask, loc, locatable, max_errors,
                           counts, stream);
}

}  // namespace gfrs
