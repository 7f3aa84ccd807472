// Correct on gfx950: repair up to two wrong chunks per byte column of an n-row stripe, in place.
//
// The cold pass of a scrub (gf_scrub.hip's gf_locate_kernel) with a decoder in place of the vote.
// After the syndrome launch, workgroups whose mask word is zero exit at once; the others recompute
// the syndrome s = H . stripe[:, c] of each byte column and, for s != 0, apply the rule:
//   1. !locatable (p < 2, or two columns of H dependent): uncorrectable.
//   2. weight 1: s == e . H[:, j] for a chunk j (parity chunks included), e = s_r / H[r][j] with r
//      column j's pivot row: stripe[j][c] ^= e. Pairwise independence makes (j, e) unique.
//   3. else, with max_errors == 2: every pair j1 < j2 is tried. Column j1 is projected out,
//      P(v) = v ^ (v_r / H[r][j1]) . H[:, j1] (P(H[:, j1]) = 0, row r of every image is 0), so
//      s = e1 . H[:, j1] ^ e2 . H[:, j2] exactly when P(s) = e2 . P(H[:, j2]) with e2 != 0, and then
//      e1 = (s_r ^ e2 . H[r][j2]) / H[r][j1], which must be nonzero. P(H[:, j2]) is formed on the
//      fly from the log tables in LDS, so nothing grows with n^2. The explanations are COUNTED over
//      all pairs (the search stops at the second): exactly one is applied, none or several leave the
//      column uncorrectable. A non-MDS H (the reference Vandermonde) has dependent 4-sets of
//      columns, on which a double error has a second explanation.
//   4. an uncorrectable column is not written.
// Fixes are ordinary per-lane byte stores into the stripe rows (columns are independent, so no two
// lanes touch one byte); nothing else of the rows is stored. Counts go through an LDS histogram per
// workgroup and one 64-bit atomic add per nonzero bin: fixed_bytes[n], weight-1 columns, weight-2
// columns, uncorrectable columns, bad columns. BATCH: grid.y = stripe, as in gf_scrub.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

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

constexpr int kLogZero = 510;  // log[0]: an index with it in the sum lands in exp's zero band

struct CorLds {
  uint8_t exp[1024];         // gf256.h layout: exp[510..1023] = 0
  uint16_t log[256];         // log[0] = 510
  uint16_t hlog[16 * 256];   // log H[i][j] at [i * n + j]
  uint8_t h[16 * 256];       // H[i][j] at [i * n + j]
  uint16_t pinvlog[256];     // log of 1 / H[piv[j]][j]
  uint8_t piv[256];          // pivot (first nonzero) row of column j
  uint32_t hist[256 + 4];    // fixed_bytes[n], weight-1, weight-2, uncorrectable, bad columns
};

// Up to 16 syndrome bytes, eight rows per 64-bit word: a byte is one select and one shift away, with
// no private array to index (a select chain over four words was turned into one, in scratch)
struct Pack {
  uint64_t lo = 0, hi = 0;
};

__device__ __forceinline__ uint32_t packed_byte(const Pack& s, int i) {
  return uint32_t((i < 8 ? s.lo : s.hi) >> (8 * (i & 7))) & 0xFFu;
}

__device__ __forceinline__ void pack_byte(Pack& s, int i, uint32_t v) {
  const uint64_t x = uint64_t(v) << (8 * (i & 7));
  s.lo |= i < 8 ? x : uint64_t(0);
  s.hi |= i < 8 ? uint64_t(0) : x;
}

__device__ __forceinline__ int mod255(int v) { return v >= 255 ? v - 255 : v; }  // v in [0, 510)

// stripe[j][col] ^= e: one byte of row j, loaded and stored by this lane alone
__device__ __forceinline__ void patch(const DescView& d, int j, int64_t col, uint32_t e) {
  const auto ptr = (gptr<uint8_t>)(d.in[j] + uint64_t(col));
  *ptr = uint8_t(*ptr ^ e);
}

// What became of a byte column
enum Outcome : uint32_t { kClean = 0, kWeight1 = 1, kWeight2 = 2, kUncorrectable = 3 };

// A lane's column totals, as one packed add per column (an increment per outcome in a branch of its
// own is sunk into one store at a computed field, which sends the counters to scratch)
struct Tally {
  uint32_t w1 = 0, w2 = 0, unc = 0, bad = 0;
  __device__ __forceinline__ void add(Outcome o) {
    w1 += uint32_t(o == kWeight1);
    w2 += uint32_t(o == kWeight2);
    unc += uint32_t(o == kUncorrectable);
    bad += uint32_t(o != kClean);
  }
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
  if (!locatable) return kUncorrectable;
  // weight 1: every chunk, natives and parity alike (H need not end in an identity)
  for (int j = 0; j < n; ++j) {
    const uint32_t sr = packed_byte(sp, l.piv[j]);
    if (sr == 0) continue;  // e would be 0
    const int le = mod255(int(l.log[sr]) + int(l.pinvlog[j]));  // log e, e = s_r / H[r][j]
    bool match = true;
#pragma unroll
    for (int i = 0; i < MT; ++i)
      if (i < p) match = match && uint32_t(l.exp[le + int(l.hlog[i * n + j])]) == packed_byte(sp, i);
    if (match) {
      patch(d, j, col, l.exp[le]);
      atomicAdd(&hist[j], 1u);
      return kWeight1;
    }
  }
  if (max_errors < 2) return kUncorrectable;
  // weight 2: count the explanations over all pairs, stop at the second
  int found = 0, f1 = 0, f2 = 0;
  uint32_t e1f = 0, e2f = 0;
  for (int j1 = 0; j1 + 1 < n && found < 2; ++j1) {
    const int r = l.piv[j1];
    const uint32_t sr = packed_byte(sp, r);
    const int lc = sr ? mod255(int(l.log[sr]) + int(l.pinvlog[j1])) : kLogZero;  // log of s_r / H[r][j1]
    Pack tp;  // P(s)
#pragma unroll
    for (int i = 0; i < MT; ++i)
      if (i < p) pack_byte(tp, i, packed_byte(sp, i) ^ uint32_t(l.exp[lc + int(l.hlog[i * n + j1])]));
    for (int j2 = j1 + 1; j2 < n && found < 2; ++j2) {
      const int hr2 = l.hlog[r * n + j2];
      const int lg = hr2 < kLogZero ? mod255(hr2 + int(l.pinvlog[j1])) : kLogZero;  // log of H[r][j2] / H[r][j1]
      int le2 = -1;  // log e2, from the first nonzero row of P(H[:, j2])
      bool ok = true;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (i < p && ok) {
          const uint32_t qi = uint32_t(l.h[i * n + j2]) ^ uint32_t(l.exp[lg + int(l.hlog[i * n + j1])]);
          const uint32_t ti = packed_byte(tp, i);
          if (le2 < 0) {
            if (qi == 0)
              ok = ti == 0;
            else if (ti == 0)
              ok = false;  // e2 would be 0
            else
              le2 = mod255(int(l.log[ti]) + 255 - int(l.log[qi]));
          } else {
            ok = uint32_t(l.exp[le2 + int(l.log[qi])]) == ti;
          }
        }
      }
      if (!ok || le2 < 0) continue;
      const uint32_t x = sr ^ uint32_t(l.exp[le2 + hr2]);  // e1 . H[r][j1]
      if (x == 0) continue;  // e1 would be 0
      if (found == 0) {
        f1 = j1;
        f2 = j2;
        e1f = l.exp[mod255(int(l.log[x]) + int(l.pinvlog[j1]))];
        e2f = l.exp[le2];
      }
      ++found;
    }
  }
  if (found != 1) return kUncorrectable;
  patch(d, f1, col, e1f);
  patch(d, f2, col, e2f);
  atomicAdd(&hist[f1], 1u);
  atomicAdd(&hist[f2], 1u);
  return kWeight2;
}

// BATCH: grid.y = stripe; the stripe's own rows, mask row and n + 4 counts. A workgroup whose
// stripe's mask word is zero leaves before any barrier.
template <int MT, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_correct_kernel(DescView d, int n, int p, int64_t ncols, int bshift,
                                                            int span_shift, const int* mask, const uint8_t* loc,
                                                            int locatable, int max_errors, int bytewise,
                                                            unsigned long long* counts) {
  if constexpr (BATCH) {
    const uint64_t b = blockIdx.y;
    d.in += b * uint64_t(n);
    mask += b * uint64_t((ncols + (int64_t(1) << bshift) - 1) >> bshift);
    counts += b * uint64_t(n + 4);
  }
  const int64_t base = int64_t(blockIdx.x) << span_shift;
  if (mask[base >> bshift] == 0) return;  // (uniform: the whole workgroup leaves before any barrier)
  __shared__ CorLds l;
  for (int t = threadIdx.x; t < 1024; t += kBlock) l.exp[t] = t < kExpLen ? d_tab.exp[t] : uint8_t(0);
  for (int t = threadIdx.x; t < 256; t += kBlock) l.log[t] = d_tab.log[t];
  for (int t = threadIdx.x; t < p * n; t += kBlock) {
    l.h[t] = loc[t];
    l.hlog[t] = d_tab.log[loc[t]];
  }
  for (int t = threadIdx.x; t < n; t += kBlock) {
    l.piv[t] = loc[p * n + t];
    l.pinvlog[t] = d_tab.log[loc[p * n + n + t]];
  }
  for (int t = threadIdx.x; t < n + 4; t += kBlock) l.hist[t] = 0;
  __syncthreads();

  const int64_t end = std::min(base + (int64_t(1) << span_shift), ncols);
  Tally tally;
  uint32_t acc[MT];
  if (!bytewise) {
    for (int64_t c = base + int64_t(threadIdx.x) * 4; c < end; c += kBlock * 4) {
      if (c + 4 <= end) {
        syn_cols<MT, uint32_t>(d, n, MT, 0, c, acc);
        for (int q = 0; q < 4; ++q) tally.add(correct_col<MT>(l, l.hist, d, acc, q, c + q, n, p, locatable != 0, max_errors));
      } else {
        for (int64_t cc = c; cc < end; ++cc) {
          syn_cols<MT, uint8_t>(d, n, MT, 0, cc, acc);
          tally.add(correct_col<MT>(l, l.hist, d, acc, 0, cc, n, p, locatable != 0, max_errors));
        }
      }
    }
  } else {
    for (int64_t c = base + threadIdx.x; c < end; c += kBlock) {
      syn_cols<MT, uint8_t>(d, n, MT, 0, c, acc);
      tally.add(correct_col<MT>(l, l.hist, d, acc, 0, c, n, p, locatable != 0, max_errors));
    }
  }
  if (tally.w1) atomicAdd(&l.hist[n], tally.w1);
  if (tally.w2) atomicAdd(&l.hist[n + 1], tally.w2);
  if (tally.unc) atomicAdd(&l.hist[n + 2], tally.unc);
  if (tally.bad) atomicAdd(&l.hist[n + 3], tally.bad);
  __syncthreads();
  for (int t = threadIdx.x; t < n + 4; t += kBlock) {
    const uint32_t v = l.hist[t];
    if (v) atomicAdd(counts + t, (unsigned long long)v);
  }
}

template <bool BATCH>
hipError_t correct_launch(const DescView& d, int n, int p, unsigned batch, int64_t ncols, bool force_bytewise,
                          int bshift, const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                          uint64_t* counts, hipStream_t stream) {
  const int span_shift = std::min(bshift, kLocSpanShift);
  const int64_t nwg = (ncols + (int64_t(1) << span_shift) - 1) >> span_shift;
  return dispatch_tile(pad_m(p), [&](auto mt) -> hipError_t {
    constexpr int MT = decltype(mt)::value;
    gf_correct_kernel<MT, BATCH><<<dim3(unsigned(nwg), batch), kBlock, 0, stream>>>(
        d, n, p, ncols, bshift, span_shift, mask, loc, locatable ? 1 : 0, max_errors, force_bytewise ? 1 : 0,
        reinterpret_cast<unsigned long long*>(counts));
    return hipGetLastError();
  });
}

// what the locate launchers refuse, p < 2 (nothing can be corrected), and a pair search the kernel
// does not offer
bool correct_args_ok(int n, int p, int64_t ncols, int64_t block_bytes, int max_errors) {
  if (!locate_args_ok(n, p, ncols, block_bytes) || p < 2) return false;
  return max_errors == 1 || (max_errors == 2 && p >= 4 && n <= kCorrectMaxPairN);
}

}  // namespace

hipError_t launch_gf_correct(const void* desc, int n, int p, int64_t ncols, bool force_bytewise, int64_t block_bytes,
                             const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                             uint64_t* counts, hipStream_t stream) {
  if (!desc || !correct_args_ok(n, p, ncols, block_bytes, max_errors) || !mask || !loc || !counts)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, size_t(n + 4) * sizeof(uint64_t), stream);
  if (e != hipSuccess || ncols == 0) return e;
  return correct_launch<false>(view(desc, n, pad_m(p)), n, p, 1, ncols, force_bytewise, log2_exact(block_bytes), mask,
                               loc, locatable, max_errors, counts, stream);
}

hipError_t launch_gf_correct_batched(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                                     int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                     int max_errors, uint64_t* counts, hipStream_t stream) {
  if (batch < 1 || !desc || !correct_args_ok(n, p, ncols, block_bytes, max_errors) || !mask || !loc || !counts)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, size_t(batch) * size_t(n + 4) * sizeof(uint64_t), stream);
  if (ncols == 0) return e;
  const int bshift = log2_exact(block_bytes);
  const int64_t nmask = (ncols + block_bytes - 1) >> bshift;
  const DescView d0 = view(desc, n, pad_m(p), batch);
  for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridY) {
    DescView d = d0;
    d.in += size_t(b0) * size_t(n);
    e = correct_launch<true>(d, n, p, unsigned(std::min(batch - b0, kMaxGridY)), ncols, force_bytewise, bshift,
                             mask + size_t(b0) * size_t(nmask), loc, locatable, max_errors,
                             counts + size_t(b0) * size_t(n + 4), stream);
  }
  return e;
}

}  // namespace gfrs
