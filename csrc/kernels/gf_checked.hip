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
//     gf_correct.hip's decoder (copied below) with the r x ns check matrix T[e:, S]. A corrected survivor byte j
//     gets ^= v, and every erased row i then ^= v . T[i][j], so it holds the value rebuilt from the
//     corrected survivors. An uncorrectable column keeps its survivors and the hot pass's rebuild.
//     Counts as gf_correct.hip: fixed_bytes[ns] by survivor index, weight-1, weight-2,
//     uncorrectable and bad columns.
// BATCH: grid.y = stripe, one erasure pattern (one T) for the whole batch.
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

// ---- the per-column decoder --------------------------------------------------------------------
// A copy of gf_correct.hip's (its LDS tables, packed syndrome bytes, tally and the weight-1 / pair
// search of correct_col, which documents the rule), with the repair handed to a functor so the erased
// rows can follow it. Shared through scrub_device.h it changed what gf_correct.hip compiles to
// (register allocation and schedule of gf_correct_kernel), so the ~80 lines live here too.
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

// The workgroup fills the tables from the field's tables and the loc operand (H row-major p x n,
// the pivot rows, the pivots' inverses) and zeroes the histogram; the caller syncs.
template <typename Tab>
__device__ __forceinline__ void fill_cor_lds(CorLds& l, const Tab& tab, const uint8_t* loc, int n, int p) {
  for (int t = threadIdx.x; t < 1024; t += kBlock) l.exp[t] = t < kExpLen ? tab.exp[t] : uint8_t(0);
  for (int t = threadIdx.x; t < 256; t += kBlock) l.log[t] = tab.log[t];
  for (int t = threadIdx.x; t < p * n; t += kBlock) {
    l.h[t] = loc[t];
    l.hlog[t] = tab.log[loc[t]];
  }
  for (int t = threadIdx.x; t < n; t += kBlock) {
    l.piv[t] = loc[p * n + t];
    l.pinvlog[t] = tab.log[loc[p * n + n + t]];
  }
  for (int t = threadIdx.x; t < n + 4; t += kBlock) l.hist[t] = 0;
}

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
  // into the histogram's four totals after its n chunk bins
  __device__ __forceinline__ void flush(uint32_t* hist, int n) const {
    if (w1) atomicAdd(&hist[n], w1);
    if (w2) atomicAdd(&hist[n + 1], w2);
    if (unc) atomicAdd(&hist[n + 2], unc);
    if (bad) atomicAdd(&hist[n + 3], bad);
  }
};

// The rule on one bad column with syndrome bytes `sp` (nonzero) under the p x n check matrix in `l`.
// fix.patch(j, e): chunk j's byte gets ^= e; fix.count(j): one more byte fixed in chunk j. A weight-2
// repair patches both chunks, then counts both.
template <int MT, typename Fix>
__device__ __forceinline__ Outcome decode_col(const CorLds& l, const Pack& sp, int n, int p, bool locatable,
                                           int max_errors, Fix&& fix) {
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
      fix.patch(j, l.exp[le]);
      fix.count(j);
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
  fix.patch(f1, e1f);
  fix.patch(f2, e2f);
  fix.count(f1);
  fix.count(f2);
  return kWeight2;
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
  if constexpr (BATCH) {
    const uint64_t b = blockIdx.y;
    d.in += b * uint64_t(ns);
    d.out += b * uint64_t(MT);
    mask += b * uint64_t((ncols + (int64_t(1) << bshift) - 1) >> bshift);
    counts += b * uint64_t(ns + 4);
  }
  const int64_t base = int64_t(blockIdx.x) << span_shift;
  if (mask[base >> bshift] == 0) return;  // (uniform: the whole workgroup leaves before any barrier)
  __shared__ CorLds l;
  fill_cor_lds(l, d_tab, loc, ns, r);
  __syncthreads();

  const uint8_t* reb = loc + r * ns + 2 * ns;
  const int64_t end = std::min(base + (int64_t(1) << span_shift), ncols);
  const bool loc_ok = locatable != 0;
  Tally tally;
  uint32_t acc[MT];
  if (!bytewise) {
    for (int64_t c = base + int64_t(threadIdx.x) * 4; c < end; c += kBlock * 4) {
      if (c + 4 <= end) {
        syn_cols<MT, uint32_t>(d, ns, MT, 0, c, acc);
        for (int q = 0; q < 4; ++q)
          tally.add(fix_col<MT>(l, l.hist, d, reb, acc, q, c + q, ns, e, r, loc_ok, max_errors));
      } else {
        for (int64_t cc = c; cc < end; ++cc) {
          syn_cols<MT, uint8_t>(d, ns, MT, 0, cc, acc);
          tally.add(fix_col<MT>(l, l.hist, d, reb, acc, 0, cc, ns, e, r, loc_ok, max_errors));
        }
      }
    }
  } else {
    for (int64_t c = base + threadIdx.x; c < end; c += kBlock) {
      syn_cols<MT, uint8_t>(d, ns, MT, 0, c, acc);
      tally.add(fix_col<MT>(l, l.hist, d, reb, acc, 0, c, ns, e, r, loc_ok, max_errors));
    }
  }
  tally.flush(l.hist, ns);
  __syncthreads();
  for (int t = threadIdx.x; t < ns + 4; t += kBlock) {
    const uint32_t v = l.hist[t];
    if (v) atomicAdd(counts + t, (unsigned long long)v);
  }
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

template <bool BATCH>
hipError_t checked_launch(const DescView& d, int ns, int e, int r, unsigned batch, int64_t ncols, bool force_bytewise,
                          int bshift, int* mask, hipStream_t stream) {
  return dispatch_tile(pad_m(e + r), [&](auto mt) -> hipError_t {
    constexpr int MT = decltype(mt)::value;
    if (force_bytewise) {
      const Grid g = make_grid(ncols, 1);
      gf_checked_byte_kernel<MT, BATCH>
          <<<dim3(g.blocks, batch), kBlock, 0, stream>>>(d, ns, e, r, ncols, g.nblk, g.ncb, mask, bshift);
      return hipGetLastError();
    }
    const int64_t ngroups = ncols / 16;
    const int tail = int(ncols % 16);
    const Grid g = make_grid(ngroups + tail, 1);  // one extra lane per ragged tail byte
    gf_checked_vec_kernel<MT, BATCH>
        <<<dim3(g.blocks, batch), kBlock, 0, stream>>>(d, ns, e, r, ngroups, g.nblk, g.ncb, tail, mask, bshift);
    return hipGetLastError();
  });
}

template <bool BATCH>
hipError_t fix_launch(const DescView& d, int ns, int e, int r, unsigned batch, int64_t ncols, bool force_bytewise,
                      int bshift, const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                      uint64_t* counts, hipStream_t stream) {
  const int span_shift = std::min(bshift, kLocSpanShift);
  const int64_t nwg = (ncols + (int64_t(1) << span_shift) - 1) >> span_shift;
  return dispatch_tile(pad_m(e + r), [&](auto mt) -> hipError_t {
    constexpr int MT = decltype(mt)::value;
    gf_checked_fix_kernel<MT, BATCH><<<dim3(unsigned(nwg), batch), kBlock, 0, stream>>>(
        d, ns, e, r, ncols, bshift, span_shift, mask, loc, locatable ? 1 : 0, max_errors, force_bytewise ? 1 : 0,
        reinterpret_cast<unsigned long long*>(counts));
    return hipGetLastError();
  });
}

}  // namespace

hipError_t launch_gf_checked(const void* desc, int ns, int e, int r, int64_t ncols, bool force_bytewise,
                             int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  if (!desc || !checked_args_ok(ns, e, r, ncols, block_bytes) || !mask) return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const int bshift = log2_exact(block_bytes);
  const int64_t nmask = (ncols + block_bytes - 1) >> bshift;
  hipError_t err = hipMemsetAsync(mask, 0, size_t(nmask) * sizeof(int32_t), stream);
  if (err != hipSuccess) return err;
  return checked_launch<false>(view(desc, ns, pad_m(e + r)), ns, e, r, 1, ncols, force_bytewise, bshift, mask, stream);
}

hipError_t launch_gf_checked_batched(const void* desc, int ns, int e, int r, int batch, int64_t ncols,
                                     bool force_bytewise, int64_t block_bytes, int32_t* mask, hipStream_t stream) {
  if (batch < 1 || !desc || !checked_args_ok(ns, e, r, ncols, block_bytes) || !mask) return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const int bshift = log2_exact(block_bytes);
  const int64_t nmask = (ncols + block_bytes - 1) >> bshift;
  const int mt = pad_m(e + r);
  hipError_t err = hipMemsetAsync(mask, 0, size_t(batch) * size_t(nmask) * sizeof(int32_t), stream);
  const DescView d0 = view(desc, ns, mt, batch);
  for (int b0 = 0; b0 < batch && err == hipSuccess; b0 += kMaxGridY) {
    DescView d = d0;
    d.in += size_t(b0) * size_t(ns);
    d.out += size_t(b0) * size_t(mt);
    err = checked_launch<true>(d, ns, e, r, unsigned(std::min(batch - b0, kMaxGridY)), ncols, force_bytewise, bshift,
                               mask + size_t(b0) * size_t(nmask), stream);
  }
  return err;
}

hipError_t launch_gf_checked_fix(const void* desc, int ns, int e, int r, int64_t ncols, bool force_bytewise,
                                 int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                 int max_errors, uint64_t* counts, hipStream_t stream) {
  if (!desc || !fix_args_ok(ns, e, r, ncols, block_bytes, max_errors) || !mask || !loc || !counts)
    return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, size_t(ns + 4) * sizeof(uint64_t), stream);
  if (err != hipSuccess || ncols == 0) return err;
  return fix_launch<false>(view(desc, ns, pad_m(e + r)), ns, e, r, 1, ncols, force_bytewise, log2_exact(block_bytes),
                           mask, loc, locatable, max_errors, counts, stream);
}

hipError_t launch_gf_checked_fix_batched(const void* desc, int ns, int e, int r, int batch, int64_t ncols,
                                         bool force_bytewise, int64_t block_bytes, const int32_t* mask,
                                         const uint8_t* loc, bool locatable, int max_errors, uint64_t* counts,
                                         hipStream_t stream) {
  if (batch < 1 || !desc || !fix_args_ok(ns, e, r, ncols, block_bytes, max_errors) || !mask || !loc || !counts)
    return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, size_t(batch) * size_t(ns + 4) * sizeof(uint64_t), stream);
  if (ncols == 0) return err;
  const int bshift = log2_exact(block_bytes);
  const int64_t nmask = (ncols + block_bytes - 1) >> bshift;
  const int mt = pad_m(e + r);
  const DescView d0 = view(desc, ns, mt, batch);
  for (int b0 = 0; b0 < batch && err == hipSuccess; b0 += kMaxGridY) {
    DescView d = d0;
    d.in += size_t(b0) * size_t(ns);
    d.out += size_t(b0) * size_t(mt);
    err = fix_launch<true>(d, ns, e, r, unsigned(std::min(batch - b0, kMaxGridY)), ncols, force_bytewise, bshift,
                           mask + size_t(b0) * size_t(nmask), loc, locatable, max_errors,
                           counts + size_t(b0) * size_t(ns + 4), stream);
  }
  return err;
}

}  // namespace gfrs
