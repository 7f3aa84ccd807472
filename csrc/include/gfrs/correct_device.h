// The per-column decoder of the cold passes that repair (gf_correct.hip on a whole stripe,
// gf_checked.hip on the survivors of a degraded one): its LDS tables, the packed syndrome bytes, a
// lane's tally and the rule itself. Include from a .hip file only.
//
// A cold pass recomputes the syndrome s = H . stripe[:, c] of each byte column under a p x n check
// matrix H and, for s != 0, applies the rule:
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
// How a repair is applied is the caller's (the Fix functor of decode_col): columns are independent,
// so a lane's byte stores meet no other lane's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gfrs/gf256.h"
#include "gfrs/perm_device.h"

namespace gfrs {
namespace scrubdev {

using namespace permdev;

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

}  // namespace scrubdev
}  // namespace gfrs
