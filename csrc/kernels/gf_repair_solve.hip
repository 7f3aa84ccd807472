// Repair coefficients solved on gfx950: one workgroup per distinct erasure pattern, everything in LDS.
//
// A repair rewrites rows `erased` (natives and/or parity) of a stripe from k surviving rows:
//     rows[erased] = G[erased] . inv(G[surv]) . rows[surv]
// The host path inverts G[surv] (k x k) per pattern, multiplies and expands the product into v_perm
// records with numpy. Here the pattern's coefficient rows are solved the erasure-code way, as
// gf_decode_system_kernel (gf_invert.hip) does for the natives, and extended to parity rows. With
//     N  = the natives among the survivors,      Mn = the natives not among them (a of them),
//     P  = the parity survivors (also a of them, since the k survivors are distinct),
// the natives in Mn satisfy G[P, Mn] x_Mn = y_P + G[P, N] x_N (characteristic 2), so their
// coefficient rows over the survivors are X = M^-1 B' with M = G[P, Mn] (a x a) and
//     B'[r][c] = G[P_r][surv_c] for a native survivor c,  [surv_c == P_r] for a parity survivor c.
// An erased parity row x is G[x, N] x_N + G[x, Mn] x_Mn: its coefficients are the base row
//     base_x[c] = G[x][surv_c] for a native survivor c, 0 for a parity survivor c
// plus G[x, Mn] . X. Both come out of ONE elimination: the system [M | B'] gets one extra row
// [G[x, Mn] | base_x] per erased parity row. Extra rows are never pivot candidates, but every pivot
// column is eliminated from them like from any other row, so when the a columns are done their left
// part is zero and their right part is base_x + G[x, Mn] M^-1 B', the Schur complement, which is the
// coefficient row. With a = 0 (only parity lost, all natives alive) nothing is eliminated and the
// rows are rows of E. The rows are unique whenever G[surv] is invertible, so they equal the host's
// G[erased] . inv(G[surv]) byte for byte.
//
// Pivot rule, bid slots, unnormalised pivot rows and the one barrier per column are those of
// gf_decode_system_kernel: the lowest unused row among the a rows of M with a nonzero entry; a column
// without one gives status 1.
//
// Sizes (n <= 256): rows a + b <= n - k (P and the erased parity rows are disjoint parity ids),
// width a + k <= min(2 k, n), so the system is at most 128 x 256 bytes (k = 128, n = 256): 33 KiB of
// LDS next to 3.9 KiB of tables and id lists, inside the 64 KiB a kernel gets without opting in and
// far inside a CU's 160 KiB. Small codes take a few hundred bytes, so several workgroups share a CU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gfrs/desc.h"
#include "gfrs/kernels.h"

namespace gfrs {
namespace {

__constant__ Tables d_gf_tables = make_tables();

__device__ __forceinline__ uint32_t xtime(uint32_t x) { return ((x << 1) ^ ((x & 0x80u) ? 0x1Du : 0u)) & 0xFFu; }

// v_perm table of "multiply by f" (same layout as gfrs::perm_for_coeff; gf_invert.hip's perm_of).
__device__ __forceinline__ void perm_of(uint32_t f, uint32_t t[5]) {
  uint32_t b[8];
  b[0] = f & 0xFFu;
#pragma unroll
  for (int i = 1; i < 8; ++i) b[i] = xtime(b[i - 1]);
  auto tri = [](uint32_t x0, uint32_t x1, uint32_t x2, uint32_t& lo, uint32_t& hi) {
    lo = (x0 << 8) | (x1 << 16) | ((x0 ^ x1) << 24);
    hi = x2 | ((x2 ^ x0) << 8) | ((x2 ^ x1) << 16) | ((x2 ^ x1 ^ x0) << 24);
  };
  tri(b[0], b[1], b[2], t[0], t[1]);
  tri(b[3], b[4], b[5], t[2], t[3]);
  t[4] = (b[6] << 8) | (b[7] << 16) | ((b[6] ^ b[7]) << 24);
}

__device__ __forceinline__ uint32_t apply4(const uint32_t t[5], uint32_t w) {
  return __builtin_amdgcn_perm(t[1], t[0], w & 0x07070707u) ^
         __builtin_amdgcn_perm(t[3], t[2], (w >> 3) & 0x07070707u) ^
         __builtin_amdgcn_perm(0u, t[4], (w >> 6) & 0x03030303u);
}

// LDS before the system: exp 1024 | log 512 | misc 64 (piv_s) | survivor bits 32 | erased bits 32 |
// seven 256-byte id lists | erased ids as int16 512.
constexpr size_t kSolveFixed = 1024 + 512 + 64 + 32 + 32 + 7 * 256 + 512;

struct SolveShape {
  int rows, pw;  // the most system rows of any pattern, and the widest row pitch in dwords
  size_t lds;
};
inline SolveShape solve_shape(int n, int k, int m_pad) {
  const int a_max = std::min(k, n - k);
  SolveShape s{};
  s.rows = std::min(n - k, a_max + m_pad);
  s.pw = ((k + a_max + 3) / 4) | 1;
  s.lds = kSolveFixed + 4 * size_t(s.rows) * size_t(s.pw);
  return s;
}

// Prefix position of the lanes of wave 0 whose `flag` is set, continuing from `base`.
__device__ __forceinline__ int wave_rank(bool flag, int lane, int& base) {
  const unsigned long long bal = __ballot(flag);
  const int at = base + __popcll(bal & ((1ull << lane) - 1ull));
  base += __popcll(bal);
  return at;
}

template <int B>
__global__ __launch_bounds__(B) void gf_repair_solve_kernel(const uint8_t* __restrict__ g, int n, int k,
                                                            const int* __restrict__ surv,
                                                            const int* __restrict__ erased, int m_pad,
                                                            uint8_t* __restrict__ coeff, uint32_t* __restrict__ tab,
                                                            int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* exp_s = smem;
  uint16_t* log_s = reinterpret_cast<uint16_t*>(smem + 1024);
  // [0..2] pivot-search slots, [3] parity survivors, [4] bad, [5] missing natives, [6] erased parity rows
  int* piv_s = reinterpret_cast<int*>(smem + 1536);
  uint32_t* seen_s = reinterpret_cast<uint32_t*>(smem + 1600);   // bit per chunk id: a survivor
  uint32_t* seen_e = reinterpret_cast<uint32_t*>(smem + 1632);   // bit per chunk id: erased
  uint8_t* perm_s = smem + 1664;     // perm_s[c] = pivot row of column c
  uint8_t* rowid_s = perm_s + 256;   // chunk id of system row r: P in survivor order, then the erased parity rows
  uint8_t* surv_s = rowid_s + 256;
  uint8_t* mn_s = surv_s + 256;      // missing natives, ascending
  uint8_t* mnpos_s = mn_s + 256;     // native id -> its index in mn_s
  uint8_t* pinv_s = mnpos_s + 256;   // 1 / M[perm_s[c]][c]
  uint8_t* xrow_s = pinv_s + 256;    // output row i (an erased parity row) -> its system row
  int16_t* er_s = reinterpret_cast<int16_t*>(xrow_s + 256);  // erased ids, -1 = no row
  uint32_t* M = reinterpret_cast<uint32_t*>(smem + kSolveFixed);
  uint8_t* Mb = reinterpret_cast<uint8_t*>(M);

  const int tid = threadIdx.x;
  const size_t q = blockIdx.x;
  surv += q * size_t(k);
  erased += q * size_t(m_pad);

  for (int i = tid; i < kExpLen; i += B) exp_s[i] = d_gf_tables.exp[i];
  for (int i = kExpLen + tid; i < 1024; i += B) exp_s[i] = 0;
  for (int i = tid; i < 256; i += B) log_s[i] = d_gf_tables.log[i];
  if (tid < 16) piv_s[tid] = 0;
  if (tid < 16) seen_s[tid] = 0;  // (seen_s and seen_e are adjacent: 16 words)
  __syncthreads();
  // 1. the lists: ids in range, survivors distinct, erased ids distinct and none a survivor
  for (int i = tid; i < k; i += B) {
    const int r = surv[i];
    const bool ok = r >= 0 && r < n;
    surv_s[i] = uint8_t(ok ? r : 0);
    if (!ok || (atomicOr(&seen_s[r >> 5], 1u << (r & 31)) >> (r & 31) & 1u)) piv_s[4] = 1;
  }
  __syncthreads();
  for (int i = tid; i < m_pad; i += B) {
    const int x = erased[i];
    const bool ok = x >= 0 && x < n;
    er_s[i] = int16_t(ok ? x : -1);
    if (x == -1) continue;  // padding
    if (!ok || (seen_s[x >> 5] >> (x & 31) & 1u) || (atomicOr(&seen_e[x >> 5], 1u << (x & 31)) >> (x & 31) & 1u))
      piv_s[4] = 1;
  }
  __syncthreads();
  if (tid < 64) {  // wave 0: three ballot prefix sums
    int base = 0;  // missing natives, ascending
    for (int i0 = 0; i0 < k; i0 += 64) {
      const int i = i0 + tid;
      const bool miss = i < k && !(seen_s[i >> 5] >> (i & 31) & 1u);
      const int at = wave_rank(miss, tid, base);
      if (miss) {
        mn_s[at] = uint8_t(i);
        mnpos_s[i] = uint8_t(at);
      }
    }
    const int nmiss = base;
    base = 0;  // parity survivors, in survivor order
    for (int j0 = 0; j0 < k; j0 += 64) {
      const int j = j0 + tid;
      const bool is_par = j < k && surv_s[j] >= k;
      const int at = wave_rank(is_par, tid, base);
      if (is_par) rowid_s[at] = surv_s[j];
    }
    const int a = base;
    // erased parity rows, in list order, after the a rows of M. Distinct, in [k, n) and disjoint from
    // P unless the pattern is bad, so a + b <= n - k <= 255; a bad pattern may count past that and
    // stores nothing then (its lists are never used).
    for (int i0 = 0; i0 < m_pad; i0 += 64) {
      const int i = i0 + tid;
      const bool is_par = i < m_pad && er_s[i] >= k;
      const int at = wave_rank(is_par, tid, base);
      if (is_par && at < 256) {
        rowid_s[at] = uint8_t(er_s[i]);
        xrow_s[i] = uint8_t(at);
      }
    }
    if (tid == 0) {
      piv_s[3] = a;
      piv_s[5] = nmiss;
      piv_s[6] = base - a;
      piv_s[0] = piv_s[1] = piv_s[2] = a;
    }
  }
  __syncthreads();
  const int a = piv_s[3];
  const int R = a + piv_s[6];
  // (uniform: every lane reads the same LDS words after the barrier)
  if (piv_s[4] || piv_s[5] != a || R > n - k) {
    if (tid == 0) status[q] = 2;
    return;
  }
  const int W = a + k;
  const int PW = (((W + 3) / 4) | 1);  // row pitch in dwords, odd => conflict-free column walks
  auto byte_at = [&](int r, int col) -> uint8_t& { return Mb[(r * PW) * 4 + col]; };

  // 2. the R x (a + k) system (pitch padding is never read as a byte, but is walked as dwords)
  for (int i = tid; i < R * PW; i += B) M[i] = 0;
  __syncthreads();
  for (int i0 = tid; i0 < R * W; i0 += 8 * B) {  // 8 independent global loads in flight per lane
    uint8_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * B;
      if (i >= R * W) break;
      const int r = i / W, col = i - r * W;
      const int id = rowid_s[r];
      const size_t grow = size_t(id) * k;
      if (col < a) {
        v[u] = g[grow + mn_s[col]];
      } else {
        const int s = surv_s[col - a];
        v[u] = s < k ? g[grow + s] : uint8_t(s == id);  // (an erased row is no survivor: 0 there)
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * B;
      if (i >= R * W) break;
      const int r = i / W;
      byte_at(r, i - r * W) = v[u];
    }
  }
  __syncthreads();

  // Gauss-Jordan over the a columns of M, one barrier per column, no row swaps (gf_invert.hip's
  // gf_decode_system_kernel). The TPR lanes of row r sit in one wave (TPR divides 64) and read the
  // row's factor before any of them writes the row.
  int TPR = 1;
  while (TPR * 2 * R <= B && TPR < 64) TPR <<= 1;
  const int r = tid / TPR, sub = tid % TPR;  // at most one row per lane group: B / TPR >= R
  bool used = false;
  int singular = 0;
  if (a > 0 && sub == 0 && r < a && byte_at(r, 0)) atomicMin(&piv_s[0], r);
  __syncthreads();
  for (int c = 0; c < a; ++c) {
    const int p = piv_s[c % 3];
    if (p >= a) {  // uniform
      singular = 1;
      break;
    }
    if (tid == 0) {
      piv_s[(c + 2) % 3] = a;
      perm_s[c] = uint8_t(p);
    }
    if (r < R && r != p) {
      const uint32_t f = byte_at(r, c);
      if (f) {
        uint32_t t[5];
        perm_of(exp_s[log_s[f] + 255 - log_s[byte_at(p, c)]], t);
        // batches of 8 dwords: all LDS reads issued before the writes (r != p, so no aliasing)
        int w = sub;
        for (; w + 7 * TPR < PW; w += 8 * TPR) {
          uint32_t pv[8], rv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            pv[u] = M[p * PW + w + u * TPR];
            rv[u] = M[r * PW + w + u * TPR];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) M[r * PW + w + u * TPR] = rv[u] ^ apply4(t, pv[u]);
        }
        for (; w < PW; w += TPR) M[r * PW + w] ^= apply4(t, M[p * PW + w]);
      }
      // only the rows of M bid; the extra rows are eliminated but never pivot
      if (r < a && !used && c + 1 < a && sub == ((c + 1) >> 2) % TPR && byte_at(r, c + 1))
        atomicMin(&piv_s[(c + 1) % 3], r);
    }
    if (r == p) used = true;
    __syncthreads();
  }
  if (tid == 0) status[q] = singular;
  if (singular) return;
  for (int b = tid; b < a; b += B) pinv_s[b] = exp_s[255 - log_s[byte_at(perm_s[b], b)]];
  __syncthreads();

  // 3. coefficient of output row i, survivor column j
  auto c_at = [&](int i, int j) -> uint32_t {
    const int x = er_s[i];
    if (x < 0) return 0u;
    if (x >= k) return byte_at(xrow_s[i], a + j);
    const int b = mnpos_s[x];
    return exp_s[log_s[byte_at(perm_s[b], a + j)] + log_s[pinv_s[b]]];
  };
  if (coeff) {
    uint8_t* dst = coeff + q * size_t(m_pad) * size_t(k);
    for (int idx = tid; idx < m_pad * k; idx += B) {
      const int i = idx / k;
      dst[idx] = uint8_t(c_at(i, idx - i * k));
    }
  }
  if (tab) {  // tab[q][j][i] = perm(c[i][j]), rows past the pattern's erasures zero
    uint32_t* blk = tab + q * size_t(k) * size_t(m_pad) * kPermStride;
    for (int idx = tid; idx < k * m_pad; idx += B) {
      const int j = idx / m_pad, i = idx - j * m_pad;
      uint32_t t[5];
      perm_of(c_at(i, j), t);
      uint32_t* dst = blk + size_t(idx) * kPermStride;
#pragma unroll
      for (int w = 0; w < 5; ++w) dst[w] = t[w];
      dst[5] = dst[6] = dst[7] = 0;
    }
  }
}

}  // namespace

int64_t repair_solve_lds_bytes(int n, int k, int m_pad) {
  if (k < 1 || k > n || n > 256 || m_pad < 1 || m_pad > 256) return -1;
  return int64_t(solve_shape(n, k, m_pad).lds);
}

hipError_t launch_gf_repair_solve(const uint8_t* g, int n, int k, const int* surv, const int* erased, int npat,
                                  int m_pad, uint8_t* coeff, void* tab, int* status, hipStream_t stream) {
  if (npat < 0 || k < 1 || k > n || n > 256 || m_pad < 1 || m_pad > 256) return hipErrorInvalidValue;
  if (npat == 0) return hipSuccess;
  if (!g || !surv || !erased || !status) return hipErrorInvalidValue;
  const SolveShape s = solve_shape(n, k, m_pad);
  if (s.lds > 65536) return hipErrorInvalidValue;  // (no n <= 256 gets here: the header comment has the sizes)
  gf_repair_solve_kernel<256><<<unsigned(npat), 256, s.lds, stream>>>(g, n, k, surv, erased, m_pad, coeff,
                                                                      static_cast<uint32_t*>(tab), status);
  return hipGetLastError();
}

}  // namespace gfrs
