// In-place parity update on gfx950: the parity of a stripe in which d natives changed, without the
// other k - d natives (the delta identity of erasure-coded stores' small writes).
//
// Over byte columns [col0, col0 + ncols), one fused pass:
//     x_t[c]       = old_t[c] ^ new_t[c]    (pair form)   or   delta_t[c]   (delta form),  t < d
//     old_t[c]    <- new_t[c]               (store_new: the native row is overwritten in place)
//     parity_i[c] ^= XOR_t L[i][t](x_t[c])  i < p, read-modify-write in place
// L[i][t] is the byte map of E[i][changed[t]], in the five-word v_perm records of gf_gemm.hip, so
// GF(2^8) coefficients and the GF(16) nibble maps run on the same code.
//
// This is not a GEMM launch. A lane owns one 16-byte group: it issues the loads of all d (2 d) rows
// before its first multiply, forms the deltas in registers with one XOR per dword and keeps them
// for every parity row, so the inputs are read once whatever p is. The lane then walks the parity
// rows itself, a sub-tile of up to 4 rows at a time (loads, math, stores). Output tiles are not
// dealt to different blocks: with store_new the block that overwrites old_t would race one that
// still reads it, whereas a lane that reads and then writes its own 16 bytes of old_t is safe.
// d <= kUpdateMaxD per launch (32 VGPRs of deltas); callers split longer lists into passes, which
// XOR accumulation makes independent. No LDS, no atomics.
//
// Batched form (template flag BATCH, grid.y = stripe), for the small overwrites of a store of small
// objects, where one launch per stripe is launch-bound: `batch` stripes of one shape, each changing d
// natives OF ITS OWN. The record is update_batch_layout(k, d, m_pad, batch) (gfrs/desc.h): stripe b
// has in[b*d + t], copy[b*d + t], out[b*m_pad + i] and d int32 ids, ids[b*d + t] in [0, k); the
// table block holds the maps of all k natives and is shared. A wave never spans two stripes, so the
// ids are wave-uniform: they are read through the constant address space and moved into SGPRs at the
// top of the kernel (sgpr_int), and row t's table address is tab + (id_t * m_pad + i) * kPermStride,
// all scalar. Everything else is the single form, whose code the flag leaves as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "gfrs/desc.h"
#include "gfrs/kernels.h"
#include "gfrs/perm_device.h"

namespace gfrs {
namespace {

using namespace permdev;

enum Form { kDelta = 0, kPairs = 1, kWrite = 2 };  // kWrite = pairs with store_new

__device__ __forceinline__ uint8_t ldb(uint64_t base, int64_t off) {
  return __builtin_nontemporal_load((gptr<const uint8_t>)(base + uint64_t(off)));
}
__device__ __forceinline__ void stb(uint64_t base, int64_t off, uint8_t v) {
  __builtin_nontemporal_store(v, (gptr<uint8_t>)(base + uint64_t(off)));
}

// One byte column at row offset `off` (rows of any alignment): the ragged tail of the vector form
// and every lane of the byte form. d is a run-time count here; the delta bytes sit in registers
// through the unrolled, guarded loops.
// BATCH: row[t] is the table row (native id) of changed row t; else the table row is t itself.
template <int FORM, bool BATCH = false>
__device__ __forceinline__ void update_byte(const DescView& dv, int d, int m_pad, int64_t off,
                                            const int (&row)[kUpdateMaxD]) {
  uint32_t x[kUpdateMaxD], y[kUpdateMaxD];
#pragma unroll
  for (int t = 0; t < kUpdateMaxD; ++t) {
    x[t] = t < d ? uint32_t(ldb(dv.in[t], off)) : 0u;
    if constexpr (FORM != kDelta) y[t] = t < d ? uint32_t(ldb(dv.copy[t], off)) : 0u;
  }
  if constexpr (FORM != kDelta) {
#pragma unroll
    for (int t = 0; t < kUpdateMaxD; ++t) {
      if constexpr (FORM == kWrite) {
        if (t < d) stb(dv.in[t], off, uint8_t(y[t]));
      }
      x[t] ^= y[t];
    }
  }
  for (int i0 = 0; i0 < m_pad; i0 += 4) {
    uint64_t op[4];
    uint32_t acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      op[i] = i0 + i < m_pad ? dv.out[i0 + i] : 0;  // (0: a padding output, never touched)
      acc[i] = op[i] ? uint32_t(ldb(op[i], off)) : 0u;
    }
#pragma unroll
    for (int t = 0; t < kUpdateMaxD; ++t) {
      if (t < d) {
        const Sel s = make_sel(x[t]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // a padding slot past m_pad applies row m_pad - 1's map to an accumulator nobody stores
          const int ii = std::min(i0 + i, m_pad - 1);
          acc[i] = mac_map(acc[i], dv.tab + (size_t(BATCH ? row[t] : t) * m_pad + ii) * kPermStride, s);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (op[i]) stb(op[i], off, uint8_t(acc[i]));
  }
}

// Stripe b = blockIdx.y of a batched launch: its own d row pointers of each kind, its own m_pad
// output pointers and its own d ids (offsets formed in 64 bits), the ids moved into SGPRs. Called at
// the top of a kernel, before any divergent branch.
template <bool BATCH>
__device__ __forceinline__ void stripe(DescView& dv, cptr<int32_t> ids, int d, int m_pad, int (&row)[kUpdateMaxD]) {
  if constexpr (BATCH) {
    const uint64_t b = blockIdx.y;
    dv.in += b * uint64_t(d);
    dv.copy += b * uint64_t(d);
    dv.out += b * uint64_t(m_pad);
    ids += b * uint64_t(d);
#pragma unroll
    for (int t = 0; t < kUpdateMaxD; ++t)
      if (t < d) row[t] = sgpr_int(ids[t]);
  }
}

// Vector form. D = changed rows (compile time: the deltas are a register array), SUB = parity rows
// per sub-tile = min(4, m_pad), so every sub-tile row has a table column. Lanes [0, ngroups) own a
// 16-byte group each, lanes [ngroups, ngroups + tail) one byte of the ragged tail; the grid strides
// over the lanes when it was capped. `base` = col0, a multiple of 16 here.
// BATCH: `ids` are the batch's native ids and blockIdx.y the stripe (stripe()); else ids is null and
// never read.
template <int D, int SUB, int FORM, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_update_vec_kernel(DescView dv, int m_pad, int64_t base, int64_t ngroups,
                                                               int tail, int64_t nblk, cptr<int32_t> ids) {
  int row[kUpdateMaxD] = {};
  stripe<BATCH>(dv, ids, D, m_pad, row);
  for (int64_t cb = blockIdx.x; cb < nblk; cb += gridDim.x) {
    const int64_t g = cb * kBlock + threadIdx.x;
    if (g < ngroups) {
      const int64_t off = base + g * 16;
      u32x4 x[D];
#pragma unroll
      for (int t = 0; t < D; ++t) x[t] = ld16<true>(row_vec(dv.in[t], off));
      if constexpr (FORM != kDelta) {
        u32x4 y[D];
#pragma unroll
        for (int t = 0; t < D; ++t) y[t] = ld16<true>(row_vec(dv.copy[t], off));
#pragma unroll
        for (int t = 0; t < D; ++t) {
          if constexpr (FORM == kWrite) st16<true>(row_vec_w(dv.in[t], off), y[t]);
          x[t] ^= y[t];
        }
      }
      for (int i0 = 0; i0 < m_pad; i0 += SUB) {
        uint64_t op[SUB];
        uint32_t acc[SUB][4];
#pragma unroll
        for (int i = 0; i < SUB; ++i) op[i] = dv.out[i0 + i];
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (op[i]) v = ld16<true>(row_vec(op[i], off));
#pragma unroll
          for (int w = 0; w < 4; ++w) acc[i][w] = v[w];
        }
        uint64_t tb = (uint64_t)dv.tab;
#pragma unroll
        for (int t = 0; t < D; t += 2) {
          // (as gf_scrub.hip's rows kernel: the table pointer re-issued per row pair, so a pair's
          // scalar table loads wait only for the pair before it and are not all hoisted)
          asm volatile("" : "+s"(tb));
          const auto t0 = (cptr<uint32_t>)tb + (size_t(BATCH ? row[t] : t) * m_pad + i0) * kPermStride;
          if (t + 1 < D) {
            const auto t1 = BATCH ? (cptr<uint32_t>)tb + (size_t(row[t + 1]) * m_pad + i0) * kPermStride
                                  : t0 + size_t(m_pad) * kPermStride;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const Sel s0 = make_sel(x[t][w]);
              const Sel s1 = make_sel(x[t + 1][w]);
#pragma unroll
              for (int i = 0; i < SUB; ++i)
                acc[i][w] = mac_pair(acc[i][w], t0 + i * kPermStride, s0, t1 + i * kPermStride, s1);
            }
          } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const Sel s = make_sel(x[t][w]);
#pragma unroll
              for (int i = 0; i < SUB; ++i) acc[i][w] = mac_map(acc[i][w], t0 + i * kPermStride, s);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < SUB; ++i)
          if (op[i]) st16<true>(row_vec_w(op[i], off), u32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]});
      }
    } else if (g - ngroups < tail) {
      update_byte<FORM, BATCH>(dv, D, m_pad, base + ngroups * 16 + (g - ngroups), row);
    }
  }
}

// Byte form: one lane per byte column, rows of any alignment, any col0.
template <int FORM, bool BATCH = false>
__global__ __launch_bounds__(kBlock) void gf_update_byte_kernel(DescView dv, int d, int m_pad, int64_t base,
                                                                int64_t ncols, int64_t nblk, cptr<int32_t> ids) {
  int row[kUpdateMaxD] = {};
  stripe<BATCH>(dv, ids, d, m_pad, row);
  for (int64_t cb = blockIdx.x; cb < nblk; cb += gridDim.x) {
    const int64_t c = cb * kBlock + threadIdx.x;
    if (c < ncols) update_byte<FORM, BATCH>(dv, d, m_pad, base + c, row);
  }
}

// ---- launch -----------------------------------------------------------------------------------
// as gf_scrub.hip's make_grid with one tile: at most 2^32 - 1 work-items along x, the kernels stride
constexpr int64_t kMaxGridBlocks = int64_t(UINT32_MAX) / kBlock / 8 * 8;
struct Grid {
  int64_t nblk;
  unsigned blocks;
};
inline Grid make_grid(int64_t items) {
  Grid g{};
  g.nblk = (items + kBlock - 1) / kBlock;
  g.blocks = static_cast<unsigned>(std::min(g.nblk, kMaxGridBlocks));
  return g;
}

// In all of these BATCH picks the batched instantiation, `batch` is grid.y (1 when !BATCH) and `ids` the
// ids of the first stripe of the launch (null when !BATCH).
template <int D, int SUB, bool BATCH>
void launch_vec(int form, const DescView& dv, cptr<int32_t> ids, int m_pad, int64_t col0, int64_t ngroups, int tail,
                const Grid& g, unsigned batch, hipStream_t stream) {
  const dim3 grid(g.blocks, batch);
  if (form == kDelta)
    gf_update_vec_kernel<D, SUB, kDelta, BATCH>
        <<<grid, kBlock, 0, stream>>>(dv, m_pad, col0, ngroups, tail, g.nblk, ids);
  else if (form == kPairs)
    gf_update_vec_kernel<D, SUB, kPairs, BATCH>
        <<<grid, kBlock, 0, stream>>>(dv, m_pad, col0, ngroups, tail, g.nblk, ids);
  else
    gf_update_vec_kernel<D, SUB, kWrite, BATCH>
        <<<grid, kBlock, 0, stream>>>(dv, m_pad, col0, ngroups, tail, g.nblk, ids);
}

template <int D, bool BATCH>
void launch_vec_d(int form, const DescView& dv, cptr<int32_t> ids, int m_pad, int64_t col0, int64_t ngroups, int tail,
                  const Grid& g, unsigned batch, hipStream_t stream) {
  if (m_pad == 1)
    launch_vec<D, 1, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream);
  else if (m_pad == 2)
    launch_vec<D, 2, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream);
  else
    launch_vec<D, 4, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream);
}

// One launch over `batch` stripes (grid.y); `dv` and `ids` are those of the first of them.
template <bool BATCH>
hipError_t update_launch(const DescView& dv, cptr<int32_t> ids, int d, int m_pad, unsigned batch, int64_t col0,
                         int64_t ncols, int form, bool force_bytewise, hipStream_t stream) {
  if (force_bytewise || col0 % 16 != 0) {
    const Grid g = make_grid(ncols);
    const dim3 grid(g.blocks, batch);
    if (form == kDelta)
      gf_update_byte_kernel<kDelta, BATCH><<<grid, kBlock, 0, stream>>>(dv, d, m_pad, col0, ncols, g.nblk, ids);
    else if (form == kPairs)
      gf_update_byte_kernel<kPairs, BATCH><<<grid, kBlock, 0, stream>>>(dv, d, m_pad, col0, ncols, g.nblk, ids);
    else
      gf_update_byte_kernel<kWrite, BATCH><<<grid, kBlock, 0, stream>>>(dv, d, m_pad, col0, ncols, g.nblk, ids);
    return hipGetLastError();
  }
  const int64_t ngroups = ncols / 16;
  const int tail = int(ncols % 16);
  const Grid g = make_grid(ngroups + tail);  // one extra lane per ragged tail byte
  switch (d) {
    case 1: launch_vec_d<1, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    case 2: launch_vec_d<2, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    case 3: launch_vec_d<3, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    case 4: launch_vec_d<4, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    case 5: launch_vec_d<5, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    case 6: launch_vec_d<6, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    case 7: launch_vec_d<7, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
    default: launch_vec_d<8, BATCH>(form, dv, ids, m_pad, col0, ngroups, tail, g, batch, stream); break;
  }
  return hipGetLastError();
}

bool update_args_ok(int d, int m_pad, int64_t col0, int64_t ncols, bool pairs, bool store_new) {
  return d >= 1 && d <= kUpdateMaxD && m_pad >= 1 && m_pad <= 256 && m_pad % tile_for(m_pad) == 0 && col0 >= 0 &&
         ncols >= 0 && (pairs || !store_new);
}

constexpr int kMaxGridY = 65535;  // stripes per launch, as launch_gf_syndrome_batched

}  // namespace

hipError_t launch_gf_update(const void* desc, int d, int m_pad, int64_t col0, int64_t ncols, bool pairs,
                            bool store_new, bool force_bytewise, hipStream_t stream) {
  if (!desc || !update_args_ok(d, m_pad, col0, ncols, pairs, store_new)) return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const int form = store_new ? kWrite : (pairs ? kPairs : kDelta);
  return update_launch<false>(view(desc, d, m_pad), nullptr, d, m_pad, 1, col0, ncols, form, force_bytewise, stream);
}

hipError_t launch_gf_update_batched(const void* desc, int k, int d, int m_pad, int batch, int64_t col0, int64_t ncols,
                                    bool pairs, bool store_new, bool force_bytewise, hipStream_t stream) {
  if (!desc || batch < 1 || k < 1 || k > 256 || !update_args_ok(d, m_pad, col0, ncols, pairs, store_new))
    return hipErrorInvalidValue;
  if (ncols == 0) return hipSuccess;
  const int form = store_new ? kWrite : (pairs ? kPairs : kDelta);
  const UpdateBatchLayout l = update_batch_layout(k, d, m_pad, batch);
  const char* base = static_cast<const char*>(desc);
  const DescView d0{(cptr<uint64_t>)(base + l.in_off), (cptr<uint64_t>)(base + l.copy_off),
                    (cptr<uint64_t>)(base + l.out_off), (cptr<uint32_t>)(base + l.tab_off)};
  const auto ids0 = (cptr<int32_t>)(base + l.ids_off);
  hipError_t e = hipSuccess;
  for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridY) {
    DescView dv = d0;
    dv.in += size_t(b0) * size_t(d);
    dv.copy += size_t(b0) * size_t(d);
    dv.out += size_t(b0) * size_t(m_pad);
    e = update_launch<true>(dv, ids0 + size_t(b0) * size_t(d), d, m_pad, unsigned(std::min(batch - b0, kMaxGridY)),
                            col0, ncols, form, force_bytewise, stream);
  }
  return e;
}

}  // namespace gfrs
