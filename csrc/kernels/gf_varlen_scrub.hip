// Variable-length scrub on gfx950: which of `batch` stripes of one code, each with a row length OF ITS
// OWN, are inconsistent, in which column blocks, and which chunk is wrong there. It joins three things
// the tree already has and adds no math of its own:
//   * the flat (stripe, column block) work list of gf_varlen.hip: blk_stripe[w] read through the
//     constant address space and moved into an SGPR, so a workgroup never spans two stripes and
//     everything per stripe (row pointers, length, first mask word) is wave-uniform and read with
//     scalar loads; `w += gridDim.x` when the grid was capped;
//   * the syndrome fold and mask rule of gfrs/scrub_device.h (group_bits, the ballots of wave_or,
//     wave_block) on gf_syndrome_vec_kernel's loop: non-temporal 16-byte loads, two rows in flight,
//     mac_pair / mac_map over the one shared table block of H, nothing stored;
//   * the locate classifier of gf_scrub.hip (LocLds / classify, gfrs/scrub_device.h) with the cold
//     scaffold's sweep_span and flush_bins.
//
// Hot pass, gf_varlen_syndrome_{vec,byte}_kernel<MT>: lanes [0, len / 16) of a stripe own a 16-byte
// group each, the next len % 16 lanes one byte of the ragged tail, later lanes nothing (byte form: one
// lane per column, for a batch with any live row off 16-byte alignment). A work item walks ALL output
// tiles of its columns in a loop (i0 += MT) instead of making (work item, tile) the grid unit: one
// tile is the whole of every code with p <= 16, the work list then needs no second coordinate, and a
// wider code re-reads its 4 KiB of columns per tile from L2 as the tiles of the (column block, tile)
// grid of gf_scrub.hip do. Each wave ORs its row bits with ballots, and lane 0 issues one atomicOr
// into the block word mask[mask_first[b] + (column >> bshift)] and one into the stripe word
// mask[nwords + b], only when a bit is set: a clean batch stores nothing. IDENT (H = [E | I_p], one
// tile of all p rows, MT <= 8): the parity rows are XORed in as they are, k x p multiplies, not n x p.
// No compile-time rows-in-flight instance: gf_syndrome_rows_kernel has no item loop (around a loop
// its table words are hoisted and spilled), and none has been measured here.
//
// Cold pass, gf_varlen_locate_kernel<MT>: a second flat list of (stripe, span) items, a span being
// min(block_bytes, 16 KiB) columns. A workgroup whose block word is zero goes on to its next item (it
// leaves, when the grid is not capped) before any barrier; a dirty one classifies every byte column of
// its span into the stripe's own n + 2 counts.
//
// Every offset is formed in 64 bits; a lane touches only columns below len[b].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "gfrs/desc.h"
#include "gfrs/kernels.h"
#include "gfrs/perm_device.h"
#include "gfrs/scrub_device.h"

namespace gfrs {
namespace {

using namespace permdev;
using namespace scrubdev;

__constant__ Tables d_tab = make_tables();

struct ScrubView {
  cptr<uint64_t> in;        // [batch * n]
  cptr<int64_t> len;        // [batch]
  cptr<int64_t> first;      // [batch] first hot work item
  cptr<int64_t> sfirst;     // [batch] first cold work item
  cptr<int64_t> mfirst;     // [batch] first mask word
  cptr<uint32_t> tab;       // [n][m_pad] records of H
  cptr<int32_t> blk;        // [nblk]
  cptr<int32_t> span;       // [nspan]
};

struct Item {
  DescView d;             // the stripe's own rows, the shared tables
  int64_t len, idx;       // its length; the item's column block (cold pass: span) within it
  int64_t word0, b;       // its first mask word; the stripe
};

// Work item w of `list`: the stripe moved into an SGPR, its rows, length and first word by scalar
// loads. Called at the top of the item loop, where the wave has reconverged.
__device__ __forceinline__ Item item(const ScrubView& a, cptr<int32_t> list, cptr<int64_t> first, int n, int64_t w) {
  const uint64_t b = uint32_t(sgpr_int(list[w]));
  const cptr<uint64_t> rows = a.in + b * uint64_t(n);
  return {{rows, rows, rows, a.tab}, a.len[b], w - first[b], a.mfirst[b], int64_t(b)};
}

// wave_or with the stripe word beside the block word: one ballot when the wave is clean, else one per
// row and two atomicOr from lane 0. Called with the whole wave converged.
template <int MT>
__device__ __forceinline__ void wave_or_both(uint32_t rowbits, int shift, int* mask, int64_t blk, int64_t stripe) {
  if (__builtin_amdgcn_ballot_w64(rowbits != 0) == 0) return;
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < MT; ++i)
    if (__builtin_amdgcn_ballot_w64(((rowbits >> i) & 1u) != 0) != 0) bits |= 1u << i;
  if ((threadIdx.x & 63u) == 0) {
    atomicOr(mask + blk, int(bits << shift));
    atomicOr(mask + stripe, int(bits << shift));
  }
}

template <int MT, bool IDENT>
__global__ __launch_bounds__(kBlock) void gf_varlen_syndrome_vec_kernel(ScrubView a, int n, int m_pad, int64_t nblk,
                                                                        int* mask, int64_t nwords, int bshift) {
  constexpr bool kPairs = MT <= 8;  // as gf_syndrome_vec_kernel
  const int nmul = IDENT ? n - MT : n;  // rows that are multiplied
  for (int64_t w = blockIdx.x; w < nblk; w += gridDim.x) {
    const Item it = item(a, a.blk, a.first, n, w);
    const DescView& d = it.d;
    const int64_t ngroups = it.len / 16;
    const int64_t tail = it.len % 16;
    const int64_t g = it.idx * kBlock + threadIdx.x;
    const int64_t word = it.word0 + wave_block(it.idx * kBlock + (threadIdx.x & ~63u), ngroups, bshift);
    for (int i0 = 0; i0 < m_pad; i0 += MT) {  // (IDENT: one tile)
      uint32_t rowbits = 0;
      if (g < ngroups) {
        const int64_t off = g * 16;
        uint32_t acc[MT][4];
        if constexpr (IDENT) {
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            const u32x4 x = ld16<true>(row_vec(d.in[nmul + i], off));
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = x[q];
          }
        } else {
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = 0;
        }
        u32x4 r0 = ld16<true>(row_vec(d.in[0], off));
        u32x4 r1 = nmul > 1 ? ld16<true>(row_vec(d.in[1], off)) : u32x4{0u, 0u, 0u, 0u};
        for (int j = 0; j < nmul; j += 2) {
          const u32x4 x0 = r0, x1 = r1;
          if (j + 2 < nmul) r0 = ld16<true>(row_vec(d.in[j + 2], off));
          if (j + 3 < nmul) r1 = ld16<true>(row_vec(d.in[j + 3], off));
          const auto t0 = d.tab + (size_t(j) * m_pad + i0) * kPermStride;
          const auto t1 = t0 + size_t(m_pad) * kPermStride;
          if (kPairs && j + 1 < nmul) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const Sel s0 = make_sel(x0[q]);
              const Sel s1 = make_sel(x1[q]);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[i][q] = mac_pair(acc[i][q], t0 + i * kPermStride, s0, t1 + i * kPermStride, s1);
            }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const Sel s0 = make_sel(x0[q]);
#pragma unroll
              for (int i = 0; i < MT; ++i) acc[i][q] = mac_map(acc[i][q], t0 + i * kPermStride, s0);
            }
            if (j + 1 < nmul) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const Sel s1 = make_sel(x1[q]);
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i][q] = mac_map(acc[i][q], t1 + i * kPermStride, s1);
              }
            }
          }
        }
        rowbits = group_bits<MT>(acc);
      } else if (g - ngroups < tail) {
        rowbits = syn_byte_bits<MT>(d, n, m_pad, i0, ngroups * 16 + (g - ngroups));
      }
      wave_or_both<MT>(rowbits, i0 & 16, mask, word, nwords + it.b);
    }
  }
}

// Byte form: one lane per byte column, rows of any alignment. A wave's 64 columns share a mask word.
template <int MT>
__global__ __launch_bounds__(kBlock) void gf_varlen_syndrome_byte_kernel(ScrubView a, int n, int m_pad, int64_t nblk,
                                                                         int* mask, int64_t nwords, int bshift) {
  for (int64_t w = blockIdx.x; w < nblk; w += gridDim.x) {
    const Item it = item(a, a.blk, a.first, n, w);
    const int64_t c = it.idx * kBlock + threadIdx.x;
    const int64_t c0 = it.idx * kBlock + (threadIdx.x & ~63u);
    const int64_t word = it.word0 + ((c0 < it.len ? c0 : 0) >> bshift);
    for (int i0 = 0; i0 < m_pad; i0 += MT) {
      const uint32_t rowbits = c < it.len ? syn_byte_bits<MT>(it.d, n, m_pad, i0, c) : 0u;
      wave_or_both<MT>(rowbits, i0 & 16, mask, word, nwords + it.b);
    }
  }
}

// gf_locate_kernel on span `idx` of the item's stripe; MT = pad_m(p), the one tile of the tables.
template <int MT>
__global__ __launch_bounds__(kBlock) void gf_varlen_locate_kernel(ScrubView a, int n, int p, int64_t nspan, int bshift,
                                                                  int span_shift, const int* mask, const uint8_t* loc,
                                                                  int locatable, int bytewise,
                                                                  unsigned long long* counts) {
  __shared__ LocLds l;
  for (int64_t w = blockIdx.x; w < nspan; w += gridDim.x) {
    const Item it = item(a, a.span, a.sfirst, n, w);
    const int64_t base = it.idx << span_shift;
    const Span span{base, std::min(base + (int64_t(1) << span_shift), it.len), true};
    if (mask[it.word0 + (base >> bshift)] == 0) continue;  // (uniform: before any barrier)
    __syncthreads();  // (a capped grid: the flush of this workgroup's last dirty item has read the histogram)
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
    sweep_span<MT>(it.d, n, span, bytewise != 0, [&](const uint32_t (&acc)[MT], int q, int64_t) {
      classify<MT>(l, l.hist, acc, q, n, p, locatable != 0, bad, unl);
    });
    if (unl) atomicAdd(&l.hist[n], unl);
    if (bad) atomicAdd(&l.hist[n + 1], bad);
    flush_bins(l.hist, n + 2, counts + uint64_t(it.b) * uint64_t(n + 2));
  }
}

// The mask cleared by a kernel: what clear_mask launches on a capturing stream.
__global__ __launch_bounds__(kBlock) void gf_varlen_clear_kernel(int* words, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) words[i] = 0;
}

// One hipMemsetAsync over the block words and the stripe words. On a stream that is being captured
// into a graph the same range is cleared by a kernel node instead: a memset node of this size came
// back from its SECOND replay holding one stale 16-byte pattern over the first 32 bytes of the mask
// (the words after them zero, the kernel's bits ORed on top; the first replay clean), while an 8-byte
// one (launch_gf_syndrome's, one stripe) replays correctly. The cause inside the runtime is supposed
// (the fill's pattern not kept with the node), not found; a kernel node carries its arguments itself.
inline hipError_t clear_mask(int32_t* mask, size_t words, hipStream_t stream) {
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) {
    (void)hipGetLastError();
    capturing = hipStreamCaptureStatusNone;
  }
  if (capturing != hipStreamCaptureStatusActive) return hipMemsetAsync(mask, 0, words * sizeof(int32_t), stream);
  if (words == 0) return hipSuccess;
  const unsigned grid = unsigned(std::min<size_t>((words + kBlock - 1) / kBlock, 1024));
  gf_varlen_clear_kernel<<<grid, kBlock, 0, stream>>>(mask, int64_t(words));
  return hipGetLastError();
}

// as gf_varlen.hip: at most 2^32 - 1 work-items along x, the kernels stride
constexpr int64_t kMaxFlatBlocks = int64_t(UINT32_MAX) / kBlock / 8 * 8;

inline unsigned flat_grid(int64_t items, int max_blocks) {
  return unsigned(std::min(items, max_blocks ? int64_t(max_blocks) : kMaxFlatBlocks));
}

inline ScrubView scrub_view(const void* desc, int n, int m_pad, int batch, int64_t nblk, int64_t nspan) {
  const VarlenScrubLayout l = varlen_scrub_layout(n, m_pad, batch, nblk, nspan);
  const char* base = static_cast<const char*>(desc);
  return {(cptr<uint64_t>)(base + l.in_off),        (cptr<int64_t>)(base + l.len_off),
          (cptr<int64_t>)(base + l.first_off),      (cptr<int64_t>)(base + l.span_first_off),
          (cptr<int64_t>)(base + l.mask_first_off), (cptr<uint32_t>)(base + l.tab_off),
          (cptr<int32_t>)(base + l.blk_off),        (cptr<int32_t>)(base + l.span_off)};
}

}  // namespace

hipError_t launch_gf_varlen_syndrome(const void* desc, int n, int m_pad, int ident, int batch, int64_t nblk,
                                     int64_t block_bytes, bool force_bytewise, int max_blocks, int32_t* mask,
                                     int64_t nwords, hipStream_t stream) {
  if (!desc || !mask || batch < 1 || !scrub_args_ok(n, m_pad, 0, block_bytes) || m_pad > 256 || ident < 0 ||
      ident > m_pad || ident >= n || nblk < 0 || nblk > int64_t(INT32_MAX) || nwords < 0 || max_blocks < 0)
    return hipErrorInvalidValue;
  // the block words and the stripe words: one allocation, one memset (clear_mask)
  const hipError_t e = clear_mask(mask, size_t(nwords) + size_t(batch), stream);
  if (e != hipSuccess || nblk == 0) return e;
  const int bshift = log2_exact(block_bytes);
  const ScrubView a = scrub_view(desc, n, m_pad, batch, nblk, 0);  // (the hot pass reads no span list)
  const unsigned grid = flat_grid(nblk, max_blocks);
  return dispatch_tile(tile_for(m_pad), [&](auto mt) -> hipError_t {
    constexpr int MT = decltype(mt)::value;
    constexpr bool kIdent = MT <= 8;  // (the 16-row tile has no registers for 16 more rows in flight)
    if (force_bytewise)
      gf_varlen_syndrome_byte_kernel<MT><<<grid, kBlock, 0, stream>>>(a, n, m_pad, nblk, mask, nwords, bshift);
    else if (kIdent && ident == MT && m_pad == MT)
      gf_varlen_syndrome_vec_kernel<MT, kIdent><<<grid, kBlock, 0, stream>>>(a, n, m_pad, nblk, mask, nwords, bshift);
    else
      gf_varlen_syndrome_vec_kernel<MT, false><<<grid, kBlock, 0, stream>>>(a, n, m_pad, nblk, mask, nwords, bshift);
    return hipGetLastError();
  });
}

hipError_t launch_gf_varlen_locate(const void* desc, int n, int p, int batch, int64_t nblk, int64_t nspan,
                                   int64_t block_bytes, bool force_bytewise, int max_blocks, const int32_t* mask,
                                   const uint8_t* loc, bool locatable, uint64_t* counts, hipStream_t stream) {
  if (!desc || !mask || !loc || !counts || batch < 1 || !locate_args_ok(n, p, 0, block_bytes) || nblk < 0 ||
      nblk > int64_t(INT32_MAX) || nspan < 0 || nspan > int64_t(INT32_MAX) || max_blocks < 0)
    return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(counts, 0, size_t(batch) * size_t(n + 2) * sizeof(uint64_t), stream);
  if (e != hipSuccess || nspan == 0) return e;
  const int bshift = log2_exact(block_bytes);
  const int span_shift = std::min(bshift, kLocSpanShift);
  const ScrubView a = scrub_view(desc, n, pad_m(p), batch, nblk, nspan);
  const unsigned grid = flat_grid(nspan, max_blocks);
  return dispatch_tile(pad_m(p), [&](auto mt) -> hipError_t {
    gf_varlen_locate_kernel<decltype(mt)::value><<<grid, kBlock, 0, stream>>>(
        a, n, p, nspan, bshift, span_shift, mask, loc, locatable ? 1 : 0, force_bytewise ? 1 : 0,
        reinterpret_cast<unsigned long long*>(counts));
    return hipGetLastError();
  });
}

}  // namespace gfrs
