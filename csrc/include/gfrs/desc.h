// Device-resident GF-GEMM descriptor shared by the host runtime and the HIP kernels.
//
// A "GF-GEMM" computes, over a byte-column range [c0, c0+ncols):
//     out[i][c] = XOR_j  coeff[i][j] * in[j][c]        i in [0,m), j in [0,k)
// and optionally copies in[j][c] -> copy[j][c] while streaming (fused survivor copy of decode).
// Rows are addressed through pointer arrays so native chunks, parity chunks and decode survivors
// may live in separate allocations (the reference instead copies every row into one staging
// buffer, src/encode.cu:389-398, src/decode.cu:149-170).
//
// Layout (all offsets from the descriptor base, 32-byte aligned records):
//   [0,  16)              header {k, m, m_pad, batch}
//   [16, 16+8k)           in_ptr[k]      (uint64 device addresses)
//   [.., +8k)             copy_ptr[k]    (0 = no copy)
//   [.., +8*m_pad)        out_ptr[m_pad] (0 = padding row, never stored)
//   align 32, [.., +32*k*m_pad)   PermTable tab[k][m_pad]
//
// The in-place parity update (csrc/kernels/gf_update.hip) reuses the record as desc_layout(d, m_pad)
// for d changed natives and p parity rows: in_ptr[t] = old_t (or delta_t in the delta form),
// copy_ptr[t] = new_t (0 in the delta form; read, not written), out_ptr[i] = parity_i (read and
// written in place; 0 = padding row, skipped), tab[t][i] = the map of E[i][changed[t]].
//
// The batched update (`batch` stripes per launch, each changing d natives of its own) has a record
// of its own, update_batch_layout(k, d, m_pad, batch): the same header {k, d, m_pad, batch}, then
//   in_ptr[batch * d]        stripe b's old_t (delta_t) at [b*d + t]
//   copy_ptr[batch * d]      new_t (0 in the delta form; read, not written)
//   out_ptr[batch * m_pad]   parity_i at [b*m_pad + i] (0 = padding row, skipped)
//   ids[batch * d]           int32, ids[b*d + t] in [0, k): the native that row t of stripe b is
//   align 32, tab[k][m_pad]  the maps of the WHOLE code, tab[j][i] = the map of E[i][j], shared by
//                            every stripe; row t of stripe b uses tab[ids[b*d + t]][.]
#pragma once

#include <cstdint>
#include <cstddef>

#include "gfrs/gf256.h"

namespace gfrs {

struct DescHeader {
  int32_t k;
  int32_t m;
  int32_t m_pad;
  int32_t batch;
};

struct DescLayout {
  size_t in_off, copy_off, out_off, tab_off, bytes;
};

constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// `batch` stripes share one table block; stripe b's pointers are in[b*k + j], copy[b*k + j],
// out[b*m_pad + i] (batched small-object encode/decode in one launch).
constexpr DescLayout desc_layout(int k, int m_pad, int batch = 1) {
  DescLayout l{};
  l.in_off = sizeof(DescHeader);
  l.copy_off = l.in_off + 8 * size_t(k) * size_t(batch);
  l.out_off = l.copy_off + 8 * size_t(k) * size_t(batch);
  l.tab_off = align_up(l.out_off + 8 * size_t(m_pad) * size_t(batch), 32);
  l.bytes = l.tab_off + sizeof(PermTable) * size_t(k) * size_t(m_pad);
  return l;
}

// Batched in-place parity update (csrc/kernels/gf_update.hip): d changed rows per stripe, their
// native ids per stripe, and one table block of all k natives (the header comment has the record).
struct UpdateBatchLayout {
  size_t in_off, copy_off, out_off, ids_off, tab_off, bytes;
};
constexpr UpdateBatchLayout update_batch_layout(int k, int d, int m_pad, int batch) {
  UpdateBatchLayout l{};
  l.in_off = sizeof(DescHeader);
  l.copy_off = l.in_off + 8 * size_t(d) * size_t(batch);
  l.out_off = l.copy_off + 8 * size_t(d) * size_t(batch);
  l.ids_off = l.out_off + 8 * size_t(m_pad) * size_t(batch);
  l.tab_off = align_up(l.ids_off + 4 * size_t(d) * size_t(batch), 32);
  l.bytes = l.tab_off + sizeof(PermTable) * size_t(k) * size_t(m_pad);
  return l;
}

// Batched repair (csrc/kernels/gf_repair.hip): `batch` stripes per launch, each with an erasure
// pattern of its own out of `npat` distinct ones, so the coefficient tables differ per stripe:
//   header {k, m_pad, batch, npat}
//   in_ptr [batch * k]       stripe b's k survivor rows, in the order of its pattern's coefficient columns
//   out_ptr[batch * m_pad]   the rows stripe b rewrites (0 = padding / fewer erasures than m_pad: skipped)
//   pat    [batch]           int32, pat[b] in [0, npat): the pattern of stripe b
//   align 32, tab[npat][k][m_pad]   PermTable records, tab[q][j][i] = the map of coeff_q[i][j]; rows i >= e_q are zero
// The host resolves survivor and erased chunk ids into row addresses: the kernel needs no chunk ids,
// only pat[b], from which it forms its table block tab + pat[b] * k * m_pad records.
struct RepairBatchLayout {
  size_t in_off, out_off, pat_off, tab_off, bytes;
};
constexpr RepairBatchLayout repair_batch_layout(int k, int m_pad, int batch, int npat) {
  RepairBatchLayout l{};
  l.in_off = sizeof(DescHeader);
  l.out_off = l.in_off + 8 * size_t(k) * size_t(batch);
  l.pat_off = l.out_off + 8 * size_t(m_pad) * size_t(batch);
  l.tab_off = align_up(l.pat_off + 4 * size_t(batch), 32);
  l.bytes = l.tab_off + sizeof(PermTable) * size_t(npat) * size_t(k) * size_t(m_pad);
  return l;
}

// Variable-length batch (csrc/kernels/gf_varlen.hip): repair_batch_layout's record for stripes whose
// rows differ in length from stripe to stripe, run on a flat grid of `nblk` (stripe, column block)
// work items:
//   header {k, m_pad, batch, npat}
//   in_ptr   [batch * k]      as repair_batch_layout
//   out_ptr  [batch * m_pad]  as repair_batch_layout
//   len      [batch]          int64: the row length of stripe b (0: the stripe has no work item)
//   first_blk[batch]          int64: the exclusive prefix sum of the stripes' block counts
//   pat      [batch]          int32, pat[b] in [0, npat)
//   blk_stripe[nblk]          int32: the stripe of work item w; item w is column block
//                             w - first_blk[blk_stripe[w]] of that stripe
//   align 32, tab[npat][k][m_pad]   as repair_batch_layout
// The 8-byte arrays come first so that each array is aligned to its element.
struct VarlenLayout {
  size_t in_off, out_off, len_off, first_off, pat_off, blk_off, tab_off, bytes;
};
constexpr VarlenLayout varlen_layout(int k, int m_pad, int batch, int npat, int64_t nblk) {
  VarlenLayout l{};
  l.in_off = sizeof(DescHeader);
  l.out_off = l.in_off + 8 * size_t(k) * size_t(batch);
  l.len_off = l.out_off + 8 * size_t(m_pad) * size_t(batch);
  l.first_off = l.len_off + 8 * size_t(batch);
  l.pat_off = l.first_off + 8 * size_t(batch);
  l.blk_off = l.pat_off + 4 * size_t(batch);
  l.tab_off = align_up(l.blk_off + 4 * size_t(nblk), 32);
  l.bytes = l.tab_off + sizeof(PermTable) * size_t(npat) * size_t(k) * size_t(m_pad);
  return l;
}

// Variable-length scrub (csrc/kernels/gf_varlen_scrub.hip): the n rows of `batch` stripes of differing
// lengths, the tables of the check matrix H (shared, no patterns, no outputs) and two flat work lists:
// `nblk` (stripe, column block) items of the hot pass, as varlen_layout's, and `nspan` (stripe, span)
// items of the cold pass, a span being min(block_bytes, 16 KiB) columns:
//   header {n, m_pad, batch, 0}
//   in_ptr    [batch * n]   stripe b's rows at [b*n + j], natives first
//   len       [batch]       int64: the row length of stripe b (0: no work item of either kind)
//   first_blk [batch]       int64: the exclusive prefix sum of the stripes' block counts
//   first_span[batch]       int64: the exclusive prefix sum of the stripes' span counts
//   mask_first[batch]       int64: the exclusive prefix sum of ceil(len / block_bytes): stripe b's
//                           first word in the mask
//   align 32, tab[n][m_pad] PermTable records of H, tab[j][i] = the map of H[i][j]
//   blk_stripe [nblk]       int32: the stripe of hot work item w
//   span_stripe[nspan]      int32: the stripe of cold work item w
// The tables stand before the two lists so that neither pass needs the other's item count to find them.
struct VarlenScrubLayout {
  size_t in_off, len_off, first_off, span_first_off, mask_first_off, tab_off, blk_off, span_off, bytes;
};
constexpr VarlenScrubLayout varlen_scrub_layout(int n, int m_pad, int batch, int64_t nblk, int64_t nspan) {
  VarlenScrubLayout l{};
  l.in_off = sizeof(DescHeader);
  l.len_off = l.in_off + 8 * size_t(n) * size_t(batch);
  l.first_off = l.len_off + 8 * size_t(batch);
  l.span_first_off = l.first_off + 8 * size_t(batch);
  l.mask_first_off = l.span_first_off + 8 * size_t(batch);
  l.tab_off = align_up(l.mask_first_off + 8 * size_t(batch), 32);
  l.blk_off = l.tab_off + sizeof(PermTable) * size_t(n) * size_t(m_pad);
  l.span_off = l.blk_off + 4 * size_t(nblk);
  l.bytes = l.span_off + 4 * size_t(nspan);
  return l;
}

// GF(2^16) descriptor (csrc/kernels/gf_gemm16.hip): the same header and pointer arrays (rows are
// byte rows holding little-endian 16-bit symbols), and FOUR records per coefficient, tab[j][i][q]
// with q = 2 * src_byte + dst_byte (gfrs/gf65536.h perm_quad).
constexpr DescLayout desc_layout16(int k, int m_pad, int batch = 1) {
  DescLayout l = desc_layout(k, m_pad, batch);
  l.bytes = l.tab_off + 4 * sizeof(PermTable) * size_t(k) * size_t(m_pad);
  return l;
}

// Output tile (outputs computed per thread). Tiles are powers of two; m is padded to a multiple.
constexpr int kMaxTile = 16;
constexpr int tile_for(int m) {
  int t = 1;
  while (t < m && t < kMaxTile) t <<= 1;
  return t;
}
constexpr int pad_m(int m) {
  const int t = tile_for(m);
  return (m + t - 1) / t * t;
}

}  // namespace gfrs
