// Launch entry points of the gfx950 HIP kernels (csrc/kernels/*.hip). Every launcher is
// asynchronous on `stream`, performs no allocation and no host synchronisation, so callers may
// capture it into a hipGraph (cdna_hip_programming.md Guideline 9).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace gfrs {

// ---- GF-GEMM (csrc/kernels/gf_gemm.hip) -------------------------------------------------------
// desc: device descriptor (gfrs/desc.h) for k inputs and m_pad outputs. Processes byte columns
// [col0, col0 + ncols). Uses the 16-byte v_perm kernel for the aligned body and a byte kernel for
// the ragged tail; `force_bytewise` routes everything through the byte kernel (unaligned rows).
// max_blocks caps grid.x (the reference's -p gridDim knob, src/main.c:74-77); 0 = uncapped.
// copies = false promises the descriptor has no fused-copy rows (an encode): k = 10 with 4-row
// output tiles then runs the rows-in-flight kernel (all k loads issued before the first multiply).
hipError_t launch_gf_gemm(const void* desc, int k, int m_pad, int64_t col0, int64_t ncols,
                          bool force_bytewise, int max_blocks, hipStream_t stream, bool copies = true);

// GF(2^16) form (csrc/kernels/gf_gemm16.hip): desc built with desc_layout16 (build_desc field_w =
// 16); rows hold little-endian 16-bit symbols, col0 and ncols are even byte counts. `symwise`
// routes every column through the one-symbol-per-lane kernel (rows not 16-byte aligned).
// one_tile: keep every output in one tile whatever the row length (the zero-copy pipeline, whose
// inputs cross PCIe once per tile; short rows otherwise run one output per tile).
hipError_t launch_gf_gemm16(const void* desc, int k, int m_pad, int64_t col0, int64_t ncols, bool symwise,
                            int max_blocks, hipStream_t stream, bool one_tile = false);
// batched: `batch` stripes (grid.y), desc built with desc_layout16(k, m_pad, batch)
hipError_t launch_gf_gemm16_batched(const void* desc, int k, int m_pad, int batch, int64_t col0, int64_t ncols,
                                    bool symwise, int max_blocks, hipStream_t stream, bool one_tile = false);

// Batched form: `batch` stripes of identical shape share the coefficient tables (small-object
// serving: one launch for many objects). desc built with desc_layout(k, m_pad, batch).
// copies = false promises no fused-copy rows (a batched encode: the rows-in-flight kernel may run).
hipError_t launch_gf_gemm_batched(const void* desc, int k, int m_pad, int batch, int64_t col0, int64_t ncols,
                                  bool force_bytewise, hipStream_t stream, bool copies = true);

// Variant selector for benchmarks/ablation: vec = 16-byte groups per lane (0 = byte kernel, -1 = the
// byte kernel's serial round-3 form),
// pf = input rows kept in flight per lane, nt = non-temporal loads/stores.
hipError_t launch_gf_gemm_variant(const void* desc, int k, int m_pad, int64_t col0, int64_t ncols,
                                  int vec, int pf, bool nt, int max_blocks, hipStream_t stream);

// LDS-LUT ablation (gf_gemm_lut.hip): the same GEMM with per-coefficient 4-bit nibble tables in LDS
// (two ds_read_u8 per byte product), built from the descriptor's tables; 16-byte aligned columns,
// the < 16-byte tail on the byte kernel.
hipError_t launch_gf_gemm_lut(const void* desc, int k, int m_pad, int64_t col0, int64_t ncols, hipStream_t stream);

// ---- scrub (csrc/kernels/gf_scrub.hip) ---------------------------------------------------------
// desc: a desc_layout(n, m_pad) descriptor whose inputs are the n stripe rows (natives first), whose
// tables are those of the parity-check matrix H = [E | I_p] (p x n, m_pad = pad_m(p)) and whose
// out_ptr entries are all 0. Computes the syndrome H . stripe over byte columns [0, ncols) without
// storing it and sets bit i % 32 of mask[b] when syndrome row i is nonzero anywhere in columns
// [b * block_bytes, (b + 1) * block_bytes); block_bytes is a power of two >= 4096 and mask holds
// ceil(ncols / block_bytes) words, zeroed here first. A consistent stripe stores nothing else.
// force_bytewise: rows that are not 16-byte aligned. Any n <= 256, any p. ident: H's last `ident`
// columns are promised to be the identity (p for H = [E | I_p], 0 for an arbitrary H): the
// rows-in-flight kernel of the narrow codes then XORs those rows in without a multiply.
hipError_t launch_gf_syndrome(const void* desc, int n, int m_pad, int ident, int64_t ncols, bool force_bytewise,
                              int64_t block_bytes, int32_t* mask, hipStream_t stream);
// Classifies every byte column of the column blocks whose mask word is nonzero (p <= 16; same desc).
// loc (device): H row-major (p x n bytes), then per column j its pivot row (first nonzero row, n
// bytes) and the inverse of that pivot (n bytes). counts (device, zeroed here first): votes[n],
// then the unlocated columns, then the inconsistent columns. A column with one nonzero syndrome
// byte s_i votes for parity chunk n - p + i; with several, for the native j with s == e . H[:, j],
// e = s_r / H[r][j], r = j's pivot row; otherwise (or when !locatable) it is unlocated.
hipError_t launch_gf_locate(const void* desc, int n, int p, int64_t ncols, bool force_bytewise, int64_t block_bytes,
                            const int32_t* mask, const uint8_t* loc, bool locatable, uint64_t* counts,
                            hipStream_t stream);
// Batched forms (small-object scrubbing: one launch for many stripes, grid.y = stripe): `batch` >= 1
// stripes of identical shape under one H. desc built with desc_layout(n, m_pad, batch): stripe b's
// rows are in_ptr[b * n + j], the tables are shared. mask holds batch rows of nmask = ceil(ncols /
// block_bytes) words (stripe b's at mask + b * nmask), zeroed here by one memset; counts holds batch
// rows of n + 2 (stripe b's at counts + b * (n + 2)), likewise. Every form of the single launchers
// runs per stripe (for (4, 6) and (10, 14) with ident == p the rows-in-flight kernel), and a
// consistent batch stores nothing but the memset. More than 65535 stripes (the grid.y limit) run as
// several launches of at most that many each. hipErrorInvalidValue with nothing written for
// batch < 1, a null desc and whatever the single launchers refuse.
hipError_t launch_gf_syndrome_batched(const void* desc, int n, int m_pad, int ident, int batch, int64_t ncols,
                                      bool force_bytewise, int64_t block_bytes, int32_t* mask, hipStream_t stream);
hipError_t launch_gf_locate_batched(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                                    int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                    uint64_t* counts, hipStream_t stream);

// ---- correct (csrc/kernels/gf_correct.hip) -----------------------------------------------------
// Error correction per byte column, in place, over the scrub descriptor, mask and loc operand above:
// every byte column of the column blocks whose mask word is nonzero gets the smallest repair that
// explains its syndrome s. A weight-1 column (s == e . H[:, j], any chunk j) has stripe[j][c] ^= e;
// otherwise, with max_errors == 2, the explanations s == e1 . H[:, j1] ^ e2 . H[:, j2] (j1 < j2,
// e1, e2 != 0) are counted over all pairs and exactly one is applied; any other column, and every
// bad column when !locatable, is uncorrectable and not written. Only the patched bytes of the
// named rows are stored. counts (device, zeroed here first): fixed_bytes[n] (bytes changed per
// chunk), then the weight-1 columns, the weight-2 columns, the uncorrectable columns and the
// inconsistent columns: n + 4 words. The rows must not overlap each other. hipErrorInvalidValue,
// with nothing written, for what launch_gf_locate refuses, a null desc, p < 2, max_errors outside
// {1, 2}, and max_errors == 2 with p < 4 or n > kCorrectMaxPairN (the pair search walks n^2 / 2
// pairs per column from log tables in LDS; max_errors == 1 works for any n <= 256).
constexpr int kCorrectMaxPairN = 64;
hipError_t launch_gf_correct(const void* desc, int n, int p, int64_t ncols, bool force_bytewise, int64_t block_bytes,
                             const int32_t* mask, const uint8_t* loc, bool locatable, int max_errors,
                             uint64_t* counts, hipStream_t stream);
// Batched form, as launch_gf_locate_batched: stripe b's counts at counts + b * (n + 4); more than
// 65535 stripes run as several launches.
hipError_t launch_gf_correct_batched(const void* desc, int n, int p, int batch, int64_t ncols, bool force_bytewise,
                                     int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                     int max_errors, uint64_t* counts, hipStream_t stream);

// ---- checked repair (csrc/kernels/gf_checked.hip) ----------------------------------------------
// Errors-and-erasures repair of a degraded stripe: e erased rows are rebuilt from the first
// k = ns - r of the ns survivors while the other r survivors check them, in one pass. desc: a
// desc_layout(ns, pad_m(e + r)) descriptor whose inputs are the ns survivor rows in ascending chunk
// order, whose out_ptr[0..e) are the erased rows (every other entry 0) and whose tables are those of
// T[:, S] ((e + r) x ns; T = inv(H[:, X + R]) . H: rows 0..e-1 rebuild, rows e..e+r-1 are [B | I_r]).
// launch_gf_checked stores out_i = T[i, S] . survivors for i < e over byte columns [0, ncols) and
// sets bit t of mask[b] when check row e + t is nonzero anywhere in column block b (mask zeroed here
// first, ceil(ncols / block_bytes) words). The erased rows are never read; a consistent stripe moves
// ns rows in, e rows out and nothing else. e = 0 only checks; r = 0 only rebuilds (mask stays zero).
// launch_gf_checked_fix (r >= 1) then runs launch_gf_correct's rule over the dirty blocks with the
// r x ns check matrix T[e:, S] on the survivors: loc = launch_gf_locate's operand for that matrix,
// followed by T[:e, S] row-major (e x ns bytes). A corrected survivor byte j gets ^= v and every
// erased row i ^= v . T[i][j]; an uncorrectable column is not written. counts (zeroed here first):
// fixed_bytes[ns] by survivor index, then weight-1, weight-2, uncorrectable and bad columns. No row
// may overlap another. hipErrorInvalidValue, with nothing written, for a null pointer, e < 0, r < 0,
// e + r outside [1, 16], r >= ns, ns > 256, a bad ncols or block_bytes (as launch_gf_syndrome), and in
// the fix launchers r < 1, max_errors outside {1, 2} and max_errors == 2 with r < 4 or
// ns > kCorrectMaxPairN. Batched forms: desc_layout(ns, pad_m(e + r), batch), stripe b's rows at
// in_ptr[b * ns + j] and out_ptr[b * pad_m(e + r) + i], one T for the batch, mask and counts rows
// per stripe as the scrub launchers; more than 65535 stripes run as several launches.
hipError_t launch_gf_checked(const void* desc, int ns, int e, int r, int64_t ncols, bool force_bytewise,
                             int64_t block_bytes, int32_t* mask, hipStream_t stream);
hipError_t launch_gf_checked_batched(const void* desc, int ns, int e, int r, int batch, int64_t ncols,
                                     bool force_bytewise, int64_t block_bytes, int32_t* mask, hipStream_t stream);
hipError_t launch_gf_checked_fix(const void* desc, int ns, int e, int r, int64_t ncols, bool force_bytewise,
                                 int64_t block_bytes, const int32_t* mask, const uint8_t* loc, bool locatable,
                                 int max_errors, uint64_t* counts, hipStream_t stream);
hipError_t launch_gf_checked_fix_batched(const void* desc, int ns, int e, int r, int batch, int64_t ncols,
                                         bool force_bytewise, int64_t block_bytes, const int32_t* mask,
                                         const uint8_t* loc, bool locatable, int max_errors, uint64_t* counts,
                                         hipStream_t stream);

// ---- in-place parity update (csrc/kernels/gf_update.hip) ---------------------------------------
// The parity of a stripe in which d natives changed, from those natives and the parity rows alone:
// over byte columns [col0, col0 + ncols), parity_i ^= XOR_t L[i][t](x_t) in place, with x_t =
// old_t ^ new_t (pairs) or x_t = delta_t (!pairs); store_new (pairs only) also overwrites old_t with
// new_t in the same pass (a write into an n-row stripe). desc: a desc_layout(d, m_pad) descriptor
// (gfrs/desc.h documents the reuse): in_ptr[t] = old_t or delta_t, copy_ptr[t] = new_t (0 in the
// delta form), out_ptr[i] = parity_i (0 = padding, skipped), tables of E[:, changed] (p x d), m_pad =
// pad_m(p) with any p in [1, 255]. One launch, one lane per 16-byte group walking every parity row;
// the ragged tail runs on extra lanes of the same launch. force_bytewise (rows not 16-byte aligned)
// or col0 % 16 != 0 takes the byte-per-lane form, the rule of launch_gf_gemm. Rows may be longer
// than 2^32 bytes. The parity rows must not overlap each other or any other row, and new_t must
// not overlap old_t: the read-modify-write is per lane. hipErrorInvalidValue, and nothing launched,
// for d outside [1, kUpdateMaxD] (callers split a longer list into passes: XOR accumulation makes
// them independent), an m_pad that pad_m does not produce, col0 < 0, ncols < 0, store_new without
// pairs, or a null desc; ncols == 0 succeeds without a launch.
constexpr int kUpdateMaxD = 8;  // 32 VGPRs of deltas per lane
hipError_t launch_gf_update(const void* desc, int d, int m_pad, int64_t col0, int64_t ncols, bool pairs,
                            bool store_new, bool force_bytewise, hipStream_t stream);
// `batch` stripes of one shape per launch (grid.y = stripe; more than 65,535 stripes run as several
// launches), each changing d natives of its own, for the small overwrites of a store of small
// objects. desc: an update_batch_layout(k, d, m_pad, batch) record (gfrs/desc.h): stripe b's rows at
// in_ptr[b*d + t], copy_ptr[b*d + t] and out_ptr[b*m_pad + i] (0 = padding, skipped), its native
// ids at ids[b*d + t], each in [0, k) and distinct within a stripe (the caller's duty: the kernel
// forms table addresses from them unchecked), and ONE table block tab[j][i] = the map of E[i][j] for
// all k natives, shared by the batch. Per stripe exactly launch_gf_update with the tables of
// E[:, ids[b]]; col0, ncols and the form are shared. force_bytewise (any row of any stripe not
// 16-byte aligned) or col0 % 16 != 0 puts the whole batch on the byte-per-lane form. No row written
// by one stripe may overlap any other row of the batch. hipErrorInvalidValue, and nothing launched,
// for a null desc, batch < 1, k outside [1, 256], and whatever launch_gf_update refuses; ncols == 0
// succeeds without a launch.
hipError_t launch_gf_update_batched(const void* desc, int k, int d, int m_pad, int batch, int64_t col0, int64_t ncols,
                                    bool pairs, bool store_new, bool force_bytewise, hipStream_t stream);

// ---- batched repair (csrc/kernels/gf_repair.hip) -----------------------------------------------
// `batch` stripes of one shape per launch (grid.y = stripe; more than 65,535 stripes run as several
// launches that advance in, out and pat and share the table block), each rewriting up to m_pad of its
// rows from k of its other rows under an erasure pattern of its own: over byte columns [0, ncols),
// out_i = XOR_j L_q[i][j](in_j) with q = pat[b]. desc: a repair_batch_layout(k, m_pad, batch, npat)
// record (gfrs/desc.h): stripe b's survivor rows at in_ptr[b*k + j], the rows it rewrites at
// out_ptr[b*m_pad + i] (0 = padding or fewer erasures than m_pad: never stored, and a tile of such rows
// is skipped), its pattern at pat[b], and npat table blocks tab[q][j][i] = the map of coeff_q[i][j],
// m_pad = pad_m(the most erasures of any pattern). pat[b] in [0, npat) is the caller's duty: it is
// device data, and the kernel forms the table address from it unchecked. One lane per 16-byte group,
// the ragged tail on extra lanes of the same launch; force_bytewise (any row of any stripe not
// 16-byte aligned) puts the whole batch on the byte-per-lane form. Rows may be longer than 2^32
// bytes and stripes further apart. No row written may overlap any other row the batch uses.
// hipErrorInvalidValue, and nothing launched, for a null desc, batch < 1, npat < 1, k outside
// [1, 256], an m_pad that pad_m does not produce or above 256, or ncols < 0; ncols == 0 succeeds
// without a launch.
hipError_t launch_gf_repair_batched(const void* desc, int k, int m_pad, int batch, int npat, int64_t ncols,
                                    bool force_bytewise, hipStream_t stream);

// ---- variable-length batch (csrc/kernels/gf_varlen.hip) -----------------------------------------
// launch_gf_repair_batched for `batch` stripes whose rows differ in length from stripe to stripe, in
// ONE launch on a flat grid of `nblk` (stripe, column block) work items: over byte columns
// [0, len[b]), out_i = XOR_j L_q[i][j](in_j) with q = pat[b]. desc: a varlen_layout(k, m_pad, batch,
// npat, nblk) record (gfrs/desc.h): in_ptr, out_ptr, pat and the table blocks as in
// repair_batch_layout, len[b] the row length of stripe b, first_blk the exclusive prefix sum of the
// stripes' block counts nb[b] = ceil((len[b] / 16 + len[b] % 16) / 256) (force_bytewise:
// ceil(len[b] / 256)), blk_stripe[w] the stripe of work item w, nblk = sum nb. A stripe of length 0
// has no work item. The arrays are device data and the caller's duty: the kernel forms addresses from
// blk_stripe[w] in [0, batch), pat[b] in [0, npat) and first_blk[b] <= w unchecked; a lane touches
// only columns below len[b]. force_bytewise (any row of any stripe not 16-byte aligned) puts the
// whole batch on the byte-per-lane form. max_blocks = 0: the default grid (one workgroup per work
// item up to the grid limit); nonzero: at most that many workgroups, which stride over the work
// items. No row written may overlap any other row the batch uses. hipErrorInvalidValue, and nothing
// launched, for a null desc, batch < 1, npat < 1, k outside [1, 256], an m_pad that pad_m does not
// produce or above 256, nblk < 0 or >= 2^31, or max_blocks < 0; nblk == 0 succeeds without a launch.
hipError_t launch_gf_varlen(const void* desc, int k, int m_pad, int batch, int npat, int64_t nblk, bool force_bytewise,
                            int max_blocks, hipStream_t stream);

// ---- variable-length scrub (csrc/kernels/gf_varlen_scrub.hip) ------------------------------------
// launch_gf_syndrome_batched / launch_gf_locate_batched for `batch` stripes whose rows differ in length
// from stripe to stripe, each pass ONE launch on a flat grid. desc: a varlen_scrub_layout(n, m_pad,
// batch, nblk, nspan) record (gfrs/desc.h): stripe b's n rows, len[b], the tables of H (m_pad =
// pad_m(p), shared), and per pass a work list: blk_stripe / first_blk over nblk (stripe, column block)
// items as launch_gf_varlen's (force_bytewise picks the byte-per-lane counts), span_stripe /
// first_span over nspan (stripe, span) items, ns[b] = ceil(len[b] / min(block_bytes, 16 KiB)); and
// mask_first[b], the exclusive prefix sum of ceil(len[b] / block_bytes). A stripe of length 0 has no
// item and no mask word. The arrays are device data and the caller's duty, read unchecked.
// mask: nwords = sum ceil(len[b] / block_bytes) block words, stripe b's from mask_first[b], each as
// launch_gf_syndrome defines it, then `batch` stripe words, word b the OR of stripe b's block words:
// one allocation, zeroed here by one memset (on a stream under graph capture: by a kernel node); a
// consistent batch stores nothing else. A work item walks
// every output tile of its columns, so any p up to 256 runs. ident as launch_gf_syndrome. max_blocks
// as launch_gf_varlen. hipErrorInvalidValue with nothing launched or written for a null desc or mask,
// batch < 1, n outside [1, 256], an m_pad that pad_m does not produce or above 256, ident outside
// [0, m_pad] or >= n, a block_bytes that is not a power of two >= 4096, nblk outside [0, 2^31),
// nwords < 0 or max_blocks < 0; nblk == 0 succeeds after the memset.
hipError_t launch_gf_varlen_syndrome(const void* desc, int n, int m_pad, int ident, int batch, int64_t nblk,
                                     int64_t block_bytes, bool force_bytewise, int max_blocks, int32_t* mask,
                                     int64_t nwords, hipStream_t stream);
// The cold pass over the same record and mask (p <= 16): every byte column of the spans whose block
// word is nonzero is classified as launch_gf_locate does, into counts + b * (n + 2), all zeroed here
// by one memset. Refused as above, and for a null loc or counts, p outside [1, 16] or >= n, and nspan
// outside [0, 2^31); nspan == 0 succeeds after the memset.
hipError_t launch_gf_varlen_locate(const void* desc, int n, int p, int batch, int64_t nblk, int64_t nspan,
                                   int64_t block_bytes, bool force_bytewise, int max_blocks, const int32_t* mask,
                                   const uint8_t* loc, bool locatable, uint64_t* counts, hipStream_t stream);

// ---- device-built repair coefficients (csrc/kernels/gf_repair_solve.hip) ------------------------
// Solves `npat` erasure patterns of one (n, k) GF(2^8) code in one launch, one workgroup each
// (grid.x = pattern): g = G (n x k, [I; E]) on the device, surv int32 [npat][k] the survivors of each
// pattern in the order of its coefficient columns, erased int32 [npat][m_pad] the rows to rewrite,
// padded with -1. Pattern q's rows G[erased_q] . inv(G[surv_q]) go to coeff + q * m_pad * k (m_pad x k
// bytes, zero rows where erased is -1) and, as v_perm records tab[q][j][i], to the q-th (k, m_pad)
// table block at `tab`: the table block of a repair_batch_layout descriptor, or with npat = 1 that of
// a desc_layout one. Either may be null. status[q] = 0 built, 1 singular, 2 invalid lists (an id
// outside [0, n), a survivor or an erased id listed twice, an erased id among the survivors); a
// pattern whose status is not 0 writes neither coefficients nor table words. hipErrorInvalidValue,
// and nothing launched, for npat < 0, k outside [1, n], n > 256, m_pad outside [1, 256], a null g,
// surv, erased or status, or a system that does not fit the LDS (repair_solve_lds_bytes above 64 KiB:
// none with n <= 256); npat == 0 succeeds without a launch and reads no pointer.
int64_t repair_solve_lds_bytes(int n, int k, int m_pad);  // -1: a shape the launcher refuses
hipError_t launch_gf_repair_solve(const uint8_t* g, int n, int k, const int* surv, const int* erased, int npat,
                                  int m_pad, uint8_t* coeff, void* tab, int* status, hipStream_t stream);

// ---- Gauss-Jordan inverse (csrc/kernels/gf_invert.hip)---------------------------------------
// Inverts `batch` n x n matrices (row-major, contiguous) with row pivoting, one workgroup each,
// [A|I] resident in LDS. status[b] = 0 ok, 1 singular. n <= 256.
// If `desc` is non-null, additionally writes the perm tables of rows `sel_rows[0..m)` of each
// inverse into desc's table block (k = n, m_pad given) — the decode GEMM then runs without a
// host round-trip. (batch must be 1 in that mode.)
// Systematic decode rows without the k x k inverse: g = G (n x k, [I; E]), rows = the k survivor
// ids, erased = the e erased native ids (device int32). Writes X (e x k, decode coefficients of the
// erased natives in survivor order) to dm (optional), status (1 = unrecoverable), and the v_perm
// tables tab[j][b] into desc (k inputs, m_pad >= e outputs) when given.
// Device-built plan (ptrs != null, desc required): `erased` becomes an OUTPUT (derived from rows on
// the device) and the descriptor's row pointers are written from ptrs = {chunk row 0..n_chunks-1,
// output row 0..k-1} (uint64 device addresses); status 2 = invalid pattern.
hipError_t launch_gf_decode_system(const uint8_t* g, int k, const int* rows, int* erased, int e, uint8_t* dm,
                                   int* status, void* desc, int m_pad, hipStream_t stream,
                                   const uint64_t* ptrs = nullptr, int n_chunks = 0);
hipError_t launch_gf_invert(const uint8_t* a, uint8_t* a_inv, int n, int batch, int* status,
                            void* desc, const int* sel_rows, int m, int m_pad, hipStream_t stream);

// GF(2^16) form (csrc/kernels/gf_decode16.hip): g = G (n x k little-endian uint16, [I; E]), rows =
// the k survivor ids (device int32). `erased` (device int32 [e]) is always an OUTPUT: the erased
// natives, ascending, derived from rows. Writes X (e x k uint16) to dm (optional), status (0 ok,
// 1 singular, 2 invalid survivor list) and, into a desc_layout16 descriptor (k inputs, m_pad >= e
// outputs), the four v_perm records per coefficient; with ptrs = {chunk row 0..n-1, output row
// 0..k-1} also the descriptor's row pointers. Systems that fit one workgroup's LDS
// (decode_system16_supported: e <= 256, ~ 8 e (e + k) + 4 n + 4 k bytes) are solved there in one
// launch; larger ones (e.g. k = 2000, e = 100, or any e > 256) by the blocked multi-workgroup solve
// (panels of pivot columns, row pivoting, rank-P updates over the chip), which needs a device
// `workspace` of decode_system16_workspace(n, k, e) bytes (-1: too large even for it: e past
// ~19 K). force_blocked takes the blocked solve for any size (tests). force_panel (tests) sets the
// blocked solve's panel width: 0 keeps the widest that fits the LDS (32 until e is about 2,200);
// 4, 8, 16 or 32 run that instantiation in the same workspace when it is no wider than the default.
// Any other value, a wider one, or a nonzero one for a system the one-workgroup kernel takes, is
// hipErrorInvalidValue with nothing launched.
bool decode_system16_supported(int n, int k, int e);
int64_t decode_system16_workspace(int n, int k, int e);
hipError_t launch_gf_decode_system16(const uint16_t* g, int n, int k, const int* rows, int* erased, int e,
                                     uint16_t* dm, int* status, void* desc, int m_pad, hipStream_t stream,
                                     const uint64_t* ptrs = nullptr, void* workspace = nullptr,
                                     bool force_blocked = false, int force_panel = 0);

// ---- matrix utilities (csrc/kernels/gf_matrix.hip) -------------------------------------------
// kind: 0 = reference Vandermonde, 1 = Cauchy. Writes the p x k block.
hipError_t launch_gen_matrix(uint8_t* e, int k, int p, int kind, hipStream_t stream);
// Build perm tables [k][m_pad] for an m x k coefficient matrix into desc's table block.
hipError_t launch_perm_tables(const uint8_t* coeff, int m, int k, void* desc, int m_pad,
                              hipStream_t stream);
// Deterministic counter-based random bytes (synthetic benchmark input), 16 B per lane stores.
hipError_t launch_fill_random(uint8_t* dst, int64_t bytes, uint64_t seed, hipStream_t stream);
// Gather an m x k sub-matrix: out[i][:] = g[rows[i]][:]  (decode system assembly on device).
hipError_t launch_gather_rows(const uint8_t* g, const int* rows, uint8_t* out, int m, int k,
                              hipStream_t stream);

// ---- int8-MFMA bit-matrix GF-GEMM (csrc/kernels/gf_mfma.hip) ----------------------------------
// Same contract as launch_gf_gemm but on matrix cores, any k; rows 4-byte aligned and col0 a
// multiple of 4 (a lane loads dwords; hipErrorInvalidValue otherwise, the caller keeps such a
// start on the v_perm kernel).
hipError_t launch_gf_gemm_mfma(const void* bitmat, const void* desc, int k, int m, int64_t col0,
                               int64_t ncols, hipStream_t stream);
size_t mfma_bitmat_bytes(int k, int m);

// ---- FP4 (e2m1) block-scaled MFMA bit-matrix GF-GEMM (csrc/kernels/gf_mfma_fp4.hip) ------------
// Rows must be 2-byte aligned; whole 256-column chunks run on the matrix cores, the remainder on
// the v_perm kernel (desc must carry the perm tables too).
// mg_cap bounds the M-tiles (4 output rows each) one block keeps in LDS/accumulators; the bitmat
// must be built with the same cap. in_stride != 0 promises input row j == input row 0 + j*in_stride
// (rows of one allocation): DMA addresses are then computed, in 64 bits, instead of read from a
// pointer table. Any non-zero stride holds: negative (rows listed in reverse) or shorter than the
// rows (overlapping views). Rows may be longer than 2^32 bytes, and col0 anywhere in them.
// copies: also write input row j to the descriptor's copy[j] (fused survivor copy of decode).
hipError_t launch_gf_gemm_fp4(const void* bitmat, const void* desc, int k, int m, int64_t col0,
                              int64_t ncols, int mg_cap, int64_t in_stride, bool copies, hipStream_t stream);
size_t fp4_bitmat_bytes(int k, int m, int mg_cap);
// the form launch_gf_gemm_fp4 runs for (k, m, copies): "v1", "ar" or "tm" (fp4_route,
// gf_mfma_fp4.hip, documents each choice with its measurement)
const char* fp4_route_name(int k, int m, bool copies, int mg_cap);
// Batched form (small-object serving): `batch` stripes of identical shape whose rows sit at fixed
// strides — stripe b's input rows are stripe 0's + b * in_bstride, its output and copy rows stripe
// 0's + b * out_bstride (desc built with desc_layout(k, m_pad, batch); the kernel reads stripe 0's
// tables). ncols per stripe; whole chunks of every stripe run in ONE persistent matrix-core launch
// (A loaded once per wave for the whole batch), the ragged remainders on the batched v_perm kernel.
// hipErrorNotSupported when the shape has no batched matrix-core form (currently the A-resident
// kernel: k in (112, 128], one M-tile group), so the caller keeps the v_perm path.
hipError_t launch_gf_gemm_fp4_batched(const void* bitmat, const void* desc, int k, int m, int batch, int64_t col0,
                                      int64_t ncols, int mg_cap, int64_t in_stride, int64_t in_bstride,
                                      int64_t out_bstride, bool copies, hipStream_t stream);
hipError_t launch_fp4_bitmat(const uint8_t* coeff, int m, int k, void* bitmat, int mg_cap, hipStream_t stream);
// row o of the coefficient matrix = coeff + sel[o] * ld (device pointers; e.g. erased rows of a
// device-computed inverse, so a decode needs no host round trip)
hipError_t launch_fp4_bitmat_sel(const uint8_t* coeff, int ld, const int* sel, int m, int k, void* bitmat, int mg_cap,
                                 hipStream_t stream);
hipError_t launch_mfma_bitmat(const uint8_t* coeff, int m, int k, void* bitmat,
                              hipStream_t stream);

// ---- GF(2^16) on the FP4 matrix cores (csrc/kernels/gf_mfma16.hip) -----------------------------
// desc: a desc_layout16 descriptor (its v_perm records run the columns past the last 512-byte chunk
// and any start not 4-byte aligned); bitmat from launch_fp16_bitmat with the same (k, m, mg_cap).
// Rows 4-byte aligned; col0 / ncols even. K is split into passes (one launch each, later passes XOR
// into the outputs); copies: fused survivor copy (decode), in_stride as launch_gf_gemm_fp4: the
// computed-address form (32-bit lane offsets over 8 rows) serves strides of 128 .. 2^28 bytes, any
// other stride runs on the row pointers like in_stride = 0. Rows longer than 2^32 bytes and any
// col0 in them are addressed in 64 bits on both forms.
hipError_t launch_gf_gemm16_fp4(const void* bitmat, const void* desc, int k, int m, int64_t col0, int64_t ncols,
                                int mg_cap, int64_t in_stride, bool copies, hipStream_t stream);
// Batched: `batch` stripes whose rows are stripe 0's plus b * in_bstride (inputs) / b * out_bstride
// (outputs, copies), desc built with desc_layout16(k, m_pad, batch). Every stripe's whole chunks run
// in one persistent launch per K pass; the ragged remainders on the batched v_perm kernel.
hipError_t launch_gf_gemm16_fp4_batched(const void* bitmat, const void* desc, int k, int m, int batch, int64_t col0,
                                        int64_t ncols, int mg_cap, int64_t in_stride, int64_t in_bstride,
                                        int64_t out_bstride, bool copies, hipStream_t stream);
size_t fp16_bitmat_bytes(int k, int m, int mg_cap);
// coefficient (o, i) = coeff[row(o) * ld + i] (uint16, device), row(o) = sel ? sel[o] : o
hipError_t launch_fp16_bitmat(const uint16_t* coeff, int ld, const int* sel, int m, int k, void* bitmat, int mg_cap,
                              hipStream_t stream);

// FP4 kernels: the bit-matrix allocation ends with a write-only sink of kFp4SinkSlots 1-KiB slots;
// each wave stores its dummy / destination-less bytes into slot (4 * block + wave) % slots, so the
// sink writes of concurrent waves land on different L2 lines (one shared 1-KiB sink made every CU of
// an XCD queue on the same L2 channel). Nothing reads it.
constexpr int kFp4SinkSlots = 256;

// ---- FP4 A-resident form (csrc/kernels/gf_mfma_fp4ar.hip; called by launch_gf_gemm_fp4) ---------
// k in (112, 128], one bitmat group of mg <= 8 M-tiles (the layout launch_fp4_bitmat builds).
// Processes the leading whole chunks of [col0, col0 + ncols) and reports how many columns in
// *done (the caller finishes the rest).
struct Fp4ArLaunch {
  const uint64_t* in;    // descriptor in_ptr[k]
  const uint64_t* out;   // descriptor out_ptr[m_pad]
  const uint64_t* copy;  // descriptor copy_ptr[k] (nullptr: no fused copy)
  const void* bitmat;
  int k, m, mg;
  int64_t col0, ncols, in_stride;
  // batched launch: `batch` stripes whose rows are stripe 0's (the tables above) plus b * in_bstride
  // (inputs) / b * out_bstride (outputs and copies); ncols is per stripe, *done per stripe
  int batch = 1;
  int64_t in_bstride = 0, out_bstride = 0;
};
bool fp4ar_supported(int k, int mg);
hipError_t launch_gf_gemm_fp4ar(const Fp4ArLaunch& a, int64_t* done, hipStream_t stream);
// Tile-major form (csrc/kernels/gf_mfma_fp4tm.hip): same launch record (batch must be 1), k in
// (112, 128] with one group of 5..8 M-tiles; the chunk's B operand resident
// in AGPRs, tiles in pairs.
bool fp4tm_supported(int k, int mg, bool copies);
hipError_t launch_gf_gemm_fp4tm(const Fp4ArLaunch& a, int64_t* done, hipStream_t stream);

}  // namespace gfrs
