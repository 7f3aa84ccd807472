"""Variable-length batches (``csrc/kernels/gf_varlen.hip``): B stripes of one code per launch, each
with a row length of its own and an erasure pattern of its own.

The batched repair (:mod:`~gpu_rscode_amd.ops.repair`) launches a ``(column blocks, stripe)`` grid for
stripes of one shape. With mixed lengths that grid would be ``B x blocks(longest)`` workgroups of which
most exit at once, so this kernel runs a flat grid over a work list of (stripe, column block) pairs:
:func:`varlen_blocks` builds the list with numpy (no loop over stripes), :func:`build_varlen_desc`
lays it out behind the row pointers, and :class:`VarlenPlan` holds the uploaded record. An encode is
the one-pattern case: survivors ``0..k-1``, "erased" ``k..n-1``, coefficients ``E``.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import hip
from .gemm import pad_m, perm_tables_from_coeff, plan_stream, ready_event
from .repair import repair_rows, repair_tables
from .scrub import MAX_LOCATE_P, BatchScrubReport, check_block_bytes, locate_table, make_batch_report
from .update import check_overlap_batch

GROUP = 16   # bytes a lane of the vector form owns
BLOCK = 256  # lanes per workgroup
MAX_BLOCKS = 2 ** 31 - 1  # work items per launch
LOCATE_SPAN = 1 << 14  # columns a workgroup of the cold scrub pass covers, at most


def varlen_layout(k: int, m_pad: int, batch: int, npat: int, nblk: int) -> dict:
    """Mirror of ``gfrs::varlen_layout`` (``csrc/include/gfrs/desc.h``); a test pins the two equal."""
    in_off = 16
    out_off = in_off + 8 * k * batch
    len_off = out_off + 8 * m_pad * batch
    first_off = len_off + 8 * batch
    pat_off = first_off + 8 * batch
    blk_off = pat_off + 4 * batch
    tab_off = (blk_off + 4 * nblk + 31) // 32 * 32
    return dict(in_off=in_off, out_off=out_off, len_off=len_off, first_off=first_off, pat_off=pat_off,
                blk_off=blk_off, tab_off=tab_off, bytes=tab_off + 32 * npat * k * m_pad)


def varlen_blocks(lengths, bytewise: bool) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The flat work list of a batch with row lengths ``lengths`` (int ``[B]``, each >= 0): ``nb`` int64
    ``[B]``, the workgroups stripe b needs (vector form: one lane per 16-byte group and one per byte
    of the ragged tail; byte form: one lane per byte; 256 lanes per workgroup; none for a stripe of
    length 0), ``first_blk`` int64 ``[B]``, the exclusive prefix sum of ``nb``, and ``blk_stripe`` int32
    ``[sum(nb)]``, the stripe of each work item: work item w is column block ``w - first_blk[b]`` of
    stripe ``b = blk_stripe[w]``. numpy only: no loop over stripes."""
    n = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 0:
        raise ValueError("row lengths must not be negative")
    lanes = n if bytewise else n // GROUP + n % GROUP
    nb = (lanes + BLOCK - 1) // BLOCK
    ends = np.cumsum(nb)
    first = ends - nb
    total = int(ends[-1]) if n.size else 0
    if total > MAX_BLOCKS:
        raise ValueError(f"the batch needs {total} workgroups, more than one launch takes ({MAX_BLOCKS})")
    if n.size > MAX_BLOCKS:
        raise ValueError(f"{n.size} stripes, more than one launch takes")
    blk = np.repeat(np.arange(n.size, dtype=np.int32), nb)
    return nb, first, blk


def build_varlen_desc(in_ptrs: np.ndarray, out_ptrs: np.ndarray, pat: np.ndarray, lengths: np.ndarray,
                      first_blk: np.ndarray, blk_stripe: np.ndarray, tables: np.ndarray) -> np.ndarray:
    """Descriptor bytes of one variable-length launch: ``in_ptrs`` uint64 ``[B, k]`` survivor row
    addresses, ``out_ptrs`` uint64 ``[B, m_pad]`` addresses of the rows to rewrite (0 = none), ``pat`` int
    ``[B]`` in ``[0, npat)``, ``lengths`` int ``[B]``, ``first_blk`` / ``blk_stripe`` from
    :func:`varlen_blocks`, ``tables`` the ``(npat, k, m_pad, 8)`` uint32 v_perm records."""
    batch, k = in_ptrs.shape
    npat, _, mp = (int(v) for v in tables.shape[:3])
    lay = varlen_layout(k, mp, batch, npat, int(blk_stripe.size))
    buf = np.zeros(lay["bytes"], dtype=np.uint8)

    def put(off, a, dt):
        raw = np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8)
        buf[off: off + raw.size] = raw

    put(0, np.array([k, mp, batch, npat]), "<i4")
    put(lay["in_off"], in_ptrs, "<u8")
    put(lay["out_off"], out_ptrs, "<u8")
    put(lay["len_off"], lengths, "<i8")
    put(lay["first_off"], first_blk, "<i8")
    put(lay["pat_off"], pat, "<i4")
    put(lay["blk_off"], blk_stripe, "<i4")
    put(lay["tab_off"], tables, "<u4")
    return buf


def check_varlen_overlap(ins: np.ndarray, outs: np.ndarray, lengths: np.ndarray) -> None:
    """The aliasing rule of a variable-length batch through
    :func:`~gpu_rscode_amd.ops.update.check_overlap_batch`: no written row may overlap any other row any
    stripe of the batch uses (which also refuses a stripe listed twice with something to write), each
    row counted with its own stripe's length; rows only read may alias. Padding entries (address 0)
    and the rows of a stripe of length 0 are rows of no bytes."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1, 1)
    try:
        check_overlap_batch(outs, ins, None, [np.where(outs != 0, n, 0), np.broadcast_to(n, ins.shape)])
    except ValueError as e:
        raise ValueError(f"a row to write overlaps another row the batch uses: the kernel works in place and "
                         f"needs disjoint rows ({e})") from None


class VarlenPlan:
    """A reusable device encode or in-place repair of B stripes of differing lengths in one launch. As
    :class:`~gpu_rscode_amd.ops.repair.BatchRepairPlan` it keeps raw row addresses only, so a cache may
    hand it out only for the caller's live tensors.

    Args:
        ptrs: uint64 ``[B, n]``: the row addresses of the stripes (device memory of ``device``).
        lengths: int ``[B]``: stripe b's row length in bytes, >= 0.
        pat: int ``[B]``: the pattern of stripe b; -1 = the stripe is not touched (it is dropped from
            the launch, so its rows are never read).
        patterns: ``patterns[q] = (survivors_q, erased_q, coeff_q)`` as
            :class:`~gpu_rscode_amd.ops.repair.BatchRepairPlan` takes them (host coefficients or maps).
        device: the GPU the rows live on.
        check: run the aliasing check (:func:`check_varlen_overlap`); False when the caller has.
        force_bytewise: take the byte-per-lane form even when every row is 16-byte aligned.
    """

    def __init__(self, ptrs: np.ndarray, lengths, pat, patterns, device, *, check: bool = True,
                 force_bytewise: bool = False):
        ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
        if ptrs.ndim != 2:
            raise ValueError("ptrs must be a [B, n] array of row addresses")
        nstripes, n = ptrs.shape
        lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        pat = np.asarray(pat, dtype=np.int64).reshape(-1)
        if lengths.shape[0] != nstripes or pat.shape[0] != nstripes:
            raise ValueError(f"{nstripes} stripes but {lengths.shape[0]} lengths and {pat.shape[0]} pattern indices")
        if lengths.size and lengths.min() < 0:
            raise ValueError("row lengths must not be negative")
        patterns = [(tuple(int(s) for s in sv), tuple(int(e) for e in er), co) for sv, er, co in patterns]
        if not patterns:
            raise ValueError("VarlenPlan needs at least one pattern")
        if pat.size and (pat.min() < -1 or pat.max() >= len(patterns)):
            raise ValueError(f"pattern indices must lie in [-1, {len(patterns)})")
        self.k = len(patterns[0][0])
        for q, (sv, er, _) in enumerate(patterns):
            ids = sv + er
            if len(sv) != self.k or not er or len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= n:
                raise ValueError(f"pattern {q}: need {self.k} survivor ids and 1.. erased ids, distinct, in [0, {n})")
        if not 1 <= self.k <= 256 or max(len(er) for _, er, _ in patterns) > 256:
            raise ValueError("VarlenPlan supports 1 <= k <= 256 and at most 256 erasures")
        self.device = torch.device(device)
        self.npat = len(patterns)
        self.m_pad = pad_m(max(len(er) for _, er, _ in patterns))
        keep = pat >= 0
        self.batch = int(keep.sum())
        self.bytewise, self.desc, self._ready, self.nblk = False, None, None, 0
        self.lengths = lengths[keep]
        if not self.batch or not self.lengths.any():
            return
        if self.device.type != "cuda":
            raise ValueError("VarlenPlan runs on a GPU")
        ins, outs = repair_rows(ptrs[keep], pat[keep], patterns, self.m_pad)
        if check:
            check_varlen_overlap(ins, outs, self.lengths)
        # one unaligned row of some bytes: the whole batch bytewise (a padding entry, 0, is aligned)
        live = (self.lengths > 0)[:, None]
        self.bytewise = bool(force_bytewise or ((ins % np.uint64(16) != 0) & live).any()
                             or ((outs % np.uint64(16) != 0) & live).any())
        _, first, blk = varlen_blocks(self.lengths, self.bytewise)
        self.nblk = int(blk.size)
        host = build_varlen_desc(ins, outs, pat[keep], self.lengths, first, blk,
                                 repair_tables(patterns, self.k, self.m_pad))
        self.desc = torch.from_numpy(host).to(self.device)
        self._ready = ready_event(self.device)

    def run(self, stream: torch.cuda.Stream | None = None, max_blocks: int = 0) -> None:
        """Launch over the whole rows on ``stream`` (default: the current stream). No host sync.
        ``max_blocks``: 0 = one workgroup per work item; else at most that many, which stride."""
        if not self.nblk:
            return
        st = plan_stream(self, stream)
        if stream is not None:
            self.desc.record_stream(stream)
        hip().varlen(int(self.desc.data_ptr()), self.k, self.m_pad, self.batch, self.npat, self.nblk, self.bytewise,
                     int(max_blocks), st.cuda_stream)


# ---- scrub (``csrc/kernels/gf_varlen_scrub.hip``) ----------------------------------------------------
def varlen_scrub_layout(n: int, m_pad: int, batch: int, nblk: int, nspan: int) -> dict:
    """Mirror of ``gfrs::varlen_scrub_layout`` (``csrc/include/gfrs/desc.h``); a test pins the two equal."""
    in_off = 16
    len_off = in_off + 8 * n * batch
    first_off = len_off + 8 * batch
    span_first_off = first_off + 8 * batch
    mask_first_off = span_first_off + 8 * batch
    tab_off = (mask_first_off + 8 * batch + 31) // 32 * 32
    blk_off = tab_off + 32 * n * m_pad
    span_off = blk_off + 4 * nblk
    return dict(in_off=in_off, len_off=len_off, first_off=first_off, span_first_off=span_first_off,
                mask_first_off=mask_first_off, tab_off=tab_off, blk_off=blk_off, span_off=span_off,
                bytes=span_off + 4 * nspan)


def varlen_spans(lengths, block_bytes: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The work list of the cold scrub pass, built as :func:`varlen_blocks` builds the hot one: ``ns``
    int64 ``[B]``, the spans of ``min(block_bytes, 16 KiB)`` columns stripe b has, ``first_span`` int64
    ``[B]``, the exclusive prefix sum of ``ns``, and ``span_stripe`` int32 ``[sum(ns)]``, the stripe of each
    work item: item w is span ``w - first_span[b]`` of stripe ``b = span_stripe[w]``."""
    n = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 0:
        raise ValueError("row lengths must not be negative")
    span = min(check_block_bytes(block_bytes), LOCATE_SPAN)
    ns = (n + span - 1) // span
    ends = np.cumsum(ns)
    total = int(ends[-1]) if n.size else 0
    if total > MAX_BLOCKS:
        raise ValueError(f"the batch has {total} spans, more than one launch takes ({MAX_BLOCKS})")
    return ns, ends - ns, np.repeat(np.arange(n.size, dtype=np.int32), ns)


def mask_offsets(lengths, block_bytes: int) -> np.ndarray:
    """int64 ``[B + 1]``: stripe b's mask words are ``[offsets[b], offsets[b + 1])``,
    ``ceil(lengths[b] / block_bytes)`` of them."""
    n = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 0:
        raise ValueError("row lengths must not be negative")
    b = check_block_bytes(block_bytes)
    return np.concatenate([[0], np.cumsum((n + b - 1) // b)]).astype(np.int64)


def build_varlen_scrub_desc(in_ptrs: np.ndarray, lengths: np.ndarray, first_blk: np.ndarray, first_span: np.ndarray,
                            mask_first: np.ndarray, blk_stripe: np.ndarray, span_stripe: np.ndarray,
                            tables: np.ndarray) -> np.ndarray:
    """Descriptor bytes of a variable-length scrub: ``in_ptrs`` uint64 ``[B, n]`` row addresses,
    ``lengths`` int ``[B]``, ``first_blk`` / ``blk_stripe`` from :func:`varlen_blocks`, ``first_span`` /
    ``span_stripe`` from :func:`varlen_spans`, ``mask_first`` int ``[B]`` (:func:`mask_offsets` without its
    last value), ``tables`` the ``(n, m_pad, 8)`` uint32 v_perm records of H, input-major."""
    batch, n = in_ptrs.shape
    mp = int(tables.shape[1])
    lay = varlen_scrub_layout(n, mp, batch, int(blk_stripe.size), int(span_stripe.size))
    buf = np.zeros(lay["bytes"], dtype=np.uint8)

    def put(off, a, dt):
        raw = np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8)
        buf[off: off + raw.size] = raw

    put(0, np.array([n, mp, batch, 0]), "<i4")
    put(lay["in_off"], in_ptrs, "<u8")
    put(lay["len_off"], lengths, "<i8")
    put(lay["first_off"], first_blk, "<i8")
    put(lay["span_first_off"], first_span, "<i8")
    put(lay["mask_first_off"], mask_first, "<i8")
    put(lay["tab_off"], tables, "<u4")
    put(lay["blk_off"], blk_stripe, "<i4")
    put(lay["span_off"], span_stripe, "<i4")
    return buf


class VarlenMask:
    """Result of :meth:`VarlenCodec.syndrome_mask` for B stripes of differing lengths.

    blocks: int32 ``[W]`` on the stripes' device, the mask words of every stripe one after the other:
    stripe b's are ``blocks[offsets[b]:offsets[b + 1]]``, ``ceil(C_b / block_bytes)`` of them, each what
    ``ReedSolomon.syndrome_mask`` defines. offsets: numpy int64 ``[B + 1]`` on the host. stripes: int32
    ``[B]`` on the device, word b the OR of stripe b's words (zero: the stripe is consistent).
    ``of(b)``: the view of stripe b's words."""

    def __init__(self, blocks: torch.Tensor, offsets: np.ndarray, stripes: torch.Tensor):
        self.blocks, self.offsets, self.stripes = blocks, offsets, stripes

    def __len__(self) -> int:
        return int(self.offsets.size) - 1

    def of(self, b: int) -> torch.Tensor:
        b = range(len(self))[b]
        return self.blocks[int(self.offsets[b]): int(self.offsets[b + 1])]

    # (``report[b]`` of a VarlenScrubReport reads ``mask[b]``, as it reads a row of a 2-D batch mask)
    __getitem__ = of


def zero_mask(lengths, block_bytes: int, device) -> VarlenMask:
    """The mask of a batch with nothing to check."""
    off = mask_offsets(lengths, block_bytes)
    both = torch.zeros(int(off[-1]) + off.size - 1, dtype=torch.int32, device=device)
    return VarlenMask(both[: int(off[-1])], off, both[int(off[-1]):])


class VarlenScrubReport(BatchScrubReport):
    """Result of :meth:`VarlenCodec.scrub` and :meth:`VarlenCodec.heal`: the fields of
    :class:`~gpu_rscode_amd.ops.scrub.BatchScrubReport` (``clean``, ``bad_columns``, ``unlocated``,
    ``votes [B, n]``, ``dirty``, ``unhealed``, ``report[b]``), with ``mask`` a :class:`VarlenMask`."""


def make_varlen_report(votes, unlocated, bad_columns, mask: VarlenMask) -> VarlenScrubReport:
    r = make_batch_report(votes, unlocated, bad_columns, mask)
    return VarlenScrubReport(r.clean, r.bad_columns, r.unlocated, r.votes, mask, r.dirty, [])


class VarlenScrubPlan:
    """A reusable device scrub of B stripes of differing lengths: one launch of the syndrome kernel
    over a flat (stripe, column block) work list, one of the locate kernel over a flat (stripe, span)
    list. As :class:`VarlenPlan` it keeps raw row addresses only, so a cache may hand it out only for
    the caller's live tensors.

    Args:
        ptrs: uint64 ``[B, n]``: the row addresses of the stripes, natives first (device memory of ``device``).
        lengths: int ``[B]``: stripe b's row length in bytes, >= 0; at least one above 0.
        h: the p x n check matrix over GF(2^8), shared by every stripe.
        device: the GPU the rows live on.
        block_bytes: columns per mask word, a power of two >= 4096.
        force_bytewise: take the byte-per-lane form even when every row is 16-byte aligned.
    """

    def __init__(self, ptrs: np.ndarray, lengths, h: np.ndarray, device, block_bytes: int = 65536, *,
                 force_bytewise: bool = False):
        ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
        h = np.asarray(h, dtype=np.uint8)
        if ptrs.ndim != 2 or h.ndim != 2 or ptrs.shape[1] != h.shape[1]:
            raise ValueError("ptrs must be a [B, n] array of row addresses and h a p x n matrix")
        self.batch, self.n = ptrs.shape
        self.p = int(h.shape[0])
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        if self.lengths.shape[0] != self.batch:
            raise ValueError(f"{self.batch} stripes but {self.lengths.shape[0]} lengths")
        if not 1 <= self.p < self.n <= 256:
            raise ValueError("VarlenScrubPlan needs 1 <= p < n <= 256")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("VarlenScrubPlan runs on a GPU")
        self.block_bytes = check_block_bytes(block_bytes)
        self.m_pad = pad_m(self.p)
        systematic = np.array_equal(h[:, self.n - self.p:], np.eye(self.p, dtype=np.uint8))
        self.ident = self.p if systematic else 0
        # one unaligned row of some bytes: the whole batch bytewise
        live = (self.lengths > 0)[:, None]
        self.bytewise = bool(force_bytewise or ((ptrs % np.uint64(16) != 0) & live).any())
        _, first, blk = varlen_blocks(self.lengths, self.bytewise)
        _, sfirst, span = varlen_spans(self.lengths, self.block_bytes)
        if not blk.size:
            raise ValueError("VarlenScrubPlan needs a stripe of some bytes")
        self.offsets = mask_offsets(self.lengths, self.block_bytes)
        self.nblk, self.nspan, self.nwords = int(blk.size), int(span.size), int(self.offsets[-1])
        tables = np.zeros((self.n, self.m_pad, 8), dtype=np.uint32)
        tables[:, : self.p] = np.transpose(perm_tables_from_coeff(h), (1, 0, 2))
        host = build_varlen_scrub_desc(ptrs, self.lengths, first, sfirst, self.offsets[:-1], blk, span, tables)
        self.desc = torch.from_numpy(host).to(self.device)
        loc, self.locatable = locate_table(h)
        self.loc = torch.from_numpy(loc).to(self.device) if self.p <= MAX_LOCATE_P else None
        self._ready = ready_event(self.device)

    def _launch_mask(self, st: torch.cuda.Stream, max_blocks: int) -> VarlenMask:
        with torch.cuda.stream(st):
            both = torch.empty(self.nwords + self.batch, dtype=torch.int32, device=self.device)
        hip().varlen_syndrome(int(self.desc.data_ptr()), self.n, self.m_pad, self.ident, self.batch, self.nblk,
                              self.block_bytes, self.bytewise, int(max_blocks), int(both.data_ptr()), self.nwords,
                              st.cuda_stream)
        return VarlenMask(both[: self.nwords], self.offsets, both[self.nwords:])

    def syndrome_mask(self, stream: torch.cuda.Stream | None = None, max_blocks: int = 0) -> VarlenMask:
        """One launch of the syndrome kernel on ``stream`` (default: the current stream); a fresh
        :class:`VarlenMask`. No host sync. ``max_blocks``: as :meth:`VarlenPlan.run`."""
        return self._launch_mask(plan_stream(self, stream, self.desc), max_blocks)

    def scrub(self, stream: torch.cuda.Stream | None = None, max_blocks: int = 0) -> VarlenScrubReport:
        """Both kernels back to back, then one sync (the copy of the counts to the host)."""
        if self.p > MAX_LOCATE_P:
            raise NotImplementedError(f"scrub locates chunks for p <= {MAX_LOCATE_P} (p = {self.p}); "
                                      "syndrome_mask works for any p")
        st = plan_stream(self, stream, self.desc, self.loc)
        mask = self._launch_mask(st, max_blocks)
        with torch.cuda.stream(st):
            counts = torch.empty((self.batch, self.n + 2), dtype=torch.int64, device=self.device)
            hip().varlen_locate(int(self.desc.data_ptr()), self.n, self.p, self.batch, self.nblk, self.nspan,
                                self.block_bytes, self.bytewise, int(max_blocks), int(mask.blocks.data_ptr()),
                                int(self.loc.data_ptr()), self.locatable, int(counts.data_ptr()), st.cuda_stream)
            host = counts.cpu().numpy()
        return make_varlen_report(host[:, : self.n].copy(), host[:, self.n].copy(), host[:, self.n + 1].copy(), mask)
