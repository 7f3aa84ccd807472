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
from .gemm import pad_m, plan_stream, ready_event
from .repair import repair_rows, repair_tables
from .update import check_overlap_batch

GROUP = 16   # bytes a lane of the vector form owns
BLOCK = 256  # lanes per workgroup
MAX_BLOCKS = 2 ** 31 - 1  # work items per launch


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
