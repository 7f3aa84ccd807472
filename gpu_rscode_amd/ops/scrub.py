"""Scrub: fused syndrome check, corrupt-chunk location and heal (``csrc/kernels/gf_scrub.hip``).

A Reed-Solomon stripe carries enough redundancy to notice a wrong chunk without any checksum. With
the parity-check matrix ``H = [E | I_p]`` the syndrome ``s = H . [data; parity]`` of a byte column
is zero exactly when the column is consistent, and a multiple of column j of ``H`` when only chunk
j is wrong there. :class:`ScrubPlan` holds the device descriptor (the n stripe rows as inputs, the
tables of ``H``, no outputs) of the two kernels; the CPU form computes the syndrome rows block by
block with the C++ codec and classifies them in numpy. :class:`BatchScrubPlan` is the same for B
stripes of one shape per launch (small objects), over the batched descriptor of ``encode_batch``.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from .. import gf
from .._native import hip
from .gemm import build_desc, pad_m, perm_tables_from_coeff, plan_stream, ready_event
from .rows import StripeBatch, stripe_part

MIN_BLOCK_BYTES = 4096
MAX_LOCATE_P = 16  # the locate kernel keeps one output tile of syndrome bytes per lane
CPU_STEP = 1 << 20  # columns per syndrome slice of the CPU form (p scratch rows of this length)


@dataclass
class ScrubReport:
    """Result of :meth:`ReedSolomon.scrub`.

    clean: no byte column has a nonzero syndrome. bad_columns: how many do. votes: int64 ``[n]``,
    the bad columns that blame each chunk. unlocated: bad columns that blame no single chunk.
    suspects: the sorted chunk ids with ``votes > 0``. mask: int32 ``[ceil(C / block_bytes)]``, bit
    ``i % 32`` set where syndrome row i is nonzero in that column block (on the stripe's device)."""

    clean: bool
    bad_columns: int
    votes: np.ndarray
    unlocated: int
    suspects: list
    mask: torch.Tensor


def check_block_bytes(block_bytes: int) -> int:
    b = int(block_bytes)
    if b < MIN_BLOCK_BYTES or b & (b - 1) or b > 1 << 30:
        raise ValueError(f"block_bytes must be a power of two in [{MIN_BLOCK_BYTES}, 2^30], got {block_bytes}")
    return b


def locate_table(h: np.ndarray) -> tuple[np.ndarray, bool]:
    """Host-prepared operand of the locate kernel: H row-major, then each column's pivot row (its
    first nonzero row) and that pivot's inverse; and whether location means anything (p >= 2 and
    pairwise independent columns)."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    piv = np.zeros(n, dtype=np.uint8)
    pinv = np.zeros(n, dtype=np.uint8)
    for j in range(n):
        nz = np.nonzero(h[:, j])[0]
        if nz.size:
            piv[j] = nz[0]
            pinv[j] = int(gf.GF256.inv(int(h[nz[0], j])))
    return np.concatenate([h.reshape(-1), piv, pinv]), bool(p >= 2 and gf.columns_independent(h))


def make_report(votes: np.ndarray, unlocated: int, bad_columns: int, mask: torch.Tensor) -> ScrubReport:
    votes, bad_columns = np.asarray(votes, dtype=np.int64), int(bad_columns)
    return ScrubReport(bad_columns == 0, bad_columns, votes, int(unlocated),
                       [int(j) for j in np.nonzero(votes)[0]], mask)


# ---- the report of B stripes scrubbed in one launch ------------------------------------------------
class _StripeReports:
    """``BatchScrubReport.report``: ``report[b]`` is stripe b's :class:`ScrubReport`, made on demand."""

    def __init__(self, batch: "BatchScrubReport"):
        self._batch = batch

    def __len__(self) -> int:
        return len(self._batch.clean)

    def __getitem__(self, b: int) -> ScrubReport:
        r = self._batch
        b = range(len(self))[b]
        return make_report(r.votes[b].copy(), int(r.unlocated[b]), int(r.bad_columns[b]), r.mask[b])

    def __iter__(self):
        return (self[b] for b in range(len(self)))


@dataclass
class BatchScrubReport:
    """Result of :meth:`ReedSolomon.scrub_batch` for B stripes: the fields of :class:`ScrubReport`
    with a leading stripe axis.

    clean: bool ``[B]``. bad_columns, unlocated: int64 ``[B]``. votes: int64 ``[B, n]``. mask: int32
    ``[B, ceil(C / block_bytes)]`` on the stripes' device. dirty: the sorted indices of the stripes
    that are not clean. unhealed: the dirty stripes :meth:`ReedSolomon.heal_batch` had to leave as
    they were (``[]`` from a scrub). ``report[b]``: stripe b's :class:`ScrubReport`, equal field
    for field to what ``scrub`` on that stripe alone returns."""

    clean: np.ndarray
    bad_columns: np.ndarray
    unlocated: np.ndarray
    votes: np.ndarray
    mask: torch.Tensor
    dirty: list
    unhealed: list

    @property
    def report(self) -> _StripeReports:
        return _StripeReports(self)


def make_batch_report(votes: np.ndarray, unlocated: np.ndarray, bad_columns: np.ndarray,
                      mask: torch.Tensor) -> BatchScrubReport:
    bad_columns = np.asarray(bad_columns, dtype=np.int64)
    return BatchScrubReport(bad_columns == 0, bad_columns, np.asarray(unlocated, dtype=np.int64),
                            np.asarray(votes, dtype=np.int64), mask, [int(b) for b in np.nonzero(bad_columns)[0]], [])


class ScrubBase:
    """What :class:`ScrubPlan` and :class:`BatchScrubPlan` share: everything but how they are built and
    whether the launches and results carry a stripe axis (``_batched``)."""

    def _build(self, batch, nrows: int, h: np.ndarray, block_bytes: int) -> None:
        """``batch``: a part or a ``StripeBatch`` of stripes of ``nrows`` rows."""
        self.p, self.n = h.shape
        if nrows != self.n:
            raise ValueError(f"expected stripes of {self.n} rows, got {nrows}")
        if batch.nstripes < 1:
            raise ValueError(f"{type(self).__name__} needs at least one stripe")
        self.device = batch.device
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} runs on a GPU")
        self.block_bytes = check_block_bytes(block_bytes)
        self.batch, self.ncols = batch.nstripes, batch.ncols
        self._lead = (self.batch,) if self._batched else ()  # the stripe axis of the launches and the results
        self.nmask = -(-self.ncols // self.block_bytes)
        self._mask_shape = self._lead + (self.nmask,)
        self.m_pad = pad_m(self.p)
        # H = [E | I_p]: the kernel may XOR the parity rows in as they are
        systematic = self.p < self.n and np.array_equal(h[:, self.n - self.p:], np.eye(self.p, dtype=np.uint8))
        self.ident = self.p if systematic else 0
        ptrs = batch.ptrs()
        self.bytewise = bool((ptrs % np.uint64(16)).any())  # one unaligned row: the whole batch bytewise
        host = build_desc(ptrs.reshape(-1), [0] * (self.p * self.batch), None, perm_tables_from_coeff(h), self.batch)
        self.desc = torch.from_numpy(host).to(self.device)
        loc, self.locatable = locate_table(h)
        self.loc = torch.from_numpy(loc).to(self.device) if self.p <= MAX_LOCATE_P else None
        self._ready = ready_event(self.device)

    def syndrome_mask(self, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Launch the syndrome kernel (one launch for a whole batch); returns a fresh int32 ``[nmask]``
        (batched: ``[B, nmask]``) device tensor. No host sync."""
        st = plan_stream(self, stream, self.desc)
        with torch.cuda.stream(st):
            mask = torch.empty(self._mask_shape, dtype=torch.int32, device=self.device)
        if self.ncols:
            launch = hip().syndrome_batched if self._batched else hip().syndrome
            launch(int(self.desc.data_ptr()), self.n, self.m_pad, self.ident, *self._lead, self.ncols, self.bytewise,
                   self.block_bytes, int(mask.data_ptr()), st.cuda_stream)
        return mask

    def scrub(self, stream: torch.cuda.Stream | None = None):
        """Both kernels back to back, then one sync (the copy of the counts to the host). Returns a
        :class:`ScrubReport` (batched: a :class:`BatchScrubReport`)."""
        if self.p > MAX_LOCATE_P:
            raise NotImplementedError(f"scrub locates chunks for p <= {MAX_LOCATE_P} (p = {self.p}); "
                                      "syndrome_mask works for any p")
        mask = self.syndrome_mask(stream)
        st = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            counts = torch.empty(self._lead + (self.n + 2,), dtype=torch.int64, device=self.device)
            if self.ncols:
                if stream is not None:
                    self.loc.record_stream(stream)
                launch = hip().locate_batched if self._batched else hip().locate
                launch(int(self.desc.data_ptr()), self.n, self.p, *self._lead, self.ncols, self.bytewise,
                       self.block_bytes, int(mask.data_ptr()), int(self.loc.data_ptr()), self.locatable,
                       int(counts.data_ptr()), st.cuda_stream)
            else:
                counts.zero_()
            host = counts.cpu().numpy()
        report = make_batch_report if self._batched else make_report
        return report(host[..., : self.n].copy(), host[..., self.n].copy(), host[..., self.n + 1].copy(), mask)


class ScrubPlan(ScrubBase):
    """A reusable device scrub of one stripe's buffers, as ``GemmPlan(hold_buffers=False)``: it keeps
    raw row pointers only, so a cache may hand it out only for the caller's live tensors.

    Args:
        rows: the n stripe rows (natives first) on one GPU; the shortest row bounds the columns.
        h: the p x n check matrix over GF(2^8).
        block_bytes: columns per mask word, a power of two >= 4096.
    """

    _batched = False

    def __init__(self, rows, h: np.ndarray, block_bytes: int = 65536):
        h = np.asarray(h, dtype=np.uint8)
        part = stripe_part(rows, "stripe")
        self._build(part, part.nrows, h, block_bytes)


class BatchScrubPlan(ScrubBase):
    """A reusable device scrub of B stripes of one shape, one launch per kernel (grid.y = stripe). As
    :class:`ScrubPlan` it keeps raw row pointers only, so a cache may hand it out only for the
    caller's live tensors.

    Args:
        stripes: B stripes of n rows each (natives first) as a list of row lists (or a
            :class:`~gpu_rscode_amd.ops.rows.StripeBatch`), all rows on one GPU and of one length C.
        h: the p x n check matrix over GF(2^8), shared by every stripe.
        block_bytes: columns per mask word, a power of two >= 4096.
    """

    _batched = True

    def __init__(self, stripes, h: np.ndarray, block_bytes: int = 65536):
        h = np.asarray(h, dtype=np.uint8)
        batch = stripes if isinstance(stripes, StripeBatch) else StripeBatch(stripes, h.shape[1])
        self._build(batch, batch.n, h, block_bytes)


@lru_cache(maxsize=1)
def mul_table() -> np.ndarray:
    """mul[a][b] over GF(2^8) (64 KiB)."""
    return np.stack([gf.GF256.mul_table(c) for c in range(256)])


@lru_cache(maxsize=16)
def _cpu_locator(h_bytes: bytes, p: int, n: int):
    """(locatable, pivot row of each native column, that column scaled so its pivot entry is 1): a
    syndrome that blames native j is s_r times the scaled column."""
    h = np.frombuffer(h_bytes, dtype=np.uint8).reshape(p, n)
    k = n - p
    _, locatable = locate_table(h)
    unit = np.zeros((k, p), dtype=np.uint8)
    piv = np.zeros(k, dtype=np.int64)
    if locatable:
        f = gf.GF256
        for j in range(k):
            piv[j] = np.nonzero(h[:, j])[0][0]
            unit[j] = f.mul(h[:, j], int(f.inv(int(h[piv[j], j]))))
    return locatable, piv, unit


def cpu_scrub(h: np.ndarray, rows: list[torch.Tensor], ncols: int, block_bytes: int, cpu_gemm, locate: bool = True):
    """CPU form: syndrome rows slice by slice into p bounded scratch rows (``cpu_gemm(coeff, ins,
    outs)`` is the codec's GEMM), mask and classification in numpy. Returns ``(mask, votes,
    unlocated, bad_columns)``; with ``locate=False`` only the mask is computed."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    k = n - p
    block_bytes = check_block_bytes(block_bytes)
    bits = np.zeros(-(-ncols // block_bytes), dtype=np.uint32)
    votes = np.zeros(n, dtype=np.int64)
    unlocated = bad_columns = 0
    if p == 0 or ncols == 0:
        return torch.from_numpy(bits.view(np.int32)), votes, 0, 0
    locatable, piv, unit = _cpu_locator(h.tobytes(), p, n)
    mul = mul_table()
    step = min(CPU_STEP, -(-ncols // 64) * 64)
    scratch = torch.empty((p, step), dtype=torch.uint8)
    for c0 in range(0, ncols, step):
        c1 = min(ncols, c0 + step)
        outs = [scratch[i, : c1 - c0] for i in range(p)]
        cpu_gemm(h, [r[c0:c1] for r in rows], outs)
        s = scratch[:, : c1 - c0].numpy()
        nzrow = s != 0
        cols = np.nonzero(nzrow.any(axis=0))[0]
        if cols.size == 0:
            continue
        for i in range(p):
            hit = cols[nzrow[i, cols]]
            bits[np.unique((c0 + hit) // block_bytes)] |= np.uint32(1 << (i % 32))
        if not locate:
            continue
        bad_columns += int(cols.size)
        if not locatable:
            unlocated += int(cols.size)
            continue
        sb = s[:, cols]  # the bad columns only
        cnt = nzrow[:, cols].sum(axis=0)
        one = cnt == 1
        votes[k:] += (nzrow[:, cols] & one).sum(axis=1)
        todo = np.nonzero(~one)[0]
        for j in range(k):
            if todo.size == 0:
                break
            st = sb[:, todo]
            e = st[piv[j]]
            hit = (mul[e[None, :], unit[j][:, None]] == st).all(axis=0) & (e != 0)
            votes[j] += int(hit.sum())
            todo = todo[~hit]
        unlocated += int(todo.size)
    return torch.from_numpy(bits.view(np.int32)), votes, unlocated, bad_columns
