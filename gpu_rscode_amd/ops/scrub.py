"""Scrub: fused syndrome check, corrupt-chunk location and heal (``csrc/kernels/gf_scrub.hip``).

A Reed-Solomon stripe carries enough redundancy to notice a wrong chunk without any checksum. With
the parity-check matrix ``H = [E | I_p]`` the syndrome ``s = H . [data; parity]`` of a byte column
is zero exactly when the column is consistent, and a multiple of column j of ``H`` when only chunk
j is wrong there. :class:`ScrubPlan` holds the device descriptor (the n stripe rows as inputs, the
tables of ``H``, no outputs) of the two kernels; the CPU form computes the syndrome rows block by
block with the C++ codec and classifies them in numpy.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from .. import gf
from .._native import hip
from .gemm import _check_rows, _rows, build_desc, pad_m, perm_tables_from_coeff

MIN_BLOCK_BYTES = 4096
MAX_LOCATE_P = 16  # the locate kernel keeps one output tile of syndrome bytes per lane
_CPU_STEP = 1 << 20  # columns per syndrome slice of the CPU form (p scratch rows of this length)


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


def stripe_rows(stripe, n: int) -> tuple[list[torch.Tensor], int, torch.device]:
    rows = _rows(stripe)
    if len(rows) != n:
        raise ValueError(f"stripe must have n={n} rows")
    dev = _check_rows(rows, "stripe", None)
    return rows, min(r.numel() for r in rows), dev


class ScrubPlan:
    """A reusable device scrub of one stripe's buffers, as ``GemmPlan(hold_buffers=False)``: it keeps
    raw row pointers only, so a cache may hand it out only for the caller's live tensors.

    Args:
        rows: the n stripe rows (natives first) on one GPU.
        h: the p x n check matrix over GF(2^8).
        block_bytes: columns per mask word, a power of two >= 4096.
    """

    def __init__(self, rows, h: np.ndarray, block_bytes: int = 65536):
        rows = _rows(rows)
        h = np.asarray(h, dtype=np.uint8)
        self.p, self.n = h.shape
        if len(rows) != self.n:
            raise ValueError(f"expected {self.n} stripe rows, got {len(rows)}")
        self.device = _check_rows(rows, "stripe", None)
        if self.device.type != "cuda":
            raise ValueError("ScrubPlan runs on a GPU")
        self.block_bytes = check_block_bytes(block_bytes)
        self.ncols = min(r.numel() for r in rows)
        self.nmask = -(-self.ncols // self.block_bytes)
        self.m_pad = pad_m(self.p)
        # H = [E | I_p]: the kernel may XOR the parity rows in as they are
        systematic = self.p < self.n and np.array_equal(h[:, self.n - self.p:], np.eye(self.p, dtype=np.uint8))
        self.ident = self.p if systematic else 0
        ptrs = [int(r.data_ptr()) for r in rows]
        self.bytewise = any(q % 16 for q in ptrs)
        host = build_desc(ptrs, [0] * self.p, None, perm_tables_from_coeff(h))
        self.desc = torch.from_numpy(host).to(self.device)
        loc, self.locatable = locate_table(h)
        self.loc = torch.from_numpy(loc).to(self.device) if self.p <= MAX_LOCATE_P else None
        self._ready = torch.cuda.Event()
        self._ready.record(torch.cuda.current_stream(self.device))

    def _stream(self, stream: torch.cuda.Stream | None) -> torch.cuda.Stream:
        st = stream or torch.cuda.current_stream(self.device)
        if self._ready is not None:
            st.wait_event(self._ready)
            self._ready = None
        if stream is not None:
            self.desc.record_stream(stream)
        return st

    def syndrome_mask(self, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Launch the syndrome kernel; returns a fresh int32 ``[nmask]`` device tensor. No host sync."""
        st = self._stream(stream)
        with torch.cuda.stream(st):
            mask = torch.empty(self.nmask, dtype=torch.int32, device=self.device)
        if self.ncols:
            hip().syndrome(int(self.desc.data_ptr()), self.n, self.m_pad, self.ident, self.ncols, self.bytewise,
                           self.block_bytes, int(mask.data_ptr()), st.cuda_stream)
        return mask

    def scrub(self, stream: torch.cuda.Stream | None = None) -> ScrubReport:
        """Both kernels back to back, then one sync (the copy of the counts to the host)."""
        if self.p > MAX_LOCATE_P:
            raise NotImplementedError(f"scrub locates chunks for p <= {MAX_LOCATE_P} (p = {self.p}); "
                                      "syndrome_mask works for any p")
        mask = self.syndrome_mask(stream)
        st = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            counts = torch.empty(self.n + 2, dtype=torch.int64, device=self.device)
            if self.ncols:
                if stream is not None:
                    self.loc.record_stream(stream)
                hip().locate(int(self.desc.data_ptr()), self.n, self.p, self.ncols, self.bytewise, self.block_bytes,
                             int(mask.data_ptr()), int(self.loc.data_ptr()), self.locatable, int(counts.data_ptr()),
                             st.cuda_stream)
            else:
                counts.zero_()
            host = counts.cpu().numpy()
        return make_report(host[: self.n].copy(), int(host[self.n]), int(host[self.n + 1]), mask)


def make_report(votes: np.ndarray, unlocated: int, bad_columns: int, mask: torch.Tensor) -> ScrubReport:
    votes = np.asarray(votes, dtype=np.int64)
    return ScrubReport(bad_columns == 0, int(bad_columns), votes, int(unlocated),
                       [int(j) for j in np.nonzero(votes)[0]], mask)


@lru_cache(maxsize=1)
def _mul_table() -> np.ndarray:
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
    mul = _mul_table()
    step = min(_CPU_STEP, -(-ncols // 64) * 64)
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
