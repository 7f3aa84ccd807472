"""Correct: error correction per byte column, in place (``csrc/kernels/gf_correct.hip``).

``heal`` repairs silent corruption at chunk granularity: it names suspect chunks and rebuilds them
whole, and gives up when more than p chunks are suspect or two are wrong in one column. A
Reed-Solomon code corrects *errors*, not only erasures, column by column. For a byte column with
syndrome ``s = H . stripe[:, c] != 0`` the rule (the contract of ``gf.correct_oracle``,
:func:`cpu_correct` and the kernel) is:

1. p < 2, or two columns of ``H`` dependent (``locate_table``'s ``locatable``): uncorrectable.
2. Weight 1: ``s = e . H[:, j]`` for a chunk j, parity chunks included, and e != 0:
   ``stripe[j][c] ^= e``. Pairwise independence makes (j, e) unique.
3. Otherwise, with ``max_errors == 2``: the explanations ``s = e1 . H[:, j1] ^ e2 . H[:, j2]``
   (j1 < j2, e1, e2 != 0) are counted over all pairs. Exactly one: both bytes are XORed. None, or
   more than one (a non-MDS ``H`` has dependent 4-sets of columns): uncorrectable.
4. An uncorrectable column is left byte for byte as it was.

:class:`CorrectPlan` and :class:`BatchCorrectPlan` are the scrub plans with one more launch: the
syndrome kernel, then the correct kernel over the dirty blocks, then one sync for the counts.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from .. import gf
from .._native import hip
from .rows import StripeBatch, stripe_part
from .scrub import CPU_STEP, MAX_LOCATE_P, ScrubBase, check_block_bytes, locate_table, mul_table
from .update import check_overlap_batch

MAX_PAIR_N = 64  # kCorrectMaxPairN: the pair search walks n^2 / 2 pairs per column from the log tables in LDS


@dataclass
class CorrectReport:
    """Result of :meth:`ReedSolomon.correct`.

    clean: no byte column had a nonzero syndrome. bad_columns: how many had. fixed_bytes: int64
    ``[n]``, the bytes changed in each chunk. by_weight: int64 ``[3]``, ``by_weight[w]`` the columns
    corrected with w errors. uncorrectable: the bad columns left as they were. mask: the syndrome
    mask **before** correction (int32 ``[ceil(C / block_bytes)]`` on the stripe's device)."""

    clean: bool
    bad_columns: int
    fixed_bytes: np.ndarray
    by_weight: np.ndarray
    uncorrectable: int
    mask: torch.Tensor


def make_correct_report(fixed_bytes, by_weight, uncorrectable, bad_columns, mask: torch.Tensor) -> CorrectReport:
    bad_columns = int(bad_columns)
    return CorrectReport(bad_columns == 0, bad_columns, np.asarray(fixed_bytes, dtype=np.int64),
                         np.asarray(by_weight, dtype=np.int64), int(uncorrectable), mask)


class _StripeReports:
    """``BatchCorrectReport.report``: ``report[b]`` is stripe b's :class:`CorrectReport`, made on demand."""

    def __init__(self, batch: "BatchCorrectReport"):
        self._batch = batch

    def __len__(self) -> int:
        return len(self._batch.clean)

    def __getitem__(self, b: int) -> CorrectReport:
        r = self._batch
        b = range(len(self))[b]
        return make_correct_report(r.fixed_bytes[b].copy(), r.by_weight[b].copy(), r.uncorrectable[b],
                                   r.bad_columns[b], r.mask[b])

    def __iter__(self):
        return (self[b] for b in range(len(self)))


@dataclass
class BatchCorrectReport:
    """Result of :meth:`ReedSolomon.correct_batch` for B stripes: the fields of :class:`CorrectReport`
    with a leading stripe axis.

    clean: bool ``[B]``. bad_columns, uncorrectable: int64 ``[B]``. fixed_bytes: int64 ``[B, n]``.
    by_weight: int64 ``[B, 3]``. mask: int32 ``[B, ceil(C / block_bytes)]`` on the stripes' device,
    before correction. dirty: the sorted indices of the stripes that were not clean. ``report[b]``:
    stripe b's :class:`CorrectReport`, equal field for field to what ``correct`` on that stripe
    alone returns."""

    clean: np.ndarray
    bad_columns: np.ndarray
    fixed_bytes: np.ndarray
    by_weight: np.ndarray
    uncorrectable: np.ndarray
    mask: torch.Tensor
    dirty: list

    @property
    def report(self) -> _StripeReports:
        return _StripeReports(self)


def make_batch_correct_report(fixed_bytes, by_weight, uncorrectable, bad_columns,
                              mask: torch.Tensor) -> BatchCorrectReport:
    bad_columns = np.asarray(bad_columns, dtype=np.int64)
    return BatchCorrectReport(bad_columns == 0, bad_columns, np.asarray(fixed_bytes, dtype=np.int64),
                              np.asarray(by_weight, dtype=np.int64), np.asarray(uncorrectable, dtype=np.int64), mask,
                              [int(b) for b in np.nonzero(bad_columns)[0]])


def check_max_errors(max_errors, p: int, n: int) -> int:
    """The validated ``max_errors`` of a (p x n) check matrix: default ``min(2, p // 2)``. ValueError
    for p < 2 (nothing can be corrected), a value outside {1, 2} and 2 with p < 4 (distance below 5);
    NotImplementedError for p > MAX_LOCATE_P and for 2 with n > MAX_PAIR_N."""
    if p < 2:
        raise ValueError(f"correct needs p >= 2 parity chunks, got p = {p}")
    if p > MAX_LOCATE_P:
        raise NotImplementedError(f"correct is implemented for p <= {MAX_LOCATE_P} (p = {p})")
    m = min(2, p // 2) if max_errors is None else max_errors
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m not in (1, 2):
        raise ValueError(f"max_errors must be 1 or 2, got {max_errors!r}")
    if m == 2 and p < 4:
        raise ValueError(f"max_errors=2 needs p >= 4 (distance 5), got p = {p}")
    if m == 2 and n > MAX_PAIR_N:
        raise NotImplementedError(f"max_errors=2 is implemented for n <= {MAX_PAIR_N} (n = {n}); max_errors=1 "
                                  "works for any n <= 256")
    return int(m)


def check_disjoint(ptrs: np.ndarray, lens) -> None:
    """ValueError when, by address range, any row overlaps another row of the same or another stripe
    (so also for a stripe listed twice): every row may be written, so every row plays "parity" in
    :func:`~gpu_rscode_amd.ops.update.check_overlap_batch`. ``ptrs``: uint64 ``[B, n]``; ``lens``:
    the rows' one length or their ``[B, n]`` lengths."""
    ptrs = np.asarray(ptrs)
    try:
        check_overlap_batch(ptrs, np.zeros((ptrs.shape[0], 0), dtype=np.uint64), None, [lens, 0])
    except ValueError as e:
        raise ValueError(f"a stripe row overlaps another row: correct works in place and needs disjoint rows ({e})"
                         ) from None


class _Correct(ScrubBase):
    """What :class:`CorrectPlan` and :class:`BatchCorrectPlan` add to the scrub plans they are built as:
    ``max_errors``, the aliasing check and the correct launch."""

    def _build_correct(self, batch, nrows: int, h: np.ndarray, max_errors, block_bytes: int, check: bool) -> None:
        p, n = h.shape
        self.max_errors = check_max_errors(max_errors, p, n)
        if nrows != n:
            raise ValueError(f"expected stripes of {n} rows, got {nrows}")
        if check:
            check_disjoint(batch.ptrs(), getattr(batch, "lens", batch.ncols))
        self._build(batch, nrows, h, block_bytes)

    def correct(self, stream: torch.cuda.Stream | None = None):
        """The syndrome launch, one correct launch, then one sync (the copy of the counts to the host).
        Returns a :class:`CorrectReport` (batched: a :class:`BatchCorrectReport`)."""
        mask = self.syndrome_mask(stream)
        st = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            counts = torch.empty(self._lead + (self.n + 4,), dtype=torch.int64, device=self.device)
            if self.ncols:
                if stream is not None:
                    self.loc.record_stream(stream)
                launch = hip().correct_batched if self._batched else hip().correct
                launch(int(self.desc.data_ptr()), self.n, self.p, *self._lead, self.ncols, self.bytewise,
                       self.block_bytes, int(mask.data_ptr()), int(self.loc.data_ptr()), self.locatable,
                       self.max_errors, int(counts.data_ptr()), st.cuda_stream)
            else:
                counts.zero_()
            host = counts.cpu().numpy()
        n = self.n
        by_weight = np.concatenate([np.zeros_like(host[..., :1]), host[..., n: n + 2]], axis=-1)
        report = make_batch_correct_report if self._batched else make_correct_report
        return report(host[..., :n].copy(), by_weight, host[..., n + 2].copy(), host[..., n + 3].copy(), mask)


class CorrectPlan(_Correct):
    """A reusable device correction of one stripe's buffers; as :class:`~gpu_rscode_amd.ops.scrub.ScrubPlan`
    it keeps raw row pointers only, so a cache may hand it out only for the caller's live tensors.

    Args:
        rows: the n stripe rows (natives first) on one GPU, corrected in place; the shortest row
            bounds the columns. No row may overlap another.
        h: the p x n check matrix over GF(2^8), 2 <= p <= 16.
        max_errors: 1 or 2 (default ``min(2, p // 2)``); 2 needs p >= 4 and n <= :data:`MAX_PAIR_N`.
        block_bytes: columns per mask word, a power of two >= 4096.
        check: run the aliasing check (:func:`check_disjoint`); False when the caller has.
    """

    _batched = False

    def __init__(self, rows, h: np.ndarray, max_errors: int | None = None, block_bytes: int = 65536, *,
                 check: bool = True):
        h = np.asarray(h, dtype=np.uint8)
        part = stripe_part(rows, "stripe")
        self._build_correct(part, part.nrows, h, max_errors, block_bytes, check)


class BatchCorrectPlan(_Correct):
    """A reusable device correction of B stripes of one shape, one launch per kernel (grid.y =
    stripe); raw row pointers only, as :class:`CorrectPlan`.

    Args:
        stripes: B stripes of n rows each as :class:`~gpu_rscode_amd.ops.scrub.BatchScrubPlan` takes
            them, corrected in place. No row may overlap another row of any stripe.
        h, max_errors, block_bytes, check: as :class:`CorrectPlan`.
    """

    _batched = True

    def __init__(self, stripes, h: np.ndarray, max_errors: int | None = None, block_bytes: int = 65536, *,
                 check: bool = True):
        h = np.asarray(h, dtype=np.uint8)
        batch = stripes if isinstance(stripes, StripeBatch) else StripeBatch(stripes, h.shape[1])
        self._build_correct(batch, batch.n, h, max_errors, block_bytes, check)


@lru_cache(maxsize=16)
def _cpu_corrector(h_bytes: bytes, p: int, n: int):
    """(locatable, pivot row of each column, each column scaled so its pivot entry is 1, the inverses)."""
    h = np.frombuffer(h_bytes, dtype=np.uint8).reshape(p, n)
    _, locatable = locate_table(h)
    inv = np.zeros(256, dtype=np.uint8)
    inv[1:] = gf.GF256.inv(np.arange(1, 256))
    piv = np.zeros(n, dtype=np.int64)
    unit = np.zeros((n, p), dtype=np.uint8)
    if locatable:
        for j in range(n):
            piv[j] = np.nonzero(h[:, j])[0][0]
            unit[j] = gf.GF256.mul(h[:, j], int(inv[h[piv[j], j]]))
    return locatable, piv, unit, inv


def _correct_columns(h: np.ndarray, s: np.ndarray, max_errors: int):
    """The rule on the bad columns ``s`` (p x m syndromes, none zero) of a locatable ``h``: returns
    ``(weight [m], j [2, m], e [2, m])``: weight 0 (uncorrectable), 1 or 2, and the chunks and error
    values of the repair. The pair search projects column j1 out, as the kernel does."""
    p, n = h.shape
    _, piv, unit, inv = _cpu_corrector(h.tobytes(), p, n)
    mul = mul_table()
    m = s.shape[1]
    weight = np.zeros(m, dtype=np.int64)
    js, es = np.zeros((2, m), dtype=np.int64), np.zeros((2, m), dtype=np.uint8)
    todo = np.arange(m)
    for j in range(n):
        if todo.size == 0:
            break
        st = s[:, todo]
        sr = st[piv[j]]
        hit = (mul[sr[None, :], unit[j][:, None]] == st).all(axis=0) & (sr != 0)
        weight[todo[hit]], js[0, todo[hit]] = 1, j
        es[0, todo[hit]] = mul[inv[h[piv[j], j]]][sr[hit]]
        todo = todo[~hit]
    if max_errors < 2 or todo.size == 0:
        return weight, js, es
    st = s[:, todo]
    count = np.zeros(todo.size, dtype=np.int64)
    fj, fe = np.zeros((2, todo.size), dtype=np.int64), np.zeros((2, todo.size), dtype=np.uint8)
    for j1 in range(n - 1):
        r = piv[j1]
        t = st ^ mul[unit[j1][:, None], st[r][None, :]]  # P(s): row r is zero
        for j2 in range(j1 + 1, n):
            q = h[:, j2] ^ mul[h[r, j2]][unit[j1]]  # P(H[:, j2])
            i = int(np.nonzero(q)[0][0])  # (pairwise independent: q != 0)
            e2 = mul[inv[q[i]]][t[i]]
            x = st[r] ^ mul[h[r, j2]][e2]  # e1 . H[r][j1]
            ok = (e2 != 0) & (x != 0) & (mul[q[:, None], e2[None, :]] == t).all(axis=0)
            first = ok & (count == 0)
            fj[0, first], fj[1, first] = j1, j2
            fe[0, first], fe[1, first] = mul[inv[h[r, j1]]][x[first]], e2[first]
            count += ok
    one = count == 1
    weight[todo[one]] = 2
    js[:, todo[one]], es[:, todo[one]] = fj[:, one], fe[:, one]
    return weight, js, es


def cpu_correct(h: np.ndarray, rows: list[torch.Tensor], ncols: int, block_bytes: int, max_errors: int, cpu_gemm,
                on_fix=None):
    """CPU form: syndrome rows slice by slice into p bounded scratch rows (``cpu_gemm(coeff, ins,
    outs)`` is the codec's GEMM, as :func:`~gpu_rscode_amd.ops.scrub.cpu_scrub` takes it), the rule
    in numpy on the bad columns only, the fixes XORed into ``rows`` in place. Returns ``(mask,
    fixed_bytes, by_weight, uncorrectable, bad_columns)``, the mask that of the stripe as it came.
    ``on_fix(j, cols, values)`` is called for the bytes ``cols`` of row j that got ``^= values``."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    block_bytes = check_block_bytes(block_bytes)
    bits = np.zeros(-(-ncols // block_bytes), dtype=np.uint32)
    fixed_bytes, by_weight = np.zeros(n, dtype=np.int64), np.zeros(3, dtype=np.int64)
    uncorrectable = bad_columns = 0
    if ncols == 0:
        return torch.from_numpy(bits.view(np.int32)), fixed_bytes, by_weight, 0, 0
    locatable = _cpu_corrector(h.tobytes(), p, n)[0]
    host = [r.numpy() for r in rows]  # (views: the fixes land in the caller's rows)
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
        bad_columns += int(cols.size)
        if not locatable:
            uncorrectable += int(cols.size)
            continue
        weight, js, es = _correct_columns(h, s[:, cols], max_errors)
        for w in (1, 2):
            sel = np.nonzero(weight >= w)[0]
            for j in np.unique(js[w - 1, sel]):
                at = sel[js[w - 1, sel] == j]
                host[j][c0 + cols[at]] ^= es[w - 1, at]
                fixed_bytes[j] += int(at.size)
                if on_fix is not None:
                    on_fix(int(j), c0 + cols[at], es[w - 1, at])
            by_weight[w] += int((weight == w).sum())
        uncorrectable += int((weight == 0).sum())
    return torch.from_numpy(bits.view(np.int32)), fixed_bytes, by_weight, uncorrectable, bad_columns
