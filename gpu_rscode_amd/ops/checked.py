"""Checked repair: rebuild the erased chunks of a degraded stripe and, in the same pass, check and
correct the survivors with the parity the erasures leave over (``csrc/kernels/gf_checked.hip``).

``reconstruct`` trusts the first k survivors blindly; ``correct`` needs all n chunks. With e chunks
lost, r = p - e check equations remain: they detect a wrong survivor for r >= 1 and locate and
correct ``r // 2`` of them per byte column (errors-and-erasures decoding). With X the erased ids, S
the others ascending, K the first k of S and R the rest, ``T = inv(H[:, X + R]) . H``
(:func:`gpu_rscode_amd.gf.checked_matrix`) has ``T[:, X + R] = I_p``: rows ``0..e-1`` rebuild X from
K, rows ``e..p-1`` re-encode survivor ``R[i]`` from K and XOR it in. Per byte column: the erased
rows get ``T[:e, K] . stripe[K]``; a column with ``u = T[e:, S] . stripe[S] != 0`` is bad and gets
``correct``'s rule with the check matrix ``T[e:, S]``; a corrected survivor byte j gets ``^= v`` and
every erased row ``^= v . T[i][j]``. The erased rows are never read. The contract is
``gf.reconstruct_checked_oracle``; :func:`cpu_reconstruct_checked` and the kernels match it exactly.

:class:`CheckedRepairPlan` and :class:`BatchCheckedRepairPlan` hold the device descriptor (the
survivors as inputs, the erased rows as outputs, the tables of ``T[:, S]``) of the two launches: the
hot pass that rebuilds and checks, the cold pass over the dirty blocks, then one sync for the counts.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import gf
from .._native import hip
from .correct import (MAX_PAIR_N, check_disjoint, cpu_correct, make_batch_correct_report, make_correct_report)
from .gemm import build_desc, pad_m, perm_tables_from_coeff, plan_stream, ready_event
from .rows import StripeBatch, stripe_part
from .scrub import MAX_LOCATE_P, check_block_bytes, locate_table, mul_table


def check_erased(erased, n: int, p: int) -> list[int]:
    """The sorted, deduplicated erased ids; ValueError for anything but integers in ``[0, n)`` and
    for more than p of them."""
    try:
        raw = [e for e in erased]
    except TypeError:
        raise ValueError(f"erased must be a sequence of chunk ids, got {erased!r}") from None
    for e in raw:
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)):
            raise ValueError(f"erased ids must be integers, got {e!r}")
    x = sorted(set(int(e) for e in raw))
    if x and not 0 <= x[0] <= x[-1] < n:
        raise ValueError(f"erased ids must lie in [0, {n}), got {x}")
    if len(x) > p:
        raise ValueError(f"{len(x)} erasures {x}, more than p={p}")
    return x


def check_checked_max_errors(max_errors, r: int, ns: int) -> int:
    """The validated ``max_errors`` of a degraded stripe with r check rows over ns survivors: default
    ``min(2, r // 2)`` and at least 1. With r < 2 nothing is corrected and 1 is all that may be asked.
    ValueError for a value outside {1, 2} and 2 with r < 4; NotImplementedError for 2 with more
    than MAX_PAIR_N survivors."""
    m = max(1, min(2, r // 2)) if max_errors is None else max_errors
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m not in (1, 2):
        raise ValueError(f"max_errors must be 1 or 2, got {max_errors!r}")
    if m == 2 and r < 4:
        raise ValueError(f"max_errors=2 needs r = p - e >= 4 check rows (distance 5 among the survivors), got r = {r}")
    if m == 2 and ns > MAX_PAIR_N:
        raise NotImplementedError(f"max_errors=2 is implemented for at most {MAX_PAIR_N} survivors ({ns} survive); "
                                  "max_errors=1 works for any n <= 256")
    return int(m)


class _CheckedRepair:
    """What :class:`CheckedRepairPlan` and :class:`BatchCheckedRepairPlan` share: everything but how
    they are built and whether the launches and results carry a stripe axis (``_batched``)."""

    def _build(self, batch, nrows: int, h: np.ndarray, erased, max_errors, block_bytes: int, check: bool) -> None:
        self.p, self.n = h.shape
        if self.p < 1 or self.p > MAX_LOCATE_P:
            raise NotImplementedError(f"checked repair is implemented for 1 <= p <= {MAX_LOCATE_P} (p = {self.p})")
        if nrows != self.n:
            raise ValueError(f"expected stripes of {self.n} rows, got {nrows}")
        if batch.nstripes < 1:
            raise ValueError(f"{type(self).__name__} needs at least one stripe")
        self.device = batch.device
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} runs on a GPU")
        self.block_bytes = check_block_bytes(block_bytes)
        x = check_erased(erased, self.n, self.p)
        self.t, self.erased, self.survivors, _ = gf.checked_matrix(h, x)
        self.e, self.r, self.ns = len(x), self.p - len(x), self.n - len(x)
        self.max_errors = check_checked_max_errors(max_errors, self.r, self.ns)
        ptrs = batch.ptrs()
        if check:
            check_disjoint(ptrs, getattr(batch, "lens", batch.ncols))
        self.batch, self.ncols = batch.nstripes, batch.ncols
        self._lead = (self.batch,) if self._batched else ()
        self.nmask = -(-self.ncols // self.block_bytes)
        self.bytewise = bool((ptrs % np.uint64(16)).any())  # one unaligned row, read or written: bytewise
        s = self.survivors
        ts = self.t[:, s]
        outs = np.zeros((self.batch, self.p), dtype=np.uint64)  # the erased rows, then rows never stored
        outs[:, : self.e] = ptrs[:, x]
        host = build_desc(ptrs[:, s].reshape(-1), outs.reshape(-1), None, perm_tables_from_coeff(ts), self.batch)
        self.desc = torch.from_numpy(host).to(self.device)
        self.loc, self.locatable = None, False
        if self.r:
            loc, self.locatable = locate_table(ts[self.e:])
            self.loc = torch.from_numpy(np.concatenate([loc, ts[: self.e].reshape(-1)])).to(self.device)
        self._ready = ready_event(self.device)

    def run(self, stream: torch.cuda.Stream | None = None):
        """The hot launch, with r >= 1 the cold launch, then one sync (the copy of the counts to the
        host; none with r = 0). Returns a :class:`~gpu_rscode_amd.ops.correct.CorrectReport`
        (batched: a :class:`~gpu_rscode_amd.ops.correct.BatchCorrectReport`) by chunk id."""
        st = plan_stream(self, stream, self.desc)
        h = hip()
        lead = (self.desc.data_ptr(), self.ns, self.e, self.r) + self._lead + (self.ncols, self.bytewise,
                                                                                self.block_bytes)
        host = np.zeros(self._lead + (self.ns + 4,), dtype=np.int64)
        with torch.cuda.stream(st):
            mask = torch.empty(self._lead + (self.nmask,), dtype=torch.int32, device=self.device)
            if self.ncols:
                (h.checked_batched if self._batched else h.checked)(*lead, int(mask.data_ptr()), st.cuda_stream)
                if self.r:
                    if stream is not None:
                        self.loc.record_stream(stream)
                    counts = torch.empty(host.shape, dtype=torch.int64, device=self.device)
                    (h.checked_fix_batched if self._batched else h.checked_fix)(
                        *lead, int(mask.data_ptr()), int(self.loc.data_ptr()), self.locatable, self.max_errors,
                        int(counts.data_ptr()), st.cuda_stream)
                    host = counts.cpu().numpy()
        ns = self.ns
        fixed = np.zeros(self._lead + (self.n,), dtype=np.int64)
        fixed[..., self.survivors] = host[..., :ns]
        by_weight = np.concatenate([np.zeros_like(host[..., :1]), host[..., ns: ns + 2]], axis=-1)
        report = make_batch_correct_report if self._batched else make_correct_report
        return report(fixed, by_weight, host[..., ns + 2].copy(), host[..., ns + 3].copy(), mask)


class CheckedRepairPlan(_CheckedRepair):
    """A reusable device checked repair of one stripe's buffers; it keeps raw row pointers only, so a
    cache may hand it out only for the caller's live tensors.

    Args:
        rows: the n stripe rows (natives first) on one GPU; the shortest row bounds the columns. No
            row may overlap another. The erased rows are written and never read.
        h: the p x n check matrix over GF(2^8), 1 <= p <= 16.
        erased: the ids of the lost rows, at most p.
        max_errors: 1 or 2 (default ``min(2, r // 2)``, at least 1); 2 needs r >= 4 and at most
            :data:`~gpu_rscode_amd.ops.correct.MAX_PAIR_N` survivors.
        block_bytes: columns per mask word, a power of two >= 4096.
        check: run the aliasing check; False when the caller has.
    """

    _batched = False

    def __init__(self, rows, h: np.ndarray, erased, max_errors: int | None = None, block_bytes: int = 65536, *,
                 check: bool = True):
        h = np.asarray(h, dtype=np.uint8)
        part = stripe_part(rows, "stripe")
        self._build(part, part.nrows, h, erased, max_errors, block_bytes, check)


class BatchCheckedRepairPlan(_CheckedRepair):
    """A reusable device checked repair of B stripes of one shape under ONE erasure list, one launch
    per kernel (grid.y = stripe); raw row pointers only, as :class:`CheckedRepairPlan`.

    Args:
        stripes: B stripes of n rows each as :class:`~gpu_rscode_amd.ops.scrub.BatchScrubPlan` takes
            them. No row may overlap another row of any stripe.
        h, erased, max_errors, block_bytes, check: as :class:`CheckedRepairPlan`.
    """

    _batched = True

    def __init__(self, stripes, h: np.ndarray, erased, max_errors: int | None = None, block_bytes: int = 65536, *,
                 check: bool = True):
        h = np.asarray(h, dtype=np.uint8)
        batch = stripes if isinstance(stripes, StripeBatch) else StripeBatch(stripes, h.shape[1])
        self._build(batch, batch.n, h, erased, max_errors, block_bytes, check)


def cpu_reconstruct_checked(t: np.ndarray, erased: list[int], rows: list[torch.Tensor], ncols: int, block_bytes: int,
                            max_errors: int, cpu_gemm):
    """CPU form on the n ``rows`` of one stripe with ``t`` and ``erased`` from ``gf.checked_matrix``: the
    rebuild as one GEMM of the codec (``cpu_gemm(coeff, ins, outs)``), then
    :func:`~gpu_rscode_amd.ops.correct.cpu_correct` with the check matrix ``T[e:, S]`` on the
    survivors, every fix carried into the erased rows. Returns ``(mask, fixed_bytes, by_weight,
    uncorrectable, bad_columns)``, ``fixed_bytes`` by chunk id."""
    p, n = t.shape
    e, k = len(erased), n - p
    s = [i for i in range(n) if i not in erased]
    block_bytes = check_block_bytes(block_bytes)
    fixed_bytes = np.zeros(n, dtype=np.int64)
    zero = (torch.zeros(-(-ncols // block_bytes), dtype=torch.int32), fixed_bytes, np.zeros(3, dtype=np.int64), 0, 0)
    if ncols == 0:
        return zero
    surv = [rows[j][:ncols] for j in s]
    lost = [rows[j][:ncols] for j in erased]
    if e:
        cpu_gemm(t[:e][:, s[:k]], surv[:k], lost)
    if p == e:
        return zero
    lost_np = [x.numpy() for x in lost]
    mul = mul_table()
    reb = t[:e][:, s]

    def on_fix(j, cols, values):  # survivor j's bytes got ^= values: so do the erased rows, times T[i][j]
        for i in range(e):
            if reb[i, j]:
                lost_np[i][cols] ^= mul[reb[i, j]][values]

    mask, fb, by_weight, uncorrectable, bad = cpu_correct(np.ascontiguousarray(t[e:][:, s]), surv, ncols, block_bytes,
                                                          max_errors, cpu_gemm, on_fix)
    fixed_bytes[s] = fb
    return mask, fixed_bytes, by_weight, uncorrectable, bad
