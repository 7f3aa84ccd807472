"""Batched in-place repair (``csrc/kernels/gf_repair.hip``): B stripes of one shape per launch, each
with an erasure pattern of its own.

Repairing a stripe is one GF-GEMM, ``rows[erased] = G[erased] . inv(G[survivors]) . rows[survivors]``,
and its coefficients depend on the whole pattern. Objects placed over different node sets lose
different chunks, so the stripes of a rebuild batch do not share a coefficient matrix: the descriptor
holds one table block per DISTINCT pattern and one pattern index per stripe, and the kernel picks the
block by the index it reads per stripe. :class:`BatchRepairPlan` holds that descriptor;
:func:`repair_rows` resolves chunk ids into row addresses with numpy, without a loop over stripes.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import hip
from .gemm import pad_m, perm_tables_from_coeff, perm_tables_from_maps, plan_stream, ready_event
from .rows import StripeBatch, batch_part
from .update import check_overlap_batch


def repair_batch_layout(k: int, m_pad: int, batch: int, npat: int) -> dict:
    """Mirror of ``gfrs::repair_batch_layout`` (``csrc/include/gfrs/desc.h``); a test pins the two equal."""
    in_off = 16
    out_off = in_off + 8 * k * batch
    pat_off = out_off + 8 * m_pad * batch
    tab_off = (pat_off + 4 * batch + 31) // 32 * 32
    return dict(in_off=in_off, out_off=out_off, pat_off=pat_off, tab_off=tab_off,
                bytes=tab_off + 32 * npat * k * m_pad)


def build_repair_batch_desc(in_ptrs: np.ndarray, out_ptrs: np.ndarray, pat: np.ndarray, tables: np.ndarray) -> np.ndarray:
    """Descriptor bytes of one batched repair: ``in_ptrs`` uint64 ``[B, k]`` survivor row addresses,
    ``out_ptrs`` uint64 ``[B, m_pad]`` addresses of the rows to rewrite (0 = none), ``pat`` int ``[B]``
    in ``[0, npat)``, ``tables`` the ``(npat, k, m_pad, 8)`` uint32 v_perm records (zero past a
    pattern's own erasures)."""
    batch, k = in_ptrs.shape
    npat, _, mp = (int(v) for v in tables.shape[:3])
    lay = repair_batch_layout(k, mp, batch, npat)
    buf = np.zeros(lay["bytes"], dtype=np.uint8)

    def put(off, a, dt):
        raw = np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8)
        buf[off: off + raw.size] = raw

    put(0, np.array([k, mp, batch, npat]), "<i4")
    put(lay["in_off"], in_ptrs, "<u8")
    put(lay["out_off"], out_ptrs, "<u8")
    put(lay["pat_off"], pat, "<i4")
    put(lay["tab_off"], tables, "<u4")
    return buf


def repair_tables(patterns, k: int, m_pad: int) -> np.ndarray:
    """The table blocks ``(npat, k, m_pad, 8)`` of ``patterns[q] = (survivors, erased, coeff)``:
    ``coeff`` an ``e x k`` GF(2^8) matrix or ``(e, k, 256)`` byte maps; rows ``i >= e`` stay zero."""
    tab = np.zeros((len(patterns), k, m_pad, 8), dtype=np.uint32)
    for q, (_, erased, coeff) in enumerate(patterns):
        coeff = np.asarray(coeff)
        t = perm_tables_from_maps(coeff) if coeff.ndim == 3 else perm_tables_from_coeff(coeff.astype(np.uint8))
        if t.shape[:2] != (len(erased), k):
            raise ValueError(f"pattern {q}: coefficients must be {len(erased)} x {k}, got {t.shape[0]} x {t.shape[1]}")
        tab[q, :, : len(erased)] = np.transpose(t, (1, 0, 2))
    return tab


def pattern_ids(patterns, m_pad: int) -> tuple[np.ndarray, np.ndarray]:
    """The id arrays of ``patterns[q] = (survivors, erased, ...)``: int32 ``[npat, k]`` survivors and
    int32 ``[npat, m_pad]`` erased ids padded with -1 (what :func:`solve_patterns` takes)."""
    surv = np.array([list(p[0]) for p in patterns], dtype=np.int32).reshape(len(patterns), -1)
    er = np.full((len(patterns), m_pad), -1, dtype=np.int32)
    for q, p in enumerate(patterns):
        er[q, : len(p[1])] = list(p[1])
    return surv, er


def solve_patterns(g_dev: torch.Tensor, surv: torch.Tensor, erased: torch.Tensor, m_pad: int, *,
                   coeff_out: torch.Tensor | None = None, tables_out: torch.Tensor | None = None,
                   stream: torch.cuda.Stream | None = None) -> torch.Tensor:
    """Solve erasure patterns on the device (``csrc/kernels/gf_repair_solve.hip``), one workgroup per
    pattern in one launch, no host work per pattern.

    ``g_dev``: the ``(n, k)`` uint8 generator ``[I; E]`` on the GPU. ``surv``: int32 ``[npat, k]`` on
    the same device, each pattern's survivors in the order of its coefficient columns. ``erased``:
    int32 ``[npat, m_pad]``, the rows to rewrite, padded with -1. ``coeff_out``: uint8, at least
    ``npat * m_pad * k`` elements, contiguous: pattern q's ``m_pad x k`` block of
    ``G[erased_q] . inv(G[surv_q])``, zero rows at the padding. ``tables_out``: a contiguous device
    tensor whose first ``npat * k * m_pad * 32`` bytes are the ``(npat, k, m_pad, 8)`` uint32 v_perm
    records: the table block of a ``repair_batch_layout`` descriptor (or of a
    :class:`~gpu_rscode_amd.ops.gemm.GemmPlan` descriptor, one pattern). Either may be None. Returns
    the int32 ``[npat]`` device status: 0 built, 1 singular, 2 invalid lists; a pattern whose status
    is not 0 leaves its blocks untouched. Asynchronous on ``stream`` (default: the current one); a
    shape whose system does not fit one workgroup's LDS raises ``NotImplementedError``."""
    if g_dev.dtype != torch.uint8 or g_dev.dim() != 2 or not g_dev.is_cuda or not g_dev.is_contiguous():
        raise ValueError("g_dev must be a contiguous 2-D uint8 tensor on a GPU")
    n, k = (int(v) for v in g_dev.shape)
    dev = g_dev.device
    for name, t, width in (("surv", surv, k), ("erased", erased, m_pad)):
        if t.dtype != torch.int32 or t.device != dev or t.dim() != 2 or t.shape[1] != width or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 [npat, {width}] tensor on {dev}")
    npat = int(surv.shape[0])
    if erased.shape[0] != npat:
        raise ValueError(f"{npat} survivor lists but {erased.shape[0]} erased lists")
    lds = hip().repair_solve_lds_bytes(n, k, m_pad)
    if lds < 0:
        raise ValueError(f"solve_patterns needs 1 <= k <= n <= 256 and 1 <= m_pad <= 256, got ({k}, {n}), m_pad {m_pad}")
    if lds > 65536:
        raise NotImplementedError(f"the ({k}, {n}) repair system with m_pad {m_pad} needs {lds} bytes of LDS")
    for name, t, need, dt in (("coeff_out", coeff_out, npat * m_pad * k, (torch.uint8,)),
                              ("tables_out", tables_out, npat * k * m_pad * 32, None)):
        if t is None:
            continue
        if t.device != dev or not t.is_contiguous() or (dt and t.dtype not in dt) or t.numel() * t.element_size() < need:
            raise ValueError(f"{name} must be a contiguous tensor on {dev} of at least {need} bytes")
    status = torch.empty(npat, dtype=torch.int32, device=dev)
    st = stream or torch.cuda.current_stream(dev)
    hip().repair_solve(g_dev.data_ptr(), n, k, surv.data_ptr(), erased.data_ptr(), npat, m_pad,
                       0 if coeff_out is None else coeff_out.data_ptr(),
                       0 if tables_out is None else tables_out.data_ptr(), status.data_ptr(), st.cuda_stream)
    if stream is not None:
        for t in (g_dev, surv, erased, coeff_out, tables_out, status):
            if t is not None:
                t.record_stream(stream)
    return status


def repair_rows(ptrs: np.ndarray, pat: np.ndarray, patterns, m_pad: int) -> tuple[np.ndarray, np.ndarray]:
    """Row addresses of a batched repair: ``ptrs`` the uint64 ``[B, n]`` row addresses of the stripes
    that take part, ``pat`` their ``[B]`` pattern indices. Returns (survivor rows ``[B, k]`` in the
    order of each pattern's survivors, rows to rewrite ``[B, m_pad]`` with 0 where a pattern has fewer
    erasures). numpy ``take`` only: no loop over stripes."""
    surv = np.array([list(s) for s, _, _ in patterns], dtype=np.int64).reshape(len(patterns), -1)
    er = np.full((len(patterns), m_pad), -1, dtype=np.int64)
    for q, (_, erased, _) in enumerate(patterns):
        er[q, : len(erased)] = list(erased)
    ins = np.take_along_axis(ptrs, surv[pat], axis=1)
    idx = er[pat]
    outs = np.where(idx >= 0, np.take_along_axis(ptrs, np.maximum(idx, 0), axis=1), np.uint64(0)).astype(np.uint64)
    return ins, outs


def check_repair_overlap(ins: np.ndarray, outs: np.ndarray, ncols: int) -> None:
    """The aliasing rule of a batched repair through :func:`~gpu_rscode_amd.ops.update.check_overlap_batch`:
    the written rows play "parity" and the survivor rows "old", so no written row may overlap any
    other used row of any stripe (which also refuses a stripe listed twice with something to write),
    while survivor rows may alias each other. Padding entries (address 0) are rows of no bytes."""
    try:
        check_overlap_batch(outs, ins, None, ncols if outs.all() else [np.where(outs != 0, ncols, 0), ncols])
    except ValueError as e:
        raise ValueError(f"a row to rewrite overlaps another row the batch uses: the repair works in place and "
                         f"needs disjoint rows ({e})") from None


class BatchRepairPlan:
    """A reusable device repair of B stripes of one shape in one launch (grid.y = stripe), each stripe
    under a pattern of its own. As :class:`~gpu_rscode_amd.ops.update.BatchUpdatePlan` it keeps raw row
    pointers only, so a cache may hand it out only for the caller's live tensors.

    Args:
        stripes: a :class:`~gpu_rscode_amd.ops.rows.StripeBatch`, or anything ``StripeBatch(stripes, n)``
            takes with n the rows per stripe it has: ``[B, n, C]`` or a sequence of B stripes.
        pat: int ``[B]``: the pattern of stripe b; -1 = the stripe is not touched (it is dropped from
            the launch, so its rows are never read).
        patterns: ``patterns[q] = (survivors_q, erased_q, coeff_q)``: k chunk ids, 1..m chunk ids, and
            the ``e_q x k`` coefficients ``G[erased] . inv(G[survivors])`` over GF(2^8) or ``(e_q, k,
            256)`` GF(2)-linear byte maps (the GF(16) nibble maps).
        check: run the aliasing check (:func:`check_repair_overlap`); False when the caller has.
        g_dev: the ``(n, k)`` uint8 generator on the stripes' device. With it every pattern is given as
            ``(survivors_q, erased_q, None)`` and no coefficients come from the host: the descriptor is
            uploaded with zeroed table blocks and :func:`solve_patterns` writes them in place, launched
            on the current stream after the upload. The statuses are read back once, here (the only
            host sync; :meth:`run` has none and is ordered after the solve by the plan's ready event),
            and kept as ``status`` (int numpy ``[npat]``: 0 built, 1 singular, 2 invalid). A plan with a
            nonzero status must not be run: the caller checks ``status`` first.
    """

    def __init__(self, stripes, pat, patterns, *, check: bool = True, g_dev: torch.Tensor | None = None):
        if not isinstance(stripes, StripeBatch):
            part = batch_part(stripes, "stripes")
            stripes = StripeBatch(part, part.nrows)
        n = stripes.n
        pat = np.asarray(pat, dtype=np.int64).reshape(-1)
        if pat.shape[0] != stripes.nstripes:
            raise ValueError(f"{stripes.nstripes} stripes but {pat.shape[0]} pattern indices")
        patterns = [(tuple(int(s) for s in sv), tuple(int(e) for e in er), co) for sv, er, co in patterns]
        if not patterns:
            raise ValueError("BatchRepairPlan needs at least one pattern")
        if pat.size and (pat.min() < -1 or pat.max() >= len(patterns)):
            raise ValueError(f"pattern indices must lie in [-1, {len(patterns)})")
        self.k = len(patterns[0][0])
        for q, (sv, er, _) in enumerate(patterns):
            ids = sv + er
            if len(sv) != self.k or not er or len(set(ids)) != len(ids) or min(ids) < 0 or max(ids) >= n:
                raise ValueError(f"pattern {q}: need {self.k} survivor ids and 1.. erased ids, distinct, in [0, {n})")
        if not 1 <= self.k <= 256 or max(len(er) for _, er, _ in patterns) > 256:
            raise ValueError("BatchRepairPlan supports 1 <= k <= 256 and at most 256 erasures")
        self.device = stripes.device
        if stripes.nstripes and self.device.type != "cuda":
            raise ValueError("BatchRepairPlan runs on a GPU")
        self.npat, self.ncols = len(patterns), stripes.ncols
        self.m_pad = pad_m(max(len(er) for _, er, _ in patterns))
        keep = pat >= 0
        self.batch = int(keep.sum())
        self.bytewise, self.desc, self._ready = False, None, None
        self.status, self._unsolved = np.zeros(self.npat, dtype=np.int32), False
        if g_dev is not None:
            if any(co is not None for _, _, co in patterns):
                raise ValueError("with g_dev the patterns carry no coefficients: (survivors, erased, None)")
            if tuple(g_dev.shape) != (n, self.k) or g_dev.device != self.device:
                raise ValueError(f"g_dev must be the ({n}, {self.k}) generator on {self.device}")
        elif any(co is None for _, _, co in patterns):
            raise ValueError("patterns without coefficients need g_dev")
        if not self.batch:
            return
        ins, outs = repair_rows(stripes.ptrs()[keep], pat[keep], patterns, self.m_pad)
        if check:
            check_repair_overlap(ins, outs, self.ncols)
        # one unaligned row: the whole batch bytewise (a padding entry, 0, is aligned)
        self.bytewise = bool((ins % np.uint64(16)).any() or (outs % np.uint64(16)).any())
        if g_dev is None:
            tables = repair_tables(patterns, self.k, self.m_pad)
        else:  # zeroed blocks, filled by the solve below
            tables = np.zeros((self.npat, self.k, self.m_pad, 8), dtype=np.uint32)
        host = build_repair_batch_desc(ins, outs, pat[keep], tables)
        self.desc = torch.from_numpy(host).to(self.device)
        if g_dev is not None:
            surv, er = pattern_ids(patterns, self.m_pad)
            ids = torch.from_numpy(np.concatenate([surv.reshape(-1), er.reshape(-1)])).to(self.device)
            tab_off = repair_batch_layout(self.k, self.m_pad, self.batch, self.npat)["tab_off"]
            status = solve_patterns(g_dev, ids[: surv.size].view(self.npat, self.k),
                                    ids[surv.size:].view(self.npat, self.m_pad), self.m_pad,
                                    tables_out=self.desc[tab_off:])
            self.status = status.cpu().numpy()  # the one sync of a device-solved plan
            self._unsolved = bool(self.status.any())
        self._ready = ready_event(self.device)

    def run(self, stream: torch.cuda.Stream | None = None) -> None:
        """Launch over the whole rows on ``stream`` (default: the current stream). No host sync."""
        if not self.batch or not self.ncols:
            return
        if self._unsolved:
            raise RuntimeError(f"pattern {int(np.nonzero(self.status)[0][0])} was not solved: its table block is empty")
        st = plan_stream(self, stream)
        if stream is not None:
            self.desc.record_stream(stream)
        hip().repair_batched(int(self.desc.data_ptr()), self.k, self.m_pad, self.batch, self.npat, self.ncols,
                             self.bytewise, st.cuda_stream)
