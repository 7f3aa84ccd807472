"""In-place parity update for partial-stripe writes (``csrc/kernels/gf_update.hip``).

Over GF(2^w) the parity of a stripe is linear in its natives, so when natives ``changed[t]`` go from
``old[t]`` to ``new[t]`` every parity row moves by ``E[i][changed[t]] . (old[t] ^ new[t])``: the
update needs the changed natives and the parity rows, not the other ``k - d`` natives, and the
delta ``old ^ new`` is what a data node ships to a parity node. :class:`UpdatePlan` holds the
device descriptors of that kernel (at most :data:`MAX_D` changed rows per launch, longer lists in
passes); :func:`cpu_update` is the host form over the codec's C++ GEMM.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import hip
from .gemm import _check_rows, _rows, build_desc, pad_m, perm_tables_from_coeff, perm_tables_from_maps

MAX_D = 8  # kUpdateMaxD: changed rows per launch (32 VGPRs of deltas per lane)
_CPU_SCRATCH = 64 << 20  # bytes of scratch rows of the CPU form


def check_overlap(parity, first, second=None, first_written: bool = False) -> None:
    """ValueError when, by address range, a parity row overlaps another parity row or any
    ``first`` (old / delta) or ``second`` (new) row, or a ``second`` row overlaps a ``first`` row; with
    ``first_written`` (a write stores into the old rows) also when two ``first`` rows overlap. The
    kernel's read-modify-write is per lane and in place: it is wrong under such aliasing."""
    spans = []
    for tag, rows in (("parity", parity), ("old", first), ("new", second or [])):
        for i, r in enumerate(rows):
            if r.numel():
                a = int(r.data_ptr())
                spans.append((a, a + r.numel(), tag, i))
    spans.sort()
    for x, (a0, a1, ta, ia) in enumerate(spans):
        for b0, _, tb, ib in spans[x + 1:]:
            if b0 >= a1:
                break
            kinds = {ta, tb}
            if "parity" in kinds or kinds == {"old", "new"} or (first_written and kinds == {"old"}):
                raise ValueError(f"{ta} row {ia} and {tb} row {ib} overlap in memory: the parity update works "
                                 "in place and needs disjoint rows")


def _window(col0: int, ncols: int | None, limit: int) -> tuple[int, int]:
    col0 = int(col0)
    ncols = limit - col0 if ncols is None else int(ncols)
    if col0 < 0 or ncols < 0 or col0 + ncols > limit:
        raise ValueError(f"column range [{col0}, {col0 + ncols}) outside rows of {limit} bytes")
    return col0, ncols


class UpdatePlan:
    """A reusable device parity update, as ``ScrubPlan``: it keeps raw row pointers only, so a cache
    may hand it out only for the caller's live tensors.

    Args:
        parity: the p parity rows on one GPU, updated in place.
        old_or_delta: d rows: the natives' old contents (with ``new``) or the deltas ``old ^ new``.
        new: d rows with the natives' new contents, or None for the delta form.
        coeff: the p x d coefficients ``E[:, changed]`` over GF(2^8); or
        maps: (p, d, 256) GF(2)-linear byte maps (the GF(16) nibble maps).
        store_new: also overwrite ``old_or_delta[t]`` with ``new[t]`` in the same pass (a write into a
            stripe). Needs ``new``.
    """

    def __init__(self, parity, old_or_delta, new=None, coeff=None, *, maps=None, store_new: bool = False):
        par, first = _rows(parity), _rows(old_or_delta)
        second = None if new is None else _rows(new)
        if store_new and second is None:
            raise ValueError("store_new needs the new rows (the pair form)")
        self.p, self.d = len(par), len(first)
        if not 1 <= self.p <= 255 or self.d < 1:
            raise ValueError("UpdatePlan needs 1..255 parity rows and at least one changed row")
        if second is not None and len(second) != self.d:
            raise ValueError(f"expected {self.d} new rows, got {len(second)}")
        dev = _check_rows(par, "parity", None)
        dev = _check_rows(first, "old" if second is not None else "delta", dev)
        if second is not None:
            dev = _check_rows(second, "new", dev)
        if dev.type != "cuda":
            raise ValueError("UpdatePlan runs on a GPU")
        self.device = dev
        check_overlap(par, first, second, store_new)
        if coeff is not None:
            tables = perm_tables_from_coeff(np.asarray(coeff, dtype=np.uint8).reshape(self.p, self.d))
        elif maps is not None:
            tables = perm_tables_from_maps(maps)
            if tables.shape[:2] != (self.p, self.d):
                raise ValueError(f"maps must be ({self.p}, {self.d}, 256)")
        else:
            raise ValueError("need coeff or maps")
        self.pairs, self.store_new = second is not None, bool(store_new)
        self.m_pad = pad_m(self.p)
        rows = par + first + (second or [])
        self.ncols = min(r.numel() for r in rows)
        ptr = lambda t: int(t.data_ptr())  # noqa: E731
        self.bytewise = any(ptr(r) % 16 for r in rows)
        # one descriptor per pass of at most MAX_D changed rows: in = old / delta, copy = new, out =
        # parity, tables of E[:, changed[pass]] (XOR accumulation makes the passes independent)
        self.passes = []
        for t0 in range(0, self.d, MAX_D):
            t1 = min(self.d, t0 + MAX_D)
            host = build_desc([ptr(r) for r in first[t0:t1]], [ptr(r) for r in par],
                              None if second is None else [ptr(r) for r in second[t0:t1]], tables[:, t0:t1])
            self.passes.append((t1 - t0, torch.from_numpy(host).to(self.device)))
        self._ready = torch.cuda.Event()
        self._ready.record(torch.cuda.current_stream(self.device))

    def run(self, stream: torch.cuda.Stream | None = None, col0: int = 0, ncols: int | None = None) -> None:
        """Launch over byte columns ``[col0, col0 + ncols)`` (default: to the end of the shortest row)
        on ``stream`` (default: the current stream). No host sync."""
        col0, ncols = _window(col0, ncols, self.ncols)
        st = stream or torch.cuda.current_stream(self.device)
        if self._ready is not None:
            st.wait_event(self._ready)
            self._ready = None
        bytewise = self.bytewise or col0 % 16 != 0
        for d, desc in self.passes:
            if stream is not None:
                desc.record_stream(stream)
            hip().update(int(desc.data_ptr()), d, self.m_pad, col0, ncols, self.pairs, self.store_new, bytewise,
                         st.cuda_stream)


def cpu_update(coeff: np.ndarray, parity, first, second, col0: int, ncols: int, cpu_gemm, store_new: bool = False,
               ) -> None:
    """CPU form: the delta by torch XOR, ``coeff . delta`` into p bounded scratch rows slice by slice
    (``cpu_gemm(coeff, ins, outs)`` is the codec's GEMM, as :func:`~gpu_rscode_amd.ops.scrub.cpu_scrub`
    takes it), XORed into ``parity``. ``coeff`` is the p x d block ``E[:, changed]``."""
    p, d = len(parity), len(first)
    if p and ncols:
        step = max(4096, min(1 << 20, _CPU_SCRATCH // (p + d) // 64 * 64))
        scratch = torch.empty((p, step), dtype=torch.uint8)
        dscratch = torch.empty((d, step), dtype=torch.uint8) if second is not None else None
        for c0 in range(col0, col0 + ncols, step):
            c1 = min(col0 + ncols, c0 + step)
            if second is not None:
                ins = [dscratch[t, : c1 - c0] for t in range(d)]
                for t in range(d):
                    torch.bitwise_xor(first[t][c0:c1], second[t][c0:c1], out=ins[t])
            else:
                ins = [r[c0:c1] for r in first]
            outs = [scratch[i, : c1 - c0] for i in range(p)]
            cpu_gemm(coeff, ins, outs)
            for i in range(p):
                parity[i][c0:c1].bitwise_xor_(outs[i])
    if store_new:
        for t in range(d):
            first[t][col0: col0 + ncols].copy_(second[t][col0: col0 + ncols])
