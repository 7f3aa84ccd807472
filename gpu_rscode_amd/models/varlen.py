"""Variable-length batches: encode, or repair in place, B objects of mixed sizes in ONE launch.

The batched calls of :class:`~gpu_rscode_amd.models.rs.ReedSolomon` take B stripes of one shape. An
object store holds objects of every size; one launch per object is host-bound, padding to the longest
object moves several times the bytes, and bucketing by size is a launch and a plan per bucket.
:class:`VarlenCodec` takes the stripes as they are: stripe b has a chunk length ``C_b >= 0`` of its own
(and, for a repair, erasures of its own), and ``csrc/kernels/gf_varlen.hip`` runs them on a flat grid
of (stripe, column block) work items.
"""
from __future__ import annotations

from functools import cached_property

import numpy as np
import torch

from ..ops.rows import as_rows
from .rs import ReedSolomon


class _Rows:
    """B stripes of r byte rows, stripe b's rows of one length ``lengths[b]``: the list form (a sequence
    of B stripes, each an ``[r, C_b]`` tensor or a list of r rows) or the packed form (one ``[r, T]``
    tensor and B + 1 offsets: stripe b's row j is ``t[j, offsets[b]:offsets[b + 1]]``). ``ptrs`` is the
    uint64 ``[B, r]`` row addresses, ``key`` names every row address and every length."""

    def __init__(self, x, what: str, offsets: np.ndarray | None):
        self.what = what
        if offsets is not None:
            if not isinstance(x, torch.Tensor) or x.dim() != 2:
                raise ValueError(f"{what}: with offsets, expected one [rows, T] tensor")
            _check_tensor(x, what)
            if offsets[-1] > x.shape[1]:
                raise ValueError(f"{what}: offsets end at {int(offsets[-1])}, past rows of {x.shape[1]} bytes")
            self.t, self.offsets, self.stripes = x, offsets, None
            self.nstripes, self.nrows, self.device = offsets.size - 1, int(x.shape[0]), x.device
            # (lengths and ptrs are worked out when a plan is built, not for the key: a repeat call on
            # hundreds of small objects is launch-bound, and the [B, r] addresses took longer than the kernel)
            self.key = ("p", int(x.data_ptr()), tuple(x.shape), tuple(x.stride()), x.device, offsets.tobytes())
            return
        if isinstance(x, torch.Tensor):
            raise ValueError(f"{what}: expected a sequence of stripes, or one [rows, T] tensor with offsets")
        try:
            items = list(x)
        except TypeError:
            raise ValueError(f"{what}: expected a sequence of stripes, or one [rows, T] tensor with offsets") from None
        self.t, self.offsets, self.stripes = None, None, []
        ptrs, lens, self.device, self.nrows = [], [], None, None
        for b, item in enumerate(items):
            if isinstance(item, torch.Tensor):
                if item.dim() != 2:
                    raise ValueError(f"{what}: stripe {b}: expected a [rows, C] tensor or a list of rows")
                _check_tensor(item, f"{what}: stripe {b}")
                rows = [item[j] for j in range(item.shape[0])]
            else:
                try:
                    rows = as_rows(item)
                except TypeError:
                    raise ValueError(f"{what}: stripe {b}: expected a [rows, C] tensor or a list of rows") from None
                for r in rows:
                    if not isinstance(r, torch.Tensor) or r.dim() != 1:
                        raise ValueError(f"{what}: stripe {b}: rows must be 1-D uint8 tensors")
                    _check_tensor(r, f"{what}: stripe {b}")
            if self.nrows is None:
                self.nrows = len(rows)
            elif len(rows) != self.nrows:
                raise ValueError(f"{what}: every stripe must have {self.nrows} rows, stripe {b} has {len(rows)}")
            n = {int(r.numel()) for r in rows}
            if len(n) > 1:
                raise ValueError(f"{what}: stripe {b}: its rows must have one length, got {sorted(n)}")
            for r in rows:
                if self.device is None:
                    self.device = r.device
                elif r.device != self.device:
                    raise ValueError(f"{what}: all rows must live on one device ({self.device} vs {r.device})")
            self.stripes.append(rows)
            ptrs.append([r.data_ptr() for r in rows])
            lens.append(n.pop() if n else 0)
        self.nstripes = len(items)
        self.nrows = self.nrows or 0
        self.device = self.device or torch.device("cpu")
        self.lengths = np.array(lens, dtype=np.int64)
        self.ptrs = np.array(ptrs, dtype=np.uint64).reshape(self.nstripes, self.nrows)
        self.key = ("l", self.ptrs.shape, self.ptrs.tobytes(), self.lengths.tobytes())

    @cached_property
    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets)

    @cached_property
    def ptrs(self) -> np.ndarray:
        row0 = int(self.t.data_ptr()) + np.arange(self.nrows, dtype=np.int64)[None, :] * int(self.t.stride(0))
        return (row0 + self.offsets[:-1, None]).astype(np.uint64)

    def rows(self, b: int) -> list[torch.Tensor]:
        if self.stripes is not None:
            return self.stripes[b]
        lo, hi = int(self.offsets[b]), int(self.offsets[b + 1])
        return [self.t[j, lo:hi] for j in range(self.nrows)]


def _check_tensor(t: torch.Tensor, what: str) -> None:
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: rows must be uint8, got {t.dtype}")
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{what}: rows must be contiguous byte rows (last stride 1)")


def _offsets(offsets) -> np.ndarray | None:
    """``offsets`` as an int64 array of B + 1 non-decreasing values >= 0, or None."""
    if offsets is None:
        return None
    if isinstance(offsets, torch.Tensor):
        if offsets.device.type != "cpu":
            raise ValueError(f"offsets are read on the host and must be a CPU tensor, got {offsets.device}")
        offsets = offsets.numpy()
    try:
        a = np.asarray(offsets)
    except ValueError:
        a = np.empty(0, dtype=object)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
        raise ValueError("offsets must be a 1-D integer sequence of B + 1 values")
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a[0] < 0 or (np.diff(a) < 0).any():
        raise ValueError("offsets must start at 0 or above and must not decrease")
    return a


class VarlenCodec:
    """Encode and repair batches of stripes of differing lengths with one code.

    Args:
        rs: the :class:`~gpu_rscode_amd.models.rs.ReedSolomon` codec: ``gf256`` or ``gf16`` on the
            GPU, any field on CPU tensors. Its matrices, its solved patterns and its plan cache
            (``rs._plans``) are used, so a new ``rs.G`` drops this codec's plans too.

    Every call takes the stripes in one of two forms:

    * *list form*: a sequence of B items, each an ``[r, C_b]`` uint8 tensor (last stride 1) or a list
      of r 1-D rows of one length ``C_b``;
    * *packed form* (``cu_seqlens``): one ``[r, T]`` tensor with ``offsets``, a CPU int64 sequence of
      B + 1 non-decreasing values, ``offsets[0] >= 0`` and ``offsets[-1] <= T``: stripe b's row j is
      ``t[j, offsets[b]:offsets[b + 1]]``. The row addresses come from numpy without a loop over
      stripes, so this is the form for tens of thousands of objects. Offsets that are multiples of
      16 (on 16-byte aligned rows) keep the launch on the vector form; one row of some bytes that is
      not 16-byte aligned puts the whole launch on the slower byte-per-lane form.

    ``C_b >= 0``, any mix; a stripe of length 0 is left alone. Per stripe the result is exactly that of
    ``rs.encode`` / ``rs.reconstruct`` on that stripe alone, and no other byte is touched. On the GPU
    the plan (descriptor, work list, tables) is cached on every row address, every length and the
    erasure ids: a repeat call on the same buffers is key building and the launch, with no host sync
    and no upload. CPU tensors loop over the stripes through ``rs``. Raised before a byte is written:
    ``ValueError`` for wrong row counts, rows of one stripe that differ in length, rows that are not
    uint8 or not contiguous, rows on mixed devices, bad ``offsets``, bad ids, id tensors on a GPU, or a
    written row that overlaps any other row of the batch (so also for a stripe listed twice);
    :class:`~gpu_rscode_amd.models.rs.UnrecoverableError` for more than p erasures or a singular
    pattern, naming the first such stripe; ``NotImplementedError`` for ``gf65536`` on CUDA tensors.
    """

    def __init__(self, rs: ReedSolomon):
        if not isinstance(rs, ReedSolomon):
            raise TypeError("VarlenCodec wraps a ReedSolomon codec")
        self.rs = rs

    # ---- helpers -----------------------------------------------------------------------------
    def _parts(self, what: str, first, first_rows: int, parity, offsets):
        """The first part and the parity part (or None) as :class:`_Rows`, checked against each other.
        ``first`` may be a part already."""
        rs = self.rs
        off = _offsets(offsets)
        a = first if isinstance(first, _Rows) else _Rows(first, what, off)
        if a.nstripes and a.nrows != first_rows:
            raise ValueError(f"{what}: expected {first_rows} rows per stripe, got {a.nrows}")
        if parity is None:
            return a, None
        b = _Rows(parity, "parity", off)
        if b.nstripes != a.nstripes:
            raise ValueError(f"{a.nstripes} stripes of {what} but {b.nstripes} of parity")
        if not a.nstripes:
            return a, b
        if b.nrows != rs.p:
            raise ValueError(f"parity: expected {rs.p} rows per stripe, got {b.nrows}")
        if rs.p and b.device != a.device:
            raise ValueError(f"all rows must live on one device ({a.device} vs {b.device})")
        # (packed parts of one call share their offsets, so their lengths)
        if rs.p and off is None and not np.array_equal(a.lengths, b.lengths):
            s = int(np.nonzero(a.lengths != b.lengths)[0][0])
            raise ValueError(f"stripe {s}: {what} rows of {int(a.lengths[s])} bytes but parity rows of "
                             f"{int(b.lengths[s])}")
        return a, b

    @staticmethod
    def _ptrs(a: _Rows, b: _Rows | None) -> np.ndarray:
        """The uint64 ``[B, rows]`` row addresses of a part and its parity part."""
        return a.ptrs if b is None else np.concatenate([a.ptrs, b.ptrs], axis=1)

    def _check_device(self, part: _Rows) -> bool:
        """True for the kernel, False for the CPU loop."""
        rs = self.rs
        if part.device.type == "cuda":
            if rs.wide:
                raise NotImplementedError("VarlenCodec runs gf256 and gf16 on the GPU, not gf65536")
            return True
        if rs.wide and (part.lengths % 2).any():
            raise ValueError("GF(2^16) rows hold 16-bit symbols: every length must be an even byte count")
        return False

    # The plan-cache keys: a hit runs the plan unexamined, so a key names everything the plan was built
    # from: every row address and every length (``_Rows.key``), and the erasure ids as given.
    @staticmethod
    def _encode_key(data: _Rows, parity: _Rows) -> tuple:
        return ("vlenc", data.key, parity.key)

    @staticmethod
    def _repair_key(stripes: _Rows, parity: _Rows | None, raw: np.ndarray) -> tuple:
        return ("vlrep", stripes.key, None if parity is None else parity.key, raw.shape, raw.tobytes())

    @staticmethod
    def _scrub_key(stripes: _Rows, parity: _Rows | None, block_bytes: int) -> tuple:
        return ("vlscrub", block_bytes, stripes.key, None if parity is None else parity.key)

    def _alloc_parity(self, data: _Rows):
        """Parity in the form of ``data``: packed, a zeroed ``[p, T]`` tensor under the same offsets;
        list, B ``[p, C_b]`` views of one zeroed arena, each stripe's columns starting at a multiple of 16."""
        p = self.rs.p
        if data.offsets is not None:
            return torch.zeros((p, data.t.shape[1]), dtype=torch.uint8, device=data.device)
        width = (data.lengths + 15) // 16 * 16
        start = np.cumsum(width) - width
        arena = torch.zeros((p, int(width.sum())), dtype=torch.uint8, device=data.device)
        return [arena[:, int(s): int(s) + int(c)] for s, c in zip(start, data.lengths)]

    # ---- encode ------------------------------------------------------------------------------
    def encode(self, data, parity=None, offsets=None, stream: torch.cuda.Stream | None = None):
        """``parity_b = E . data_b`` for every stripe b. ``data``: B stripes of k rows, ``parity``: B
        stripes of p rows in the same form (None: allocated in the form of ``data``). Returns
        ``parity``."""
        from ..ops.varlen import VarlenPlan, check_varlen_overlap

        rs = self.rs
        if parity is None:
            data = _Rows(data, "data", _offsets(offsets))
            parity = self._alloc_parity(data)
        d, par = self._parts("data", data, rs.k, parity, offsets)
        if not d.nstripes or rs.p == 0:
            return parity
        kernel = self._check_device(d)
        key = self._encode_key(d, par) if kernel else None
        plan = rs._plans.get(key) if kernel else None
        if plan is not None:
            plan.run(stream)
            return parity
        ptrs, lengths = self._ptrs(d, par), d.lengths
        check_varlen_overlap(ptrs[:, : rs.k], ptrs[:, rs.k:], lengths)
        if kernel:
            maps = rs._maps(rs.E)
            pattern = (tuple(range(rs.k)), tuple(range(rs.k, rs.n)), rs.E if maps is None else maps)
            plan = rs._plans[key] = VarlenPlan(ptrs, lengths, np.zeros(d.nstripes, dtype=np.int64), [pattern],
                                               d.device, check=False)
            plan.run(stream)
            return parity
        for b in np.nonzero(lengths)[0]:
            rs.encode(d.rows(int(b)), par.rows(int(b)))
        return parity

    # ---- repair ------------------------------------------------------------------------------
    def reconstruct(self, stripes, erased, parity=None, offsets=None, stream: torch.cuda.Stream | None = None):
        """In-place repair of every stripe b: rows ``erased_b`` rewritten from the first k rows not
        erased, as ``rs.reconstruct``. ``stripes``: B stripes of n rows, or of k rows with their p
        parity rows in ``parity``. ``erased``: the forms of ``ReedSolomon.reconstruct_batch`` (a flat
        sequence shared by every stripe, B id sequences of 0..p ids, or an integer ``[B, e]`` array or
        CPU tensor padded with -1); an empty list leaves its stripe untouched. Returns ``stripes``."""
        from ..ops.varlen import VarlenPlan, check_varlen_overlap
        from ..ops.repair import repair_rows

        rs = self.rs
        s, par = self._parts("stripes", stripes, rs.n if parity is None else rs.k, parity, offsets)
        raw = rs._erased_raw(erased, rs.n)
        kernel = self._check_device(s)
        key = self._repair_key(s, par, raw) if kernel else None
        plan = rs._plans.get(key) if kernel else None
        if plan is not None:
            plan.run(stream)
            return stripes
        ptrs, lengths = self._ptrs(s, par), s.lengths
        pat, patterns = rs._erased_patterns(raw, s.nstripes)
        pat = np.where(lengths > 0, pat, -1)  # (a stripe of no bytes has nothing to repair)
        keep = pat >= 0
        if not keep.any():
            return stripes
        m_pad = max(len(er) for _, er in patterns)
        check_varlen_overlap(*repair_rows(ptrs[keep], pat[keep], [(sv, er, None) for sv, er in patterns], m_pad),
                             lengths[keep])
        if kernel:
            full = []
            for sv, er in patterns:
                coeff = rs.gf.matmul(rs.G[list(er)], rs.decode_matrix(sv)).astype(rs.G.dtype)
                maps = rs._maps(coeff)
                full.append((sv, er, coeff if maps is None else maps))
            plan = rs._plans[key] = VarlenPlan(ptrs, lengths, pat, full, s.device, check=False)
            plan.run(stream)
            return stripes
        for b in np.nonzero(keep)[0]:
            rows = s.rows(int(b)) + ([] if par is None else par.rows(int(b)))
            rs.reconstruct(rows, patterns[int(pat[b])][1])
        return stripes

    # ---- scrub -------------------------------------------------------------------------------
    def _scrub(self, what: str, stripes, parity, offsets, block_bytes: int, stream, locate: bool):
        """The call behind :meth:`syndrome_mask` and :meth:`scrub` (``locate``): a cached plan on the
        GPU, else zeros (p = 0 or no bytes: nothing to check) or the CPU form stripe by stripe."""
        from ..ops.scrub import MAX_LOCATE_P, check_block_bytes, cpu_scrub
        from ..ops.varlen import VarlenScrubPlan, make_varlen_report, zero_mask

        rs = self.rs
        if rs.field != "gf256":
            raise NotImplementedError(f"{what} is implemented for field='gf256', not {rs.field!r}")
        s, par = self._parts("stripes", stripes, rs.n if parity is None else rs.k, parity, offsets)
        block_bytes = check_block_bytes(block_bytes)
        if s.device.type == "cuda" and rs.p > 0 and s.nstripes > 0:
            key = self._scrub_key(s, par, block_bytes)
            plan = rs._plans.get(key)
            if plan is None and s.lengths.any():  # (a batch of no bytes gets no plan and launches nothing)
                plan = rs._plans[key] = VarlenScrubPlan(self._ptrs(s, par), s.lengths, rs.H, s.device, block_bytes)
            if plan is not None:
                return plan.scrub(stream) if locate else plan.syndrome_mask(stream)  # (scrub refuses p > 16 itself)
        if locate and rs.p > MAX_LOCATE_P:
            raise NotImplementedError(f"{what} locates chunks for p <= {MAX_LOCATE_P} (p = {rs.p}); syndrome_mask "
                                      "works for any p")
        lengths = s.lengths if s.nstripes else np.zeros(0, dtype=np.int64)
        mask = zero_mask(lengths, block_bytes, s.device)
        votes = np.zeros((s.nstripes, rs.n), dtype=np.int64)
        unlocated, bad = np.zeros(s.nstripes, dtype=np.int64), np.zeros(s.nstripes, dtype=np.int64)
        if s.device.type != "cuda" and rs.p > 0:
            h = rs.H
            for b in np.nonzero(lengths)[0]:
                b = int(b)
                rows = s.rows(b) + ([] if par is None else par.rows(b))
                words, votes[b], unlocated[b], bad[b] = cpu_scrub(h, rows, int(lengths[b]), block_bytes, rs._cpu_gemm,
                                                                  locate)
                mask.of(b).copy_(words)
                mask.stripes[b] = int(np.bitwise_or.reduce(words.numpy()))
        return make_varlen_report(votes, unlocated, bad, mask) if locate else mask

    def syndrome_mask(self, stripes, parity=None, offsets=None, block_bytes: int = 65536,
                      stream: torch.cuda.Stream | None = None):
        """``rs.syndrome_mask`` for every stripe b in ONE launch with no host sync: a
        :class:`~gpu_rscode_amd.ops.varlen.VarlenMask` whose ``of(b)`` (``blocks[offsets[b]:offsets[b + 1]]``,
        ``ceil(C_b / block_bytes)`` int32 words on the stripes' device) equals what ``rs.syndrome_mask`` on
        stripe b alone returns, and whose ``stripes[b]`` is the OR of those words. ``stripes``: B stripes
        of n rows, natives first, or of k rows with their p parity rows in ``parity``. A stripe of
        length 0 has no words and a zero stripe word; a batch of nothing but such stripes launches
        nothing. Any p; no row is written."""
        return self._scrub("syndrome_mask", stripes, parity, offsets, block_bytes, stream, False)

    def scrub(self, stripes, parity=None, offsets=None, block_bytes: int = 65536,
              stream: torch.cuda.Stream | None = None):
        """``rs.scrub`` for every stripe b: on the GPU one launch of each kernel and one sync for the
        whole batch. Returns a :class:`~gpu_rscode_amd.ops.varlen.VarlenScrubReport`: the fields of
        ``BatchScrubReport`` with ``mask`` a ``VarlenMask``; ``report[b]`` equals, field for field, what
        ``rs.scrub`` on stripe b alone returns. p > 16 raises ``NotImplementedError``. No row is written."""
        return self._scrub("scrub", stripes, parity, offsets, block_bytes, stream, True)

    def heal(self, stripes, parity=None, offsets=None, report=None):
        """Repair the dirty stripes of the batch in place, each from its own redundancy, by
        ``rs.heal_batch``'s rule stripe by stripe. Scrubs if no ``report`` is given. A dirty stripe with
        no unlocated column, 1..p suspects and a recoverable pattern is rewritten as
        ``rs.reconstruct(stripe_b, erased=suspects_b)`` would, all such stripes in ONE
        :meth:`reconstruct` call; any other dirty stripe is left byte for byte as it was and listed in
        ``unhealed``, and nothing is raised for it. If anything was rewritten the batch is scrubbed
        once more and that second report is returned, else the first; either has ``unhealed`` filled in."""
        rs = self.rs
        if rs.field != "gf256":
            raise NotImplementedError(f"heal is implemented for field='gf256', not {rs.field!r}")
        if report is None:
            report = self.scrub(stripes, parity, offsets)
        unhealed = []
        erased = np.full((len(report.clean), rs.p), -1, dtype=np.int64)
        for b in report.dirty:
            rep = report.report[b]
            sus = sorted(set(int(e) for e in rep.suspects))
            if (rep.unlocated > 0 or not sus or len(sus) > rs.p
                    or not rs.is_recoverable([i for i in range(rs.n) if i not in sus][: rs.k])):
                unhealed.append(b)  # (nothing is written)
                continue
            erased[b, : len(sus)] = sus
        if (erased >= 0).any():
            self.reconstruct(stripes, erased, parity, offsets)
            report = self.scrub(stripes, parity, offsets)
        report.unhealed = unhealed
        return report
