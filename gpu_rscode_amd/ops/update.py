"""In-place parity update for partial-stripe writes (``csrc/kernels/gf_update.hip``).

Over GF(2^w) the parity of a stripe is linear in its natives, so when natives ``changed[t]`` go from
``old[t]`` to ``new[t]`` every parity row moves by ``E[i][changed[t]] . (old[t] ^ new[t])``: the
update needs the changed natives and the parity rows, not the other ``k - d`` natives, and the
delta ``old ^ new`` is what a data node ships to a parity node. :class:`UpdatePlan` holds the
device descriptors of that kernel (at most :data:`MAX_D` changed rows per launch, longer lists in
passes); :func:`cpu_update` is the host form over the codec's C++ GEMM. :class:`BatchUpdatePlan` is
the same for B stripes of one shape per launch (small objects), each stripe changing natives of its
own: the kernel picks its coefficient maps by the ids it reads per stripe.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import hip
from .gemm import build_desc, pad_m, perm_tables_from_coeff, perm_tables_from_maps, plan_stream, ready_event
from .rows import as_rows, batch_part, check_parts, check_rows, window

MAX_D = 8  # kUpdateMaxD: changed rows per launch (32 VGPRs of deltas per lane)
_CPU_SCRATCH = 64 << 20  # bytes of scratch rows of the CPU form


def check_overlap(parity, first, second=None, first_written: bool = False) -> None:
    """ValueError when, by address range, a parity row overlaps another parity row or any
    ``first`` (old / delta) or ``second`` (new) row, or a ``second`` row overlaps a ``first`` row; with
    ``first_written`` (a write stores into the old rows) also when two ``first`` rows overlap. The
    kernel's read-modify-write is per lane and in place: it is wrong under such aliasing. This is
    the rule of :func:`check_overlap_batch` for one stripe's lists of row tensors, each row of its own
    length, kept as a loop over sorted spans: on the half dozen rows of a single update the array form
    costs a fifth of the whole first call. ``tests/test_rows.py`` holds the two to one verdict."""
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


class _Update:
    """What :class:`UpdatePlan` and :class:`BatchUpdatePlan` share once built: ``passes``, a list of
    ``(d, descriptor)``, and how they are launched. A subclass has ``_launch``."""

    def run(self, stream: torch.cuda.Stream | None = None, col0: int = 0, ncols: int | None = None) -> None:
        """Launch over byte columns ``[col0, col0 + ncols)`` of every stripe (default: to the end of
        the shortest row) on ``stream`` (default: the current stream). No host sync."""
        col0, ncols = window(col0, ncols, self.ncols)
        st = plan_stream(self, stream)
        bytewise = self.bytewise or col0 % 16 != 0
        for d, desc in self.passes:
            if stream is not None:
                desc.record_stream(stream)
            self._launch(int(desc.data_ptr()), d, col0, ncols, bytewise, st.cuda_stream)


class UpdatePlan(_Update):
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
        par, first = as_rows(parity), as_rows(old_or_delta)
        second = None if new is None else as_rows(new)
        if store_new and second is None:
            raise ValueError("store_new needs the new rows (the pair form)")
        self.p, self.d = len(par), len(first)
        if not 1 <= self.p <= 255 or self.d < 1:
            raise ValueError("UpdatePlan needs 1..255 parity rows and at least one changed row")
        if second is not None and len(second) != self.d:
            raise ValueError(f"expected {self.d} new rows, got {len(second)}")
        dev = check_rows(par, "parity", None)
        dev = check_rows(first, "old" if second is not None else "delta", dev)
        if second is not None:
            dev = check_rows(second, "new", dev)
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
        self._ready = ready_event(self.device)

    def _launch(self, desc: int, d: int, col0: int, ncols: int, bytewise: bool, stream: int) -> None:
        hip().update(desc, d, self.m_pad, col0, ncols, self.pairs, self.store_new, bytewise, stream)


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


# ---- batched update: B stripes of one shape per launch, d changed natives of its own each --------
def update_batch_layout(k: int, d: int, m_pad: int, batch: int) -> dict:
    """Mirror of ``gfrs::update_batch_layout`` (``csrc/include/gfrs/desc.h``); a test pins the two equal."""
    in_off = 16
    copy_off = in_off + 8 * d * batch
    out_off = copy_off + 8 * d * batch
    ids_off = out_off + 8 * m_pad * batch
    tab_off = (ids_off + 4 * d * batch + 31) // 32 * 32
    return dict(in_off=in_off, copy_off=copy_off, out_off=out_off, ids_off=ids_off, tab_off=tab_off,
                bytes=tab_off + 32 * k * m_pad)


def build_update_batch_desc(ids: np.ndarray, first: np.ndarray, second: np.ndarray | None, parity: np.ndarray,
                            tables: np.ndarray) -> np.ndarray:
    """Descriptor bytes of one batched launch: ``ids`` int ``[B, d]``, ``first`` / ``second`` uint64 row
    addresses ``[B, d]`` (``second`` None in the delta form), ``parity`` ``[B, p]``, ``tables`` the
    (p, k, 8) uint32 v_perm records of the whole code."""
    batch, d = ids.shape
    p, k = tables.shape[:2]
    mp = pad_m(p)
    lay = update_batch_layout(k, d, mp, batch)
    buf = np.zeros(lay["bytes"], dtype=np.uint8)

    def put(off, a, dt):
        raw = np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8)
        buf[off: off + raw.size] = raw

    put(0, np.array([k, d, mp, batch]), "<i4")
    put(lay["in_off"], first, "<u8")
    if second is not None:
        put(lay["copy_off"], second, "<u8")
    out = np.zeros((batch, mp), dtype="<u8")
    out[:, :p] = parity
    put(lay["out_off"], out, "<u8")
    put(lay["ids_off"], ids, "<i4")
    t = np.zeros((k, mp, 8), dtype="<u4")
    t[:, :p, :] = np.transpose(np.asarray(tables, dtype=np.uint32), (1, 0, 2))
    put(lay["tab_off"], t, "<u4")
    return buf


def batch_ids(changed, nstripes: int, k: int, what: str = "changed") -> np.ndarray:
    """The changed natives of a batch as a validated int32 ``[B, d]`` array. ``changed``: a sequence of
    d ids (every stripe changes the same natives) or ``[B, d]`` ids as a nested list, an integer numpy
    array or a CPU integer tensor; each row 1..k distinct ids in ``[0, k)``, any order. Ids are
    validated on the host, so a CUDA tensor is refused. Anything else raises ``ValueError``."""
    if isinstance(changed, torch.Tensor):
        if changed.device.type != "cpu":
            raise ValueError(f"{what}: ids are validated on the host and must be a CPU tensor, got {changed.device}")
        if changed.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"{what}: ids must be integers, got {changed.dtype}")
        a = changed.numpy()
    else:
        try:
            a = np.asarray(changed)
        except ValueError:  # a ragged nested list
            raise ValueError(f"{what}: every stripe must list the same number of ids") from None
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"{what}: expected d ids or [B, d] ids (integers, one d for every stripe)")
    if a.ndim == 1:
        a = np.broadcast_to(a, (nstripes, a.shape[0]))
    if a.ndim != 2 or a.shape[0] != nstripes:
        raise ValueError(f"{what}: expected d ids or [{nstripes}, d] ids, got shape {tuple(a.shape)}")
    d = a.shape[1]
    if not 1 <= d <= k:
        raise ValueError(f"{what}: each stripe changes 1..k={k} natives, got {d}")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= k):
        raise ValueError(f"{what}: ids must lie in [0, {k})")
    srt = np.sort(a, axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
    if dup.any():
        b = int(np.nonzero(dup)[0][0])
        raise ValueError(f"{what}: stripe {b} lists a native twice: {a[b].tolist()}")
    return np.ascontiguousarray(a, dtype=np.int32)


_KINDS = ("parity", "old", "new")


def check_overlap_batch(parity: np.ndarray, first: np.ndarray, second: np.ndarray | None, ncols,
                        first_written: bool = False) -> None:
    """The aliasing rule, on uint64 ``[B, rows]`` address arrays: ValueError when, by address range, a
    parity row overlaps any other row of any stripe (so also for a stripe listed twice), a ``second``
    (new) row overlaps a ``first`` (old / delta) row, or, with ``first_written`` (a write stores into
    the old rows), two ``first`` rows overlap. The kernel's read-modify-write is per lane and in
    place: it is wrong under such aliasing. ``ncols`` is the rows' one length, or a list with one
    entry per address array given: that array's row length, or the array of its rows' lengths (the
    form the single-stripe rule, :func:`check_overlap`, is tested against). Rows of no bytes overlap nothing. The
    spans are sorted by start and each start compared with the running maximum end of the spans
    before it; the kinds are looked at only if something overlaps."""
    groups = [np.asarray(g) for g in (parity, first, second) if g is not None]
    lens = list(ncols) if isinstance(ncols, (list, tuple)) else [ncols] * len(groups)
    start = np.concatenate([g.reshape(-1) for g in groups]).astype(np.int64)
    order = np.argsort(start, kind="stable")
    s = start[order]
    if all(np.ndim(n) == 0 for n in lens) and len(set(int(n) for n in lens)) == 1:
        e = s + int(lens[0])
    else:
        e = s + np.concatenate([np.full(g.size, n) if np.ndim(n) == 0 else np.asarray(n).reshape(-1)
                                for g, n in zip(groups, lens)])[order]
    if not (s[1:] < np.maximum.accumulate(e)[:-1]).any():
        return
    lowest = np.iinfo(np.int64).min

    def reach(sel):  # does span i, of some bytes, start inside a span of `sel` that comes before it in start order?
        end = np.where(sel, e, lowest)
        return (e > s) & (s < np.concatenate([[lowest], np.maximum.accumulate(end)[:-1]]))

    kind = np.concatenate([np.full(g.size, i, dtype=np.int8) for i, g in enumerate(groups)])[order]
    bad = reach(kind == 0) | ((kind == 0) & reach(True))
    bad |= ((kind == 2) & reach(kind == 1)) | ((kind == 1) & reach(kind == 2))
    if first_written:
        bad |= (kind == 1) & reach(kind == 1)
    if bad.any():
        x = int(order[np.nonzero(bad)[0][0]])
        for i, g in enumerate(groups):
            if x < g.size:
                b, r = divmod(x, g.shape[1])
                raise ValueError(f"{_KINDS[i]} row {r} of stripe {b} overlaps another row in memory: the parity "
                                 "update works in place and needs disjoint rows")
            x -= g.size


class BatchUpdatePlan(_Update):
    """A reusable device parity update of B stripes of one shape, one launch per pass (grid.y =
    stripe), each stripe changing d natives of its own. As :class:`UpdatePlan` it keeps raw row
    pointers only, so a cache may hand it out only for the caller's live tensors.

    Args:
        parity: ``[B, p, C]``: the parity rows, updated in place.
        old_or_delta: ``[B, d, C]``: the natives' old contents (with ``new``) or the deltas.
        new: ``[B, d, C]`` new contents, or None for the delta form.
            Each of the three is a tensor (any batch and row strides, last stride 1) or a sequence of B
            stripes, each a ``[rows, C]`` tensor or a list of rows; all rows on one GPU, of one length.
        changed: d ids shared by every stripe, or ``[B, d]`` ids (:func:`batch_ids`).
        coeff: the p x k encoding matrix of the WHOLE code over GF(2^8); or
        maps: (p, k, 256) GF(2)-linear byte maps (the GF(16) nibble maps).
        store_new: also overwrite ``old_or_delta`` with ``new`` in the same pass. Needs ``new``.
        check: run the aliasing check (:func:`check_overlap_batch`); False when the caller has.
    """

    def __init__(self, parity, old_or_delta, new=None, *, changed, coeff=None, maps=None, store_new: bool = False,
                 check: bool = True):
        par, first = batch_part(parity, "parity"), batch_part(old_or_delta, "old" if new is not None else "delta")
        second = None if new is None else batch_part(new, "new")
        if store_new and second is None:
            raise ValueError("store_new needs the new rows (the pair form)")
        if coeff is not None:
            tables = perm_tables_from_coeff(np.asarray(coeff, dtype=np.uint8))
        elif maps is not None:
            tables = perm_tables_from_maps(maps)
        else:
            raise ValueError("need coeff or maps")
        self.p, self.k = (int(v) for v in tables.shape[:2])
        self.batch = par.nstripes
        if self.batch < 1 or not 1 <= self.p <= 255:
            raise ValueError("BatchUpdatePlan needs at least one stripe and 1..255 parity rows")
        ids = batch_ids(changed, self.batch, self.k)
        self.d = ids.shape[1]
        check_parts(par, first, second, self.p, self.d)
        self.device = par.device
        if self.device.type != "cuda":
            raise ValueError("BatchUpdatePlan runs on a GPU")
        self.pairs, self.store_new = second is not None, bool(store_new)
        self.m_pad, self.ncols = pad_m(self.p), par.ncols
        pp, fp = par.ptrs(), first.ptrs()
        sp = None if second is None else second.ptrs()
        if check:
            check_overlap_batch(pp, fp, sp, self.ncols, self.store_new)
        # one unaligned row: the whole batch bytewise
        self.bytewise = any(bool((a % np.uint64(16)).any()) for a in (pp, fp, sp) if a is not None)
        # one descriptor per pass of at most MAX_D changed rows of every stripe (ids[:, t0:t1])
        self.passes = []
        for t0 in range(0, self.d, MAX_D):
            t1 = min(self.d, t0 + MAX_D)
            host = build_update_batch_desc(ids[:, t0:t1], fp[:, t0:t1], None if sp is None else sp[:, t0:t1], pp,
                                           tables)
            self.passes.append((t1 - t0, torch.from_numpy(host).to(self.device)))
        self._ready = ready_event(self.device)

    def _launch(self, desc: int, d: int, col0: int, ncols: int, bytewise: bool, stream: int) -> None:
        hip().update_batched(desc, self.k, d, self.m_pad, self.batch, col0, ncols, self.pairs, self.store_new,
                             bytewise, stream)
