"""Row arguments: what the plans and the codec accept as "rows of stripes", in one place.

A row is a contiguous 1-D uint8 tensor. One stripe's rows come as a ``[rows, C]`` tensor or a list of
rows (:func:`as_rows`); the rows of B stripes as a *part*: :class:`TensorPart` (a ``[B, rows, C]``
tensor), :class:`ListPart` (a sequence of stripes) or :class:`PickPart` (rows picked by id from
another part). Every part has ``nstripes``, ``nrows``, ``ncols``, ``device``, ``key`` (names the
buffers, for a plan cache), ``ptrs()`` (the uint64 ``[B, rows]`` row addresses), ``rows(b)`` (stripe
b's row tensors) and ``lens`` (the rows' lengths). A single stripe is a part of one stripe
(:func:`stripe_part`) with one licence a batch does not have: its rows may differ in length, and the
shortest one counts (``ragged``).
"""
from __future__ import annotations

import numpy as np
import torch


class RowDtypeError(TypeError, ValueError):
    """Rows that are not uint8. The plans have raised ``TypeError`` for them and the codec's update
    and batched calls ``ValueError``: both still catch it."""


def as_rows(x) -> list[torch.Tensor]:
    if isinstance(x, torch.Tensor):
        if x.dim() == 1:
            return [x]
        if x.dim() != 2:
            raise ValueError("expected a 2-D [rows, bytes] tensor or a list of 1-D tensors")
        return [x[i] for i in range(x.shape[0])]
    return list(x)


def check_rows(rows: list[torch.Tensor], what: str, device: torch.device | None) -> torch.device:
    for r in rows:
        if r.dtype != torch.uint8:
            # a TypeError to the plans' callers, as since GemmPlan; a ValueError to the callers of the parts and
            # of the codec's batched calls, which raise nothing else for a bad row
            raise RowDtypeError(f"{what} rows must be uint8, got {r.dtype}")
        if r.dim() != 1 or (r.numel() > 1 and r.stride(0) != 1):
            raise ValueError(f"{what} rows must be contiguous 1-D byte rows")
        if device is None:
            device = r.device
        elif r.device != device:
            raise ValueError(f"all rows must live on one device ({device} vs {r.device})")
    return device


def stripe_rows(stripe, n: int) -> tuple[list[torch.Tensor], int, torch.device]:
    """One stripe as (its n rows, the shortest row's length, the device)."""
    rs = as_rows(stripe)
    if len(rs) != n:
        raise ValueError(f"stripe must have n={n} rows")
    dev = check_rows(rs, "stripe", None)
    return rs, min(r.numel() for r in rs), dev


def window(col0: int, ncols: int | None, limit: int) -> tuple[int, int]:
    col0 = int(col0)
    ncols = limit - col0 if ncols is None else int(ncols)
    if col0 < 0 or ncols < 0 or col0 + ncols > limit:
        raise ValueError(f"column range [{col0}, {col0 + ncols}) outside rows of {limit} bytes")
    return col0, ncols


class null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


class TensorPart:
    """Rows ``[:, j, :]`` of a ``[B, r, C]`` tensor (any batch and row strides, last stride 1)."""

    ragged = False

    def __init__(self, t: torch.Tensor, what: str):
        if t.dim() != 3:
            raise ValueError(f"{what}: expected a [B, rows, C] tensor or a sequence of stripes")
        if t.dtype != torch.uint8:
            raise ValueError(f"{what}: rows must be uint8, got {t.dtype}")
        if t.shape[2] > 1 and t.stride(2) != 1:
            raise ValueError(f"{what}: rows must be contiguous byte rows (last stride 1)")
        self.t = t
        self.nstripes, self.nrows, self.ncols = (int(v) for v in t.shape)
        self.lens, self.device = self.ncols, t.device
        self.key = ("t", int(t.data_ptr()), tuple(t.shape), tuple(t.stride()))

    def ptrs(self) -> np.ndarray:
        t = self.t
        b = np.arange(self.nstripes, dtype=np.int64)[:, None] * int(t.stride(0))
        return (int(t.data_ptr()) + b + np.arange(self.nrows, dtype=np.int64)[None, :] * int(t.stride(1))).astype(np.uint64)

    def rows(self, b: int) -> list[torch.Tensor]:
        return [self.t[b, j] for j in range(self.nrows)]


class ListPart:
    """A sequence of stripes, each an ``[r, C]`` tensor or a list of r rows. All rows have one length,
    unless ``ragged``: then ``ncols`` is the shortest row's, and ``lens`` the int64 ``[B, r]`` lengths where
    they differ."""

    def __init__(self, stripes, what: str, ragged: bool = False):
        try:
            self.stripes = [as_rows(s) for s in stripes]
        except TypeError:
            raise ValueError(f"{what}: expected a [B, rows, C] tensor or a sequence of stripes") from None
        self.ragged = ragged
        self.nstripes = len(self.stripes)
        self.nrows = len(self.stripes[0]) if self.stripes else 0
        first = self.stripes[0][0] if self.nrows else None
        self.device = first.device if isinstance(first, torch.Tensor) else torch.device("cpu")
        ptrs, lens = [], []
        for rs in self.stripes:
            if len(rs) != self.nrows:
                raise ValueError(f"{what}: every stripe must have {self.nrows} rows, got {len(rs)}")
            try:
                check_rows(rs, what, self.device)
            except AttributeError:  # (not tensors)
                raise ValueError(f"{what}: rows must be uint8 tensors") from None
            ptrs.append([r.data_ptr() for r in rs])
            lens += [r.numel() for r in rs]
        self.ncols = min(lens, default=0)
        one = not lens or max(lens) == self.ncols
        if not ragged and not one:
            raise ValueError(f"{what}: rows must have one length ({self.ncols} vs {max(lens)})")
        shape = (self.nstripes, self.nrows)
        self.lens = self.ncols if one else np.array(lens, dtype=np.int64).reshape(shape)
        self._ptrs = np.array(ptrs, dtype=np.uint64).reshape(shape)

    @property
    def key(self) -> tuple:
        # (the [B, r] shape too: two stripes of three rows and three of two have the same pointer bytes)
        return ("l", self._ptrs.shape, self.lens if isinstance(self.lens, int) else self.lens.tobytes(),
                self._ptrs.tobytes())

    def ptrs(self) -> np.ndarray:
        return self._ptrs

    def rows(self, b: int) -> list[torch.Tensor]:
        return self.stripes[b]


class PickPart:
    """Rows ``idx[b, t]`` of stripe b of another part of one row length (or of a ``StripeBatch``): the
    changed natives of a batched write, or its parity rows. ``key`` names the source, the ``[B, r]`` shape
    of the ids and their bytes; a ``tag`` stands in for the bytes, and is the caller's promise that
    within one plan cache the tag and the shape determine the ids (the parity rows ``k..n-1`` of a codec)."""

    ragged = False

    def __init__(self, src, idx: np.ndarray, tag=None):
        self.src, self.idx = src, np.ascontiguousarray(idx, dtype=np.int64)
        self.nstripes, self.nrows = (int(v) for v in self.idx.shape)
        self.ncols, self.lens, self.device = src.ncols, src.ncols, src.device
        self.key = ("p", src.key, self.idx.shape, tag if tag is not None else self.idx.tobytes())

    def ptrs(self) -> np.ndarray:
        return np.take_along_axis(self.src.ptrs(), self.idx, axis=1)

    def rows(self, b: int) -> list[torch.Tensor]:
        r = self.src.rows(b)
        return [r[int(j)] for j in self.idx[b]]


def batch_part(x, what: str):
    """A row argument of a batched call as a part: a ``[B, rows, C]`` tensor, a sequence of B stripes
    (each a ``[rows, C]`` tensor or a list of rows), or a part as it is."""
    if isinstance(x, (TensorPart, ListPart, PickPart)):
        return x
    return TensorPart(x, what) if isinstance(x, torch.Tensor) else ListPart(x, what)


def stripe_part(x, what: str):
    """A row argument of a single-stripe call (a ``[rows, C]`` tensor or a list of rows) as a part of
    one stripe, whose rows may differ in length; or a part as it is."""
    if isinstance(x, (TensorPart, ListPart, PickPart)):
        return x
    return ListPart([x], what, ragged=True)


def check_parts(par, first, second, p: int, d: int) -> None:
    """ValueError unless the parts hold one number of stripes, p / d / d rows per stripe, one device
    (a part without rows, the parity of a p = 0 code, has none) and, unless ragged, one row length."""
    for part, want, name in ((par, p, "parity"), (first, d, "old / delta"), (second, d, "new")):
        if part is None:
            continue
        if part.nstripes != first.nstripes:
            raise ValueError(f"{first.nstripes} stripes of changed rows but {part.nstripes} of {name} rows")
        if not part.nstripes:
            continue
        if part.nrows != want:
            raise ValueError(f"expected {want} {name} rows per stripe, got {part.nrows}")
        if part.nrows and not part.ragged and part.ncols != first.ncols:
            raise ValueError(f"rows must have one length ({first.ncols} vs {name} rows of {part.ncols})")
        if part.nrows and part.device != first.device:
            raise ValueError(f"all rows must live on one device ({first.device} vs {part.device})")


class StripeBatch:
    """B stripes of n byte rows of one length C on one device, in any of the forms the batched scrub
    calls take: a ``[B, n, C]`` tensor; a sequence of B stripes, each an ``[n, C]`` tensor or a list of
    n rows; or natives ``[B, k, C]`` with ``parity`` ``[B, p, C]`` in another allocation. ``key``
    names the buffers (for a plan cache), ``ptrs()`` is the uint64 ``[B, n]`` row addresses,
    ``rows(b)`` stripe b's row tensors. Anything else raises ``ValueError``."""

    def __init__(self, stripes, n: int, parity=None, k: int | None = None):
        self.parts = [batch_part(stripes, "stripes")] + ([] if parity is None else [batch_part(parity, "parity")])
        first = self.parts[0]
        self.nstripes, self.ncols, self.device, self.n = first.nstripes, first.ncols, first.device, n
        if parity is not None:
            last = self.parts[1]
            if last.nstripes != self.nstripes:
                raise ValueError(f"{self.nstripes} stripes of natives but {last.nstripes} of parity")
            if self.nstripes and (first.nrows, last.nrows) != (k, n - k):
                raise ValueError(f"expected {k} native and {n - k} parity rows per stripe, "
                                 f"got {first.nrows} and {last.nrows}")
            if self.nstripes and last.ncols != self.ncols:
                raise ValueError(f"native rows of {self.ncols} bytes but parity rows of {last.ncols}")
            if self.nstripes and last.device != self.device:
                raise ValueError(f"all rows must live on one device ({self.device} vs {last.device})")
        elif self.nstripes and first.nrows != n:
            raise ValueError(f"every stripe must have n={n} rows, got {first.nrows}")

    @property
    def key(self) -> tuple:
        return tuple(part.key for part in self.parts)

    def ptrs(self) -> np.ndarray:
        ptrs = [part.ptrs() for part in self.parts]
        return np.concatenate(ptrs, axis=1) if len(ptrs) > 1 else ptrs[0]

    def rows(self, b: int) -> list[torch.Tensor]:
        return [r for part in self.parts for r in part.rows(b)]
