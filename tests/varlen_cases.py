"""Shared cases of tests/test_varlen.py (CPU) and tests/test_gpu_varlen.py (GPU): batches of stripes
of differing lengths, their rows as views of one guard-filled arena, and numpy oracles of every byte.

The length sets come from the kernel's units (``ops.varlen.GROUP``: the 16 bytes a lane of the vector
form owns; ``ops.varlen.BLOCK``: the 256 lanes of a workgroup): a full workgroup of groups is
``BLOCK * GROUP`` = 4096 bytes, and the ragged tail of a row takes one more lane per byte, so 4095 bytes
are 255 groups and 15 tail lanes, 270 lanes, and the tail opens a second workgroup.

The oracle of a batch is computed once per (code, lengths, seed) and shared read-only. Nothing here
touches a GPU unless a test passes ``device="cuda"``.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd.ops.varlen import BLOCK, GROUP

F8 = gf.GF256
FULL = BLOCK * GROUP  # bytes of one workgroup of whole groups
GUARD, FRESH = 0xA5, 0x5A  # the arena's filling; what an output row holds before the call

# every size at which the lane rule takes another turn
LENGTHS = (0, 1, GROUP - 1, GROUP, GROUP + 1,
           FULL - 1,                   # 255 groups + 15 tail lanes: the tail opens a second block
           FULL, FULL + 1, FULL + GROUP - 1, FULL + GROUP,
           2 * FULL - 1,
           16 * FULL + 3)              # 4096 groups + 3 tail lanes: 17 blocks
assert LENGTHS == (0, 1, 15, 16, 17, 4095, 4096, 4097, 4111, 4112, 8191, 65539)


def _short(count: int, seed: int, top: int = 3 * GROUP) -> tuple:
    return tuple(int(v) for v in np.random.default_rng(seed).integers(1, top + 1, size=count))


BATCHES = {
    "b1": (FULL - 1,),
    "b2": (1, FULL + GROUP),
    "b3": (FULL + 1, GROUP, 2 * FULL - 1),
    "b257": tuple(int(v) for v in np.random.default_rng(257).integers(0, 2 * BLOCK + 1, size=257)),
    "zero-first": (0, GROUP + 1, FULL),
    "zero-middle": (GROUP - 1, 0, FULL + GROUP - 1),
    "zero-last": (FULL + 1, 1, 0),
    "zeros-only": (0, 0, 0),
    "ladder": LENGTHS,
    "one-long-among-256": _short(128, 1) + (16 * FULL + 3,) + _short(128, 2),
    "equal": (FULL + 5,) * 5,
}
WIDE_BATCH = (1, FULL + 1, 2 * GROUP + 1)  # the (128, 160) code runs these only

CODES = {
    "c10_14": (10, 14, "cauchy", "gf256"),
    "c4_6": (4, 6, "cauchy", "gf256"),        # m_pad 2
    "c3_4": (3, 4, "cauchy", "gf256"),        # m_pad 1
    "c9_14": (9, 14, "cauchy", "gf256"),      # p = 5: two tiles
    "c3_19": (3, 19, "cauchy", "gf256"),      # p = 16
    "v10_14": (10, 14, "vandermonde", "gf256"),
    "g16_4_6": (4, 6, "cauchy", "gf16"),
    "c128_160": (128, 160, "cauchy", "gf256"),
}

# (code, batch): every batch on the flagship code; the ladder (every length) and a zero-length stripe
# in the middle on every other code; the wide code at its three lengths
CASES = ([("c10_14", b) for b in BATCHES]
         + [(c, b) for c in CODES if c not in ("c10_14", "c128_160") for b in ("ladder", "zero-middle")]
         + [("c128_160", "wide")])


def lengths_of(batch: str) -> tuple:
    return WIDE_BATCH if batch == "wide" else BATCHES[batch]


@functools.lru_cache(maxsize=None)
def codec(code: str) -> ReedSolomon:
    k, n, matrix, field = CODES[code]
    return ReedSolomon(k, n, matrix=matrix, field=field)


# ---- oracles -------------------------------------------------------------------------------------
def gemm(code: str, coeff: np.ndarray, data: np.ndarray) -> np.ndarray:
    """``coeff . data`` on byte rows from the numpy field: GF(2^8), or GF(16) on each nibble."""
    if CODES[code][3] == "gf16":
        f = gf.field(4)
        return (f.gemm(coeff, data & 15) | (f.gemm(coeff, data >> 4) << 4)).astype(np.uint8)
    return F8.gemm(np.asarray(coeff, dtype=np.uint8), data).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def consistent(code: str, lengths: tuple, seed: int = 0) -> tuple:
    """Consistent stripes ``[n, C_b]`` of the code, one per length (read-only): random natives and
    the oracle's ``E . natives``, computed in one GEMM over the concatenated columns."""
    rs = codec(code)
    rng = np.random.default_rng([seed, rs.k, rs.n, len(lengths)])
    data = rng.integers(0, 256, size=(rs.k, int(sum(lengths))), dtype=np.uint8)
    full = np.concatenate([data, gemm(code, rs.E, data)])
    ends = np.cumsum(lengths)
    out = tuple(np.ascontiguousarray(full[:, e - c: e]) for c, e in zip(lengths, ends))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def erasures(code: str, nstripes: int, seed: int = 0, kind: str = "mixed") -> tuple:
    """Erased ids per stripe, a pattern per stripe: the count cycles through 0..p, the ids are drawn
    from the natives, the parity rows or all rows (``kind``); unsorted. On the reference Vandermonde
    code (not MDS) a draw whose survivors are singular is drawn again."""
    rs = codec(code)
    rng = np.random.default_rng([seed, nstripes, rs.n])
    pool = {"natives": np.arange(rs.k), "parity": np.arange(rs.k, rs.n), "mixed": np.arange(rs.n)}[kind]
    out = []
    for b in range(nstripes):
        e = min((b + 1) % (rs.p + 1), pool.size)
        while True:
            ids = tuple(int(i) for i in rng.permutation(pool)[:e])
            sv = [i for i in range(rs.n) if i not in ids][: rs.k]
            if rs.field != "gf256" or CODES[code][2] == "cauchy" or F8.is_invertible(rs.G[sv]):
                break
        out.append(ids)
    return tuple(out)


def damaged(good, erased) -> list:
    """Copies of the stripes with the erased rows holding FRESH."""
    out = []
    for g, ids in zip(good, erased):
        a = np.array(g)
        a[list(ids)] = FRESH
        out.append(a)
    return out


def repaired(code: str, bad, erased) -> list:
    """The oracle of a repair, stripe by stripe: ``gf.reconstruct_oracle`` over GF(2^8); for the GF(16)
    code the same route on each nibble."""
    rs = codec(code)
    out = []
    for a, ids in zip(bad, erased):
        if rs.field == "gf256":
            out.append(gf.reconstruct_oracle(rs.G, a, ids))
            continue
        a = np.array(a)
        ids = sorted(set(ids))
        if ids:
            f = gf.field(4)
            sv = [i for i in range(rs.n) if i not in ids][: rs.k]
            coeff = f.matmul(rs.G[ids], f.invert(rs.G[sv]))
            a[ids] = gemm(code, coeff, a[sv])
        out.append(a)
    return out


# ---- the arena -----------------------------------------------------------------------------------
GAP = 48     # guard bytes after every row, at least
HEAD = 512   # guard bytes before the first row and after the last


class Batch:
    """B stripes of ``nrows`` rows, stripe b's of ``lengths[b]`` bytes, as views of one guard-filled
    arena on ``device``. List form: every row starts ``shift.get((b, j), 0)`` bytes past a 16-byte
    boundary, GAP guard bytes or more after it; ``arg`` is the list of stripes, each a list of rows
    (``as2d``: an ``[nrows, C_b]`` strided view per stripe instead). Packed form (``packed``): one
    ``[nrows, T]`` tensor ``arg`` with ``offsets`` (``lead`` bytes of guard before the first stripe and
    GAP after the last inside every row; stripes follow each other without a gap). ``image`` is the
    oracle of every byte of the arena: ``put`` writes it, ``upload`` copies it to the buffer."""

    def __init__(self, nrows: int, lengths, device: str = "cpu", packed: bool = False, shift=None, lead: int = 16,
                 as2d: bool = False):
        self.nrows, self.lengths, self.packed = nrows, [int(c) for c in lengths], packed
        nb = len(self.lengths)
        self.off = np.zeros((nb, nrows), dtype=np.int64)
        self.offsets = None
        if packed:
            self.offsets = np.concatenate([[lead], lead + np.cumsum(self.lengths)]).astype(np.int64)
            width = int(self.offsets[-1]) + GAP
            pitch = (width + 255) // 256 * 256
            self.off[:] = HEAD + np.arange(nrows)[None, :] * pitch + self.offsets[:-1, None]
            size = HEAD + nrows * pitch + HEAD
        else:
            shift = shift or {}
            cursor = HEAD
            if as2d:  # the rows of a stripe one pitch apart
                for b, c in enumerate(self.lengths):
                    pitch = (c + GAP + 15) // 16 * 16
                    self.off[b] = cursor + np.arange(nrows) * pitch
                    cursor += nrows * pitch
            else:
                for b, c in enumerate(self.lengths):
                    for j in range(nrows):
                        self.off[b, j] = (cursor + 15) // 16 * 16 + shift.get((b, j), 0)
                        cursor = int(self.off[b, j]) + c + GAP
            size = cursor + HEAD
        self.image = np.full(size, GUARD, dtype=np.uint8)
        raw = torch.full((size + 256,), GUARD, dtype=torch.uint8, device=device)
        self.buf = raw[(-raw.data_ptr()) % 256:][:size]
        base = self.buf.storage_offset()  # (as_strided counts from the storage, not from the view)
        if packed:
            self.arg = self.buf.as_strided((nrows, width), (pitch, 1), base + HEAD)
        elif as2d:
            self.arg = [self.buf.as_strided((nrows, c), ((c + GAP + 15) // 16 * 16, 1), base + int(self.off[b, 0]))
                        for b, c in enumerate(self.lengths)]
        else:
            self.arg = [[self.buf[int(o): int(o) + c] for o in self.off[b]] for b, c in enumerate(self.lengths)]
        # the rows in address order, to name a byte that differs
        flat = self.off.reshape(-1)
        self._order = np.argsort(flat, kind="stable")
        self._starts = flat[self._order]

    def put(self, stripes, rows=None) -> None:
        """Writes ``stripes[b]`` (``[len(rows), C_b]``) into rows ``rows`` (default: all) of the image."""
        rows = range(self.nrows) if rows is None else rows
        for b, s in enumerate(stripes):
            c = self.lengths[b]
            for x, j in zip(np.asarray(s, dtype=np.uint8).reshape(len(rows), c), rows):
                self.image[self.off[b, j]: self.off[b, j] + c] = x

    def put_packed(self, full, rows=None) -> None:
        """Packed form: ``full`` (``[len(rows), sum(lengths)]``, the stripes side by side) into the image."""
        rows = range(self.nrows) if rows is None else rows
        lo = self.off[0] if len(self.lengths) else None
        for x, j in zip(np.asarray(full, dtype=np.uint8), rows):
            self.image[lo[j]: lo[j] + x.size] = x

    def upload(self) -> None:
        self.buf.copy_(torch.from_numpy(self.image.copy()).to(self.buf.device))

    def kw(self) -> dict:
        return {"offsets": self.offsets} if self.packed else {}

    def check(self, what: str, got: np.ndarray | None = None) -> None:
        """The WHOLE arena against the image: a byte past a row's end, a byte of another stripe, a byte
        not stored. The message names the stripe, the row and the column of the first byte that differs."""
        if got is None:
            if self.buf.is_cuda:
                torch.cuda.synchronize()
            got = self.buf.cpu().numpy()
        if np.array_equal(got, self.image):
            return
        bad = np.flatnonzero(got != self.image)
        x = int(bad[0])
        i = int(np.searchsorted(self._starts, x, side="right")) - 1
        if i < 0:
            where = f"{int(self._starts[0]) - x} bytes before the first row"
        else:
            b, j = divmod(int(self._order[i]), self.nrows)
            col = x - int(self._starts[i])
            where = f"stripe {b}, row {j}, column {col} (the row has {self.lengths[b]} bytes)"
        raise AssertionError(f"{what}: {bad.size} bytes of the arena differ from the oracle and the guard; the first "
                             f"at arena offset {x}: {where}: got {got[x]:#04x}, want {self.image[x]:#04x}")


def encode_case(code: str, lengths, device: str, seed: int = 0, **kw):
    """(data batch, parity batch, the consistent stripes): natives in place, parity rows FRESH, uploaded;
    the parity image already holds the oracle."""
    rs = codec(code)
    good = consistent(code, tuple(lengths), seed)
    data, par = Batch(rs.k, lengths, device, **kw), Batch(rs.p, lengths, device, **kw)
    data.put([g[: rs.k] for g in good])
    par.put([np.full((rs.p, g.shape[1]), FRESH, dtype=np.uint8) for g in good])
    data.upload()
    par.upload()
    par.put([g[rs.k:] for g in good])
    return data, par, good


def repair_case(code: str, lengths, erased, device: str, seed: int = 0, **kw):
    """(the batch of n-row stripes, damaged and uploaded, its image already holding the oracle of
    the repair; the damaged stripes; the oracle's stripes)."""
    rs = codec(code)
    good = consistent(code, tuple(lengths), seed)
    bad = damaged(good, erased)
    want = repaired(code, bad, erased)
    batch = Batch(rs.n, lengths, device, **kw)
    batch.put(bad)
    batch.upload()
    batch.put(want)
    return batch, bad, want
