"""Shared pieces of tests/test_engine_cases.py and tests/test_gpu_engines.py: inputs for the GEMM
engines that a random draw never produces.

Three families, for GF(2^8) (w = 8) and GF(2^16) (w = 16):

* the count ladder (:func:`ladder_coeff`, :func:`ladder_data`). The matrix-core engines compute an
  integer count per output bit and keep its parity. With random operands a product bit is 1 with
  probability 1/4, so the counts stay in the lower third of their range. The ladder uses the one
  coefficient per output bit whose bit-matrix row is all ones (:func:`saturating`) and columns whose
  first t input rows are all-ones symbols: the count of the saturated bit is exactly w * t, and one
  launch walks 0, w, 2w, ... w * k, every second lap one less;
* structured matrices (:data:`STRUCTURED`, :func:`structured`): zero, null rows and columns between
  random ones, selections, all ones, and a third zeros / a third ones;
* every coefficient on one input row at a time (:func:`every_coeff`): impulse columns that spell
  out the whole product table of the field (w = 8) or every coefficient's 16 x 16 bit map (w = 16).

:func:`counts` is an integer bit-matrix product that uses neither the kernels nor the oracle's gemm;
:func:`oracle_gemm` is the oracle's gemm with its per-coefficient tables computed once per distinct
coefficient (the CPU module pins the two equal). Only numpy and ``gpu_rscode_amd.gf`` are used here.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from gpu_rscode_amd import gf

LADDER_EXTRA = 77  # ragged symbols after the 16 laps


def field(w: int) -> gf.GF:
    return gf.field(w)


def sym_dtype(w: int):
    return np.uint8 if w == 8 else np.dtype("<u2")


# ---- bit matrices -----------------------------------------------------------------------------------
def bit_images(F: gf.GF, coeff) -> np.ndarray:
    """(..., w, w) 0/1 array of the GF(2) matrices of ``coeff``: entry [..., b, a] is bit b of
    coeff * 2^a (the oracle's multiply on the basis symbols)."""
    c = np.asarray(coeff, dtype=np.int64)
    img = F.mul(c[..., None], (1 << np.arange(F.w)).reshape((1,) * c.ndim + (-1,)))  # (..., a)
    return ((img[..., None, :] >> np.arange(F.w).reshape((1,) * c.ndim + (-1, 1))) & 1).astype(np.uint8)


def _solve_gf2(a: np.ndarray, rhs: np.ndarray) -> np.ndarray:
    """The unique x with a . x = rhs over GF(2) (a square and nonsingular)."""
    n = a.shape[0]
    aug = np.concatenate([a.astype(np.uint8) & 1, rhs.reshape(n, 1).astype(np.uint8) & 1], axis=1)
    for c in range(n):
        p = c + int(np.nonzero(aug[c:, c])[0][0])
        if p != c:
            aug[[c, p]] = aug[[p, c]]
        for r in range(n):
            if r != c and aug[r, c]:
                aug[r] ^= aug[c]
    return aug[:, n]


@lru_cache(maxsize=None)
def saturating(w: int) -> tuple:
    """(c_0, ..., c_{w-1}): c_b is the one field element for which bit b of c_b * x is the XOR of all
    bits of x (row b of its bit matrix is all ones). GF(2^8): found by searching the 256 values.
    GF(2^16): c -> (bit b of c * 2^a, a < 16) is GF(2)-linear in the bits of c, so c_b solves the
    16 x 16 system T_b . bits(c) = (1, ..., 1) with T_b[a, i] = bit b of 2^i * 2^a."""
    F = field(w)
    if w == 8:
        rows = bit_images(F, np.arange(256)).all(axis=2)  # [c, b]: row b of c's matrix is all ones
        out = []
        for b in range(w):
            hit = np.nonzero(rows[:, b])[0]
            assert hit.size == 1
            out.append(int(hit[0]))
        return tuple(out)
    basis = bit_images(F, 1 << np.arange(w))  # [i, b, a]
    out = []
    for b in range(w):
        x = _solve_gf2(basis[:, b, :].T, np.ones(w, np.uint8))
        out.append(int((x.astype(np.int64) << np.arange(w)).sum()))
    return tuple(out)


def bit_matrix(F: gf.GF, coeff) -> np.ndarray:
    """The (w m x w k) 0/1 matrix of an m x k coefficient matrix: row w i + b, column w j + a."""
    c = np.asarray(coeff, dtype=np.int64)
    m, k = c.shape
    return bit_images(F, c).transpose(0, 2, 1, 3).reshape(m * F.w, k * F.w)


def bits_of(F: gf.GF, data) -> np.ndarray:
    """(w k x C) 0/1 matrix of k symbol rows: row w j + a is bit a of row j."""
    d = np.asarray(data, dtype=np.int64)
    return ((d[:, None, :] >> np.arange(F.w).reshape(1, -1, 1)) & 1).reshape(d.shape[0] * F.w, d.shape[1]) \
        .astype(np.uint8)


def counts(F: gf.GF, coeff, data) -> np.ndarray:
    """(m, w, C) integer counts behind every output bit: the bit-matrix product over the integers,
    in float32 (exact: a count is at most w * k < 2^24)."""
    m, k = np.asarray(coeff).shape
    assert F.w * k < 1 << 24
    c = bit_matrix(F, coeff).astype(np.float32) @ bits_of(F, data).astype(np.float32)
    return np.rint(c).astype(np.int64).reshape(m, F.w, -1)


def from_counts(F: gf.GF, cnt: np.ndarray) -> np.ndarray:
    """Output symbols whose bit b is the parity of count [i, b, c]."""
    return ((cnt & 1) << np.arange(F.w).reshape(1, -1, 1)).sum(axis=1).astype(sym_dtype(F.w))


def oracle_gemm(F: gf.GF, coeff, data) -> np.ndarray:
    """``F.gemm(coeff, data)`` with ``F.mul_table`` computed once per distinct coefficient (a ladder
    matrix holds w distinct values in up to 12,000 entries)."""
    coeff = np.asarray(coeff, dtype=np.int64)
    data = np.asarray(data)
    out = np.zeros((coeff.shape[0], data.shape[1]), dtype=F.dtype)
    tables: dict[int, np.ndarray] = {}
    for i in range(coeff.shape[0]):
        for j in range(coeff.shape[1]):
            c = int(coeff[i, j])
            if c == 0:
                continue
            if c == 1:
                out[i] ^= data[j]
                continue
            if c not in tables:
                tables[c] = F.mul_table(c)
            out[i] ^= tables[c][data[j]]
    return out


# ---- A. count ladder --------------------------------------------------------------------------------
def ladder_ncols(k: int) -> int:
    """Symbols per row: 16 laps of k + 1 heights plus a ragged rest."""
    return 16 * (k + 1) + LADDER_EXTRA


def ladder_coeff(w: int, m: int, k: int, first: int = 0) -> np.ndarray:
    """Row i is c_{(first + i) mod w} in every column: output row i saturates bit (first + i) mod w.
    With m >= w every output bit has a saturating row; a one-row engine shape takes ``first`` =
    0 .. w - 1 in turn."""
    sat = np.array(saturating(w), dtype=np.int64)
    return np.repeat(sat[(first + np.arange(m)) % w].reshape(m, 1), k, axis=1)


def ladder_heights(k: int, ncols: int | None = None):
    """(t, odd lap) per column: t = c mod (k + 1) all-ones rows, on every second lap one bit less."""
    c = np.arange(ladder_ncols(k) if ncols is None else ncols)
    return c % (k + 1), (c // (k + 1)) % 2 == 1


def ladder_data(w: int, k: int, ncols: int | None = None) -> np.ndarray:
    """(k, ncols) symbols: column c has its first t = c mod (k + 1) rows set to the all-ones symbol
    and the rest zero; on odd laps bit 0 of row 0 is cleared where t >= 1."""
    t, odd = ladder_heights(k, ncols)
    ones = (1 << w) - 1
    d = np.where(np.arange(k).reshape(-1, 1) < t.reshape(1, -1), ones, 0).astype(np.int64)
    d[0, odd & (t >= 1)] &= ~1
    return d.astype(sym_dtype(w))


def ladder_count_set(w: int, k: int) -> set:
    return {w * t for t in range(k + 1)} | {w * t - 1 for t in range(1, k + 1)}


# ---- B. structured matrices -------------------------------------------------------------------------
STRUCTURED = ("zero", "null_rows_cols", "selection", "all_ones", "thirds")


# engine -> (k, m, symbols per row, rows per output tile): the shapes the GPU module runs the
# structured cases on and the CPU module holds to their conditions. ``tile`` is the engine's own
# output tile at that shape: tile_for(m_pad) on the v_perm, byte and LDS-table kernels (8 on the
# k-split kernel that a wide short-row launch takes), 4 output rows per M-tile on every matrix-core
# engine (32 MFMA rows: 4 x 8 bits, or 2 x 16 bits in two byte planes of 4 symbols), and 1 on the
# GF(2^16) v_perm kernels at short rows (one output per tile). Row lengths: at least one whole vector
# block of the engine plus a ragged tail. m >= 2 tile + 2 wherever the engine allows it, so that a
# whole tile's worth of null rows sits at the end beside live ones; NULL_TAIL_ONE_ROW lists the
# engines that cannot (their kernels exist for one tile of at most 4 rows only).
ENGINES8 = {
    "vec": (12, 40, 32 * 256 * 2 + 32 + 11, 16),         # 16-row tiles, two 16-byte groups per lane
    "valu_wide": (40, 20, 16 * 64 * 3 + 16 * 5 + 7, 8),  # the default launch of a wide short-row code
    "byte": (5, 40, 4099, 16),
    "lut": (16, 40, 65536 + 5, 16),
    "mfma_i8": (32, 20, 512 * 5 + 123, 4),
    "mfma_v1": (128, 12, 256 * 9 + 77, 4),
    "mfma_ar": (128, 16, 256 * 9 + 77, 4),
    "mfma_tm": (128, 20, 256 * 9 + 77, 4),
    "batched_valu": (10, 40, 4099, 16),
    "batched_fp4": (128, 32, 256 * 3 + 50, 4),
}
for _k in (4, 8, 10, 16):  # rows-in-flight: its own tile (pf = 0: m <= 4) or 1- / 2-row tiles
    for _pf, _m in ((0, 4), (-1, 4), (-2, 8)):
        ENGINES8[f"rows_k{_k}_pf{_pf}"] = (_k, _m, 16 * (256 * 3 + 5) + 11, {0: 4, -1: 1, -2: 2}[_pf])

ENGINES16 = {
    "valu16_g1": (20, 12, 8 * (256 * 2 + 9) + 5, 1),   # short rows: one output per tile, one group per lane
    "valu16_g2": (6, 4, 8 * (512 * 70 + 100) + 5, 4),  # long rows, two groups per lane: tiles of <= 4 only
    "sym": (6, 5, 3001, 1),
    "mfma": (20, 12, 512 * 3 + 77, 4),
    "batched_valu16": (6, 4, 1003, 1),
    "batched_mfma": (20, 12, 512 * 2 + 45, 4),
}
NULL_TAIL_ONE_ROW = {(8, f"rows_k{_k}_pf0") for _k in (4, 8, 10, 16)} | {(16, "valu16_g2")}
BATCH = 3  # stripes of the batched engines


def engines(w: int) -> dict:
    return ENGINES8 if w == 8 else ENGINES16


def engine_seed(w: int, engine: str) -> int:
    return 100 + sorted(engines(w)).index(engine)


def null_layout(m: int, k: int, tile: int):
    """(zero rows, zero columns) of the ``null_rows_cols`` case for an engine whose output tile
    holds ``tile`` rows: the first and the last row of the first tile, and, where the matrix is tall
    enough to keep random rows in between (m >= 2 tile + 2), a whole tile's worth at the end, as if
    the last tile were padding; otherwise (only the one-tile kernels of NULL_TAIL_ONE_ROW, m = tile)
    the last row alone. Columns 0, k - 1 and k // 2 are zero where k >= 4."""
    t = min(tile, m)
    rows = {0, t - 1}
    rows |= set(range(m - tile, m)) if m >= 2 * tile + 2 else {m - 1}
    if len(rows) >= m:  # (m <= 2: keep row m - 1 random)
        rows = {0} if m > 1 else set()
    cols = {0, k - 1, k // 2} if k >= 4 else set()
    return sorted(rows), sorted(cols)


def selection_map(m: int, k: int, seed: int) -> np.ndarray:
    """pi(i) for output row i: a seeded permutation of the inputs, wrapping for m > k."""
    perm = np.random.default_rng(seed).permutation(k)
    return perm[np.arange(m) % k]


def structured(name: str, w: int, m: int, k: int, tile: int, seed: int) -> np.ndarray:
    """The m x k coefficient matrix of one structured case (int64)."""
    F = field(w)
    rng = np.random.default_rng([seed, w, m, k, STRUCTURED.index(name)])
    if name == "zero":
        return np.zeros((m, k), dtype=np.int64)
    if name == "all_ones":
        return np.ones((m, k), dtype=np.int64)
    if name == "selection":
        c = np.zeros((m, k), dtype=np.int64)
        c[np.arange(m), selection_map(m, k, seed)] = 1
        return c
    if name == "null_rows_cols":
        c = rng.integers(1, F.order, size=(m, k)).astype(np.int64)
        rows, cols = null_layout(m, k, tile)
        c[rows, :] = 0
        c[:, cols] = 0
        return c
    if name == "thirds":
        kind = rng.integers(0, 3, size=(m, k))
        c = rng.integers(2, F.order, size=(m, k)).astype(np.int64)
        c[kind == 0] = 0
        c[kind == 1] = 1
        return c
    raise ValueError(name)


def structured_expect(name: str, w: int, m: int, k: int, seed: int, data: np.ndarray):
    """What the case's output must be, straight from the input rows (no field arithmetic), or None
    where only the oracle says."""
    data = np.asarray(data)
    if name == "zero":
        return np.zeros((m, data.shape[1]), dtype=data.dtype)
    if name == "selection":
        return data[selection_map(m, k, seed)]
    if name == "all_ones":
        return np.repeat(np.bitwise_xor.reduce(data, axis=0).reshape(1, -1), m, axis=0)
    return None


def random_symbols(w: int, rows: int, ncols: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 1 << w, size=(rows, ncols)).astype(sym_dtype(w))


# ---- C. every coefficient, one input row at a time --------------------------------------------------
EVERY_RANDOM = {8: 1000, 16: 256}  # random symbols after the impulses


def every_dims(w: int):
    """(n, impulses per input row): coeff is n x n; w = 8 sends every value v through every
    coefficient, w = 16 every basis symbol 2^e."""
    return (16, 256) if w == 8 else (256, 16)


@lru_cache(maxsize=None)
def every_coeff(w: int):
    """``(coeff, data, table)``: coeff = arange(order) as an n x n matrix; data holds, for each input
    row j, ``per`` impulse columns (column per * j + v holds v (w = 8) or 2^v (w = 16) in row j and
    zero elsewhere), then random symbols; ``table[i, per * j + v]`` is the oracle's product
    coeff[i, j] * impulse, which the output's impulse columns must equal."""
    F = field(w)
    n, per = every_dims(w)
    coeff = np.arange(F.order, dtype=np.int64).reshape(n, n)
    imp = np.arange(per, dtype=np.int64) if w == 8 else (1 << np.arange(per, dtype=np.int64))
    data = np.zeros((n, n * per + EVERY_RANDOM[w]), dtype=np.int64)
    for j in range(n):
        data[j, per * j: per * (j + 1)] = imp
    data[:, n * per:] = random_symbols(w, n, EVERY_RANDOM[w], 1234 + w)
    table = F.mul(coeff[:, :, None], imp.reshape(1, 1, -1)).reshape(n, n * per)
    data = data.astype(sym_dtype(w))
    table = table.astype(sym_dtype(w))
    for a in (coeff, data, table):
        a.setflags(write=False)
    return coeff, data, table


@lru_cache(maxsize=None)
def every_expect(w: int) -> np.ndarray:
    """Whole expected output of :func:`every_coeff`: the product table, then the oracle's matrix
    product on the random symbols."""
    F = field(w)
    coeff, data, table = every_coeff(w)
    n, per = every_dims(w)
    out = np.concatenate([table, F.matmul(coeff, data[:, n * per:]).astype(sym_dtype(w))], axis=1)
    out.setflags(write=False)
    return out
