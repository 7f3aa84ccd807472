"""Shared pieces of tests/test_solver_cases.py and tests/test_gpu_solvers.py: decode systems whose
Gauss-Jordan must pivot.

The device solvers (gf_invert.hip, gf_decode16.hip) take as column c's pivot the lowest row that is
not yet a pivot and has a nonzero in column c. On a Cauchy or systematic Vandermonde generator that
row is always row c: every square submatrix is nonsingular, so after c elimination steps each
Schur-complement entry of column c is a ratio of two nonzero minors. The systems here are planted
so that the rule picks a known, scattered order instead (:func:`planted`), fails at a known column
(``dep_col``), and sits inside a generator [I; E] exactly as the kernels read it (:func:`embed`).

The result X = M^-1 B' is unique whatever the pivot order, so every comparison made with these cases
is exact. Only numpy and ``gpu_rscode_amd.gf`` are used here.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from gpu_rscode_amd import gf

PANELS = (4, 8, 16, 32)  # the instantiations of the blocked solve (force_panel)


def field(w: int) -> gf.GF:
    return gf.field(w)


# ---- construction -----------------------------------------------------------------------------------
def planted(F: gf.GF, e: int, blocks, seed: int, dep_col: int | None = None):
    """``(M, sigma)``: an e x e matrix over ``F`` with a planted pivot order.

    D is block upper triangular with dense random nonzero blocks: the b rows of each block of
    ``blocks`` (which sums to e) are nonzero from the block's first column to column e - 1 and zero
    to the left. M is D with row i moved to row ``sigma[i]``, a seeded random permutation. Rows of a
    later block are zero in an earlier block's columns, so elimination never touches them, and the
    rule "lowest row not yet a pivot with a nonzero in column c" takes each block's scattered rows
    in ascending order (:func:`predicted_sequence`). Blocks of size 1 are pure back-substitution;
    large blocks are dense forward elimination under a non-identity pivot order.

    ``dep_col = c`` replaces column c by a random nonzero combination of the columns before it
    (``dep_col = 0``: a zero column): the solve then finds no pivot exactly in column c.
    """
    blocks = [int(b) for b in blocks]
    assert sum(blocks) == e and min(blocks) >= 1
    rng = np.random.default_rng(seed)
    sigma = rng.permutation(e)  # (drawn first: planted_sigma() repeats it without the rest)
    d = np.zeros((e, e), dtype=np.int64)
    r0 = 0
    for b in blocks:
        d[r0 : r0 + b, r0:] = rng.integers(1, F.order, size=(b, e - r0))
        r0 += b
    if dep_col is not None:
        assert 0 <= dep_col < e
        if dep_col == 0:
            d[:, 0] = 0
        else:
            coef = rng.integers(1, F.order, size=(dep_col, 1))
            d[:, dep_col] = F.matmul(d[:, :dep_col], coef)[:, 0]
    m = np.zeros_like(d)
    m[sigma] = d
    return m.astype(F.dtype), sigma


def predicted_sequence(blocks, sigma) -> list[int]:
    """The pivot rows the kernels' rule takes on a :func:`planted` matrix whose blocks stay
    nonsingular under elimination: per block, the rows it was scattered to, ascending."""
    seq, r0 = [], 0
    for b in blocks:
        seq += sorted(int(s) for s in sigma[r0 : r0 + b])
        r0 += b
    return seq


def pivot_sequence(F: gf.GF, m: np.ndarray):
    """The kernels' pivot rule in numpy: ``(sequence, failed_column)``. Column c's pivot is the lowest
    row that is not yet a pivot and has a nonzero in column c; every other such row is cleared in
    column c. ``failed_column`` is the first column with no pivot (the sequence stops there), or
    ``None``."""
    a = np.array(m, dtype=np.int64)
    e = a.shape[0]
    free = np.ones(e, dtype=bool)
    seq: list[int] = []
    for c in range(e):
        cand = np.nonzero(free & (a[:, c] != 0))[0]
        if cand.size == 0:
            return seq, c
        p = int(cand[0])
        seq.append(p)
        free[p] = False
        rest = cand[1:]
        if rest.size:
            f = F.mul(a[rest, c], int(F.inv(int(a[p, c]))))
            a[rest] ^= F.mul(f.reshape(-1, 1), a[p].reshape(1, -1))
    return seq, None


def embed(F: gf.GF, k: int, n: int, e: int, m: np.ndarray, seed: int):
    """``(G, rows, erased)``: a generator G = [I; E] (n x k, dense random E), a seeded choice of e
    erased natives (ascending, as the kernels derive them) and of e parity survivors, and the
    shuffled survivor list ``rows``, with ``E[parity survivors in survivor order][:, erased] = m``:
    the matrix M of the kernels' system (gf_decode16.hip's header comment) is then exactly ``m``."""
    assert 1 <= e <= k and k + e <= n <= F.order and m.shape == (e, e)
    rng = np.random.default_rng(seed)
    E = rng.integers(1, F.order, size=(n - k, k)).astype(np.int64)
    erased = sorted(int(i) for i in rng.choice(k, size=e, replace=False))
    par = [k + int(i) for i in rng.choice(n - k, size=e, replace=False)]
    rows = [i for i in range(k) if i not in set(erased)] + par
    rows = [int(rows[i]) for i in rng.permutation(k)]
    order = [r - k for r in rows if r >= k]  # parity survivors in survivor order
    E[np.ix_(order, erased)] = np.asarray(m, dtype=np.int64)
    G = np.vstack([np.eye(k, dtype=np.int64), E]).astype(F.dtype)
    return G, rows, erased


def system_matrix(G: np.ndarray, k: int, rows, erased) -> np.ndarray:
    """M = G[P, erased] as the kernels gather it: P the parity survivors in survivor order."""
    return np.asarray(G)[np.ix_([r for r in rows if r >= k], list(erased))]


def split(e: int, bmax: int, seed: int) -> tuple[int, ...]:
    """A seeded composition of e into blocks of 1..bmax rows, at least two of them (one dense block
    has a nonzero in every place, and any pivot order solves it)."""
    rng = np.random.default_rng(seed)
    bmax = max(1, min(bmax, e - 1))
    out, left = [], e
    while left:
        b = int(rng.integers(1, min(bmax, left) + 1))
        out.append(b)
        left -= b
    return tuple(out)


# ---- what a case must satisfy -----------------------------------------------------------------------
def panel_gaps(seq, e: int, P: int) -> list[str]:
    """Why the pivot sequence ``seq`` of an e x e system does not exercise the blocked solve's row
    routing at panel width P (empty: it does). Every panel [c0, c0 + P) after the first must take a
    pivot row from above the panel's own rows (index < c0: a row an earlier panel left unused) and
    one from below them (index >= c0 + P). The last panel has no rows below it when c0 + P >= e, and
    is then held to the first half only. A system of one panel (e <= P) needs a non-identity order."""
    if e <= P:
        return [] if list(seq) != list(range(e)) or e == 1 else [f"P={P}: identity order"]
    why = []
    for c0 in range(P, e, P):
        piv = seq[c0 : c0 + P]
        if not any(p < c0 for p in piv):
            why.append(f"P={P} panel at {c0}: no pivot row above the panel")
        if c0 + P < e and not any(p >= c0 + P for p in piv):
            why.append(f"P={P} panel at {c0}: no pivot row below the panel")
    return why


def sequence_gaps(seq, e: int, panels=()) -> list[str]:
    """Every reason the good case's sequence is too tame: more than 10 % of the columns pick row c
    (a 1 x 1 system has no other order), or a panel width of ``panels`` is not exercised."""
    why = []
    fixed = sum(1 for c, p in enumerate(seq) if p == c)
    if e > 1 and fixed * 10 > e:
        why.append(f"{fixed} of {e} columns pick row c")
    for P in panels:
        why += panel_gaps(seq, e, P)
    return why


class ZeroPivot(Exception):
    pass


def solve_without_search(F: gf.GF, m: np.ndarray, b: np.ndarray) -> np.ndarray:
    """A deliberately wrong Gauss-Jordan solve of m X = b: row c is column c's pivot, no search.
    Right on a matrix whose leading minors are all nonzero (Cauchy), :class:`ZeroPivot` otherwise."""
    a = np.hstack([np.asarray(m, dtype=np.int64), np.asarray(b, dtype=np.int64)])
    e = a.shape[0]
    for c in range(e):
        if a[c, c] == 0:
            raise ZeroPivot(f"row {c} has a zero in column {c}")
        a[c] = F.mul(a[c], int(F.inv(int(a[c, c]))))
        rest = np.nonzero(a[:, c])[0]
        rest = rest[rest != c]
        if rest.size:
            a[rest] ^= F.mul(a[rest, c].reshape(-1, 1), a[c].reshape(1, -1))
    return a[:, e:].astype(F.dtype)


# ---- the cases --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One planted system. ``k = 0``: a bare e x e matrix (gf_invert); otherwise it is embedded in an
    (n, k) generator. ``panels``: the panel widths of the blocked solve it is run with."""
    id: str
    w: int
    e: int
    blocks: tuple
    seed: int
    k: int = 0
    n: int = 0
    panels: tuple = ()
    dep_col: int | None = None

    @property
    def F(self) -> gf.GF:
        return field(self.w)

    @property
    def good(self) -> bool:
        return self.dep_col is None

    def __str__(self) -> str:
        return self.id


@lru_cache(maxsize=None)
def matrix(case: Case):
    """``(M, sigma)`` of the case (computed once; do not modify)."""
    m, sigma = planted(case.F, case.e, case.blocks, case.seed, case.dep_col)
    m.setflags(write=False)
    return m, sigma


@lru_cache(maxsize=None)
def system(case: Case):
    """``(G, rows, erased)`` of an embedded case (computed once; do not modify)."""
    G, rows, erased = embed(case.F, case.k, case.n, case.e, matrix(case)[0], case.seed + 1)
    G.setflags(write=False)
    return G, tuple(rows), tuple(erased)


@lru_cache(maxsize=None)
def sequence(case: Case):
    return pivot_sequence(case.F, matrix(case)[0])


@lru_cache(maxsize=None)
def oracle_inverse(case: Case) -> np.ndarray:
    """numpy inverse of the good case's bare matrix (computed once; do not modify)."""
    inv = case.F.invert(matrix(case)[0])
    inv.setflags(write=False)
    return inv


@lru_cache(maxsize=None)
def oracle_rows(case: Case) -> np.ndarray:
    """Rows ``erased`` of the numpy inverse of G[rows]: the decode rows X (computed once; do not
    modify)."""
    G, rows, erased = system(case)
    x = case.F.invert(G[list(rows)])[list(erased)]
    x.setflags(write=False)
    return x


def singular_of(case: Case, dep_col: int) -> Case:
    """The same planted system with column ``dep_col`` made dependent on the columns before it."""
    return Case(f"{case.id}-dep{dep_col}", case.w, case.e, case.blocks, case.seed, case.k, case.n, (), dep_col)


# The block sizes the construction was first tried with (pivot rows from below / above the panel's
# own rows at panel width 32: 4 / 4, 17 / 19, 29 / 29).
B40 = (7, 1, 1, 13, 18)
B70 = (5, 1, 27, 1, 33, 3)
B97 = (31, 2, 33, 30, 1)

# Seeds (default 0) for which sequence_gaps() is empty and solve_without_search() fails
# (tests/test_solver_cases.py holds every case to both): the first such seed counting up from 0.
# A narrow panel through a large block sees that block's rows in ascending order, so the cases of the
# narrow panels are cut into blocks no larger than the panel; at P = 4 the 17 or 24 panels of e = 70
# and 97 must each take a row from above and from below, which few permutations do.
SEEDS: dict[str, int] = {
    "inv8-n4": 4, "ds8-k10-e4": 4, "ds16-e7": 9, "ds16-e8": 2, "ds16-e97": 1,
    "blk16-e4-p4": 3, "blk16-e8-p4": 8, "blk16-e9-p4": 18, "blk16-e70-p4": 68941, "blk16-e97-p4": 34354995,
    "blk16-e8-p8": 2, "blk16-e16-p8": 2, "blk16-e97-p8": 12, "blk16-e16-p16": 2, "blk16-e17-p16": 2,
    "blk16-e97-p16": 4, "blk16-e65-p32": 2, "blk16-e97-p32": 1, "e2e16-k64-e16": 2,
}


def _seed(cid: str) -> int:
    return SEEDS.get(cid, 0)


def _bare(n: int, blocks) -> Case:
    cid = f"inv8-n{n}"
    return Case(cid, 8, n, tuple(blocks), _seed(cid))


def _sys(cid: str, w: int, k: int, n: int, e: int, blocks, panels=()) -> Case:
    return Case(cid, w, e, tuple(blocks), _seed(cid), k, n, tuple(panels))


# gf_invert: the 64-thread form (n <= 32) and the 256-thread form, the LDS opt-in sizes
INVERT = [_bare(4, (1, 2, 1)), _bare(32, (9, 1, 14, 8)), _bare(33, (10, 1, 1, 13, 8)), _bare(97, B97),
          _bare(255, (60, 1, 90, 2, 70, 32)), _bare(256, (33, 100, 1, 1, 90, 31))]
INVERT_BATCH_N = 33
INVERT_BATCH = [INVERT[2], singular_of(INVERT[2], 0), Case("inv8-n33-b", 8, 33, (4, 20, 1, 8), _seed("inv8-n33-b")),
                singular_of(INVERT[2], 16), singular_of(INVERT[2], 32)]

# w = 8 decode_system: (k, n, e); the last is e = k (no native survivors in B')
DS8 = [_sys("ds8-k10-e4", 8, 10, 14, 4, (1, 2, 1)), _sys("ds8-k100-e70", 8, 100, 200, 70, B70),
       _sys("ds8-k128-e97", 8, 128, 256, 97, B97), _sys("ds8-k128-e128", 8, 128, 256, 128, (40, 1, 1, 50, 36))]
DS8_SINGULAR = [singular_of(DS8[1], c) for c in (0, 1, 35, 69)]

# w = 16, one workgroup: e across the lane split's steps (lanes per row 64, 64, 64, 32, 16, 8, 4, 4,
# 4 and, at e = k = 64, 8); each is also run on the blocked solve at its own panel width, 32
DS16 = [_sys("ds16-e1", 16, 5, 8, 1, (1,), (32,)), _sys("ds16-e7", 16, 20, 30, 7, (2, 1, 4), (32,)),
        _sys("ds16-e8", 16, 24, 40, 8, (3, 1, 4), (32,)), _sys("ds16-e9", 16, 17, 30, 9, (4, 1, 1, 3), (32,)),
        _sys("ds16-e20", 16, 33, 60, 20, (6, 1, 9, 4), (32,)), _sys("ds16-e40", 16, 90, 140, 40, B40, (32,)),
        _sys("ds16-e70", 16, 100, 200, 70, B70, (32,)), _sys("ds16-e97", 16, 128, 230, 97, B97, (32,)),
        _sys("ds16-e128", 16, 140, 270, 128, (40, 1, 1, 50, 36), (32,)),
        _sys("ds16-ek64", 16, 64, 130, 64, (20, 1, 30, 13), (32,))]
DS16_EK64 = DS16[-1]


def _blocks_for(e: int, P: int) -> tuple:
    if P == 32:
        return {70: B70, 97: B97}.get(e, split(e, 20, e))
    return split(e, P, 100 * P + e)


def _panel_case(e: int, P: int) -> Case:
    return _sys(f"blk16-e{e}-p{P}", 16, e + 11, 2 * e + 14, e, _blocks_for(e, P), (P,))


# blocked solve: every panel width at one panel, one panel and a column, two panels, two and a
# column, and the two large systems
BLOCKED = [(_panel_case(e, P), P) for P in PANELS for e in (P, P + 1, 2 * P, 2 * P + 1, 70, 97)]
# e % 8 != 0 (row stride 264 symbols for W = 257) and W - c0 across 256: two column blocks in the
# first panel's y / update grids, one in the second's
BLOCKED_ODD = _sys("blk16-e37-k220", 16, 220, 300, 37, (11, 1, 16, 9), (32,))

# late singularity, both w = 16 solvers: the e = 70 system, failing in the first columns, around
# every panel edge and in the last column
LATE = DS16[6]
LATE_COLS = {P: (0, 1, P - 1, P, P + 1, LATE.e - 1) for P in PANELS}
LATE_SINGULAR = {c: singular_of(LATE, c) for c in sorted({c for cols in LATE_COLS.values() for c in cols})}

# end to end through PatternDecoder (the matrix-core engines build their bit-matrix from the
# device-solved rows)
E2E = [_sys("e2e8-k128-e26", 8, 128, 160, 26, (9, 1, 12, 4)), _sys("e2e16-k64-e16", 16, 64, 96, 16, (5, 1, 7, 3))]


def limit_e(supported) -> int:
    """The largest e for which ``supported(2 e, e, e)`` holds (the one-workgroup w = 16 kernel at its
    LDS limit), found by calling it."""
    e = 1
    assert supported(2, 1, 1)
    while supported(2 * (e + 1), e + 1, e + 1):
        e += 1
    return e


def limit_case(e: int) -> Case:
    """The e = k system at (or one past) the one-workgroup kernel's limit. e is only known where the
    native module is loaded, so the seed is searched here: the first whose predicted sequence has no
    gaps at panel width 32 (the tests then hold the simulated one to the same conditions)."""
    blocks = split(e, 40, e)
    for seed in range(1000):
        sigma = planted_sigma(e, seed)
        if not sequence_gaps(predicted_sequence(blocks, sigma), e, (32,)):
            return Case(f"ds16-limit-e{e}", 16, e, blocks, seed, e, 2 * e, (32,))
    raise AssertionError(f"no seed for e = {e}")


def planted_sigma(e: int, seed: int) -> np.ndarray:
    """The permutation :func:`planted` draws, without the field arithmetic."""
    return np.random.default_rng(seed).permutation(e)


def all_cases() -> list[Case]:
    """Every fixed case the GPU module parametrises over (the limit cases are built where the native
    module says what e is)."""
    seen, out = set(), []
    for c in (INVERT + INVERT_BATCH + DS8 + DS8_SINGULAR + DS16 + [c for c, _ in BLOCKED] + [BLOCKED_ODD]
              + list(LATE_SINGULAR.values()) + E2E):
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)
    return out
