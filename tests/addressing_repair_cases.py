"""Shared pieces of tests/test_gpu_addressing_repair.py: four REAL rows longer than 2^32 bytes, the
columns at which they are hit, and the expected reports.

The repair kernels patch single bytes at an ``int64_t`` column (the cold passes of correct and checked
repair), store whole rebuilt rows at ``group * 16`` (checked repair, the batched repair, the
variable-length kernel) and find a work item's column block through a block map (variable-length). A
column or block index cut to 32 bits lands INSIDE the same rows, 2^32 bytes lower, so nothing faults:
the target byte stays wrong and the landing byte becomes wrong. Both show in the syndrome mask of the
whole stripe, which tests/test_gpu_addressing.py pins on rows of this length.

An expected report is the numpy oracle run on the 65,536-byte blocks that hold a hit, summed
(:func:`expect_correct`, :func:`expect_checked`); a CPU test holds that sum to the whole-stripe CPU
paths on short rows.
"""
from __future__ import annotations

import numpy as np
import torch

import addressing_cases as ac
from gpu_rscode_amd import ReedSolomon, gf

P31, P32 = ac.P31, ac.P32
L = ac.WHOLE8            # 2^32 + 16,011: 2^28 + 1,000 sixteen-byte groups and a ragged tail of 11 bytes
BB = 65536               # block_bytes of every mask here
NMASK = -(-L // BB)      # 65,537 words
GUARD = 4096
FILL, ERASED = 0x5A, 0xA5
N = 4
ROW_BYTES = GUARD + L + GUARD + 16
NEED = N * ROW_BYTES + (3 << 29)  # + the scratch of the checks
CODES = {"rs24": (2, 4), "rs14": (1, 4)}  # p = 2: a 2-row tile; p = 3: a 4-row tile, one padding check row
DOUBLE_COL = P32 + 4096 + 1  # the column that gets two flips (beyond a code with max_errors = 1)
APART = P32 + 4096       # item 5: the distance of the two stripes


def codec(code: str) -> ReedSolomon:
    k, n = CODES[code]
    return ReedSolomon(k, n, matrix="cauchy")


# ---- hit columns --------------------------------------------------------------------------------------
def crossing(ptr: int, length: int) -> int:
    """The column (>= 1) of a row at address ``ptr`` whose absolute address is a multiple of 2^32 (the
    arithmetic of ``ac.crossing_window``)."""
    x = (-int(ptr)) % P32
    if x < 1:
        x += P32
    assert 1 <= x < length and (int(ptr) + x) % P32 == 0
    return x


def hit_groups(length: int, ptrs) -> list[list[int]]:
    """The columns every case is hit at, in rows of ``length`` bytes (L, or L - 1 for the byte form), in
    groups that may share a 65,536-byte block: 2^31 - 1, 2^31 + 7 and 2^32 - 1 alone; 2^32 + 5,
    length - 11 (on aligned rows the first tail byte) and length - 1 together (the row ends 16,011 bytes
    past 2^32, so every column from 2^32 on lies in the last, ragged block: no two of them can have a
    block each); and for each address in ``ptrs`` (an input row's, an output row's) the pair ``x - 1``,
    ``x`` with ``x`` the column at which the row's absolute address crosses a 2^32 multiple. No block
    holds columns of two groups: a crossing pair that falls into a block already taken is left out."""
    groups = [[P31 - 1], [P31 + 7], [P32 - 1], [P32 + 5, length - 11, length - 1]]
    for p in ptrs:
        x = crossing(p, length)
        if not {(x - 1) // BB, x // BB} & {c // BB for g in groups for c in g}:
            groups.append([x - 1, x])
    return groups


def hit_columns(length: int, ptrs) -> list[int]:
    return [c for g in hit_groups(length, ptrs) for c in g]


def blocks_of(cols) -> list[int]:
    return sorted({int(c) // BB for c in cols})


# ---- bytes of the hit blocks ----------------------------------------------------------------------------
def fetch(rows, blocks, bb: int = BB) -> dict[int, np.ndarray]:
    """block -> the (n, <= bb) host bytes of that block of every row."""
    length = min(r.numel() for r in rows)
    return {b: np.stack([r[b * bb: min(length, (b + 1) * bb)].cpu().numpy() for r in rows]) for b in blocks}


def store(rows, saved: dict[int, np.ndarray], bb: int = BB) -> None:
    """Write blocks from :func:`fetch` back into every row."""
    for b, a in saved.items():
        for j, r in enumerate(rows):
            r[b * bb: b * bb + a.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(a[j])))


def flip(row: torch.Tensor, col: int, bits: int) -> None:
    row[col: col + 1] ^= bits


def damaged(good: dict[int, np.ndarray], hits, bb: int = BB) -> dict[int, np.ndarray]:
    """The host blocks ``good`` with the flips ``hits`` = [(chunk, column, bits)] applied."""
    out = {b: np.array(a) for b, a in good.items()}
    for j, col, bits in hits:
        out[col // bb][j, col % bb] ^= bits
    return out


def wrong_bytes(got: dict[int, np.ndarray], want: dict[int, np.ndarray], bb: int = BB) -> list[tuple[int, int]]:
    """(row, column) of up to eight bytes of the blocks ``got`` that differ from ``want``."""
    out = []
    for b in sorted(want):
        for j, c in np.argwhere(got[b] != want[b])[:8].tolist():
            out.append((j, b * bb + c))
    return out[:8]


def describe(at) -> str:
    return ", ".join(f"row {j} column {c} ({c:#x}{', above 2^32' if c >= P32 else ''})" for j, c in at)


# ---- expected reports: the oracle on the hit blocks, summed --------------------------------------------------
def expect_correct(h: np.ndarray, bad: dict[int, np.ndarray], max_errors: int, nmask: int, bb: int = BB):
    """``(rows, fixed_bytes, by_weight, uncorrectable, bad_columns, mask)`` of ``gf.correct_oracle`` over
    the damaged blocks ``bad`` of a stripe that is consistent everywhere else: ``rows`` block -> the
    corrected bytes, the counts summed, ``mask`` the ``nmask`` words of ``gf.scrub_oracle`` (zero
    outside the blocks)."""
    n = h.shape[1]
    rows, mask = {}, np.zeros(nmask, dtype=np.int32)
    fixed, by_weight, unc, nbad = np.zeros(n, dtype=np.int64), np.zeros(3, dtype=np.int64), 0, 0
    for b, blk in bad.items():
        rows[b], f, w, u, c = gf.correct_oracle(h, blk, max_errors)
        fixed, by_weight, unc, nbad = fixed + f, by_weight + w, unc + u, nbad + c
        mask[b] = gf.scrub_oracle(h, blk, bb)[0][0]
    return rows, fixed, by_weight, unc, nbad, mask


def expect_checked(h: np.ndarray, bad: dict[int, np.ndarray], erased, max_errors, nmask: int, bb: int = BB):
    """As :func:`expect_correct` for ``gf.reconstruct_checked_oracle`` (the erased rows of ``bad`` are
    never read); the mask from the oracle's T: bit i where check row i, ``T[e + i, S] . stripe[S]``, is
    nonzero in the block."""
    p, n = h.shape
    x = sorted(set(int(e) for e in erased))
    s = [i for i in range(n) if i not in x]
    rows, mask = {}, np.zeros(nmask, dtype=np.int32)
    fixed, by_weight, unc, nbad = np.zeros(n, dtype=np.int64), np.zeros(3, dtype=np.int64), 0, 0
    for b, blk in bad.items():
        rows[b], f, w, u, c, t = gf.reconstruct_checked_oracle(h, blk, x, max_errors)
        fixed, by_weight, unc, nbad = fixed + f, by_weight + w, unc + u, nbad + c
        if len(x) < p:
            mask[b] = gf.scrub_oracle(t[len(x):][:, s], blk[s], bb)[0][0]
    return rows, fixed, by_weight, unc, nbad, mask


def assert_report(rep, want, what) -> None:
    """Every field of a CorrectReport against ``want`` from expect_correct / expect_checked."""
    _, fixed, by_weight, unc, nbad, mask = want
    got = (rep.bad_columns, rep.uncorrectable, rep.fixed_bytes.tolist(), rep.by_weight.tolist())
    assert got == (nbad, unc, fixed.tolist(), by_weight.tolist()), (what, got, (nbad, unc, fixed, by_weight))
    assert rep.clean == (nbad == 0), what
    gm = rep.mask.cpu().numpy()
    assert gm.dtype == np.int32 and gm.shape == mask.shape, (what, gm.shape)
    diff = np.nonzero(gm != mask)[0]
    assert diff.size == 0, (what, "mask words", [(int(b), int(gm[b]), int(mask[b])) for b in diff[:8]])


# ---- the variable-length work list ----------------------------------------------------------------------
def closed_form_blocks(lengths, bytewise: bool) -> np.ndarray:
    """nb per stripe: ``ceil((len // 16 + len % 16) / 256)``, byte form ``ceil(len / 256)``."""
    return np.array([-(-(c if bytewise else c // 16 + c % 16) // 256) for c in lengths], dtype=np.int64)


def lane_bytes(length: int, cb: int, bytewise: bool) -> list[tuple[int, int]]:
    """The [lo, hi) byte ranges the 256 lanes of column block ``cb`` of a stripe of ``length`` bytes
    own, in lane order (gf_varlen.hip's rule): the vector form's lane g = cb * 256 + lane owns group
    g below ``length // 16`` groups, then one tail byte each; the byte form's one byte."""
    out = []
    ngroups, tail = length // 16, length % 16
    for lane in range(256):
        g = cb * 256 + lane
        if bytewise:
            if g < length:
                out.append((g, g + 1))
        elif g < ngroups:
            out.append((16 * g, 16 * g + 16))
        elif g - ngroups < tail:
            out.append((16 * ngroups + g - ngroups, 16 * ngroups + g - ngroups + 1))
    return out


# ---- the four rows ------------------------------------------------------------------------------------
class Rows:
    """Four real rows of L bytes, each in an allocation of its own with GUARD bytes of FILL on either
    side and a 16-byte aligned start; made on first use, given back on :meth:`release`. ``stripe(code)``
    makes them the consistent stripe of that code (natives first): random natives, parity from a
    GemmPlan, compared once per code with the torch reference over the whole rows."""

    def __init__(self):
        self.raw = self.rows = None
        self.code = None
        self.checked: set[str] = set()
        self.rs = {c: codec(c) for c in CODES}

    def acquire(self) -> str | None:
        """None when the rows are there; otherwise why not (too little free device memory)."""
        if self.rows is not None:
            return None
        free, _ = torch.cuda.mem_get_info()
        if free < NEED:
            return f"needs {NEED >> 20} MiB of device memory, {free >> 20} MiB are free"
        self.raw, self.rows = [], []
        for j in range(N):
            raw = torch.empty(ROW_BYTES, dtype=torch.uint8, device="cuda")
            off = (-raw.data_ptr()) % 16
            raw[off: off + GUARD] = FILL
            raw[off + GUARD + L: off + GUARD + L + GUARD] = FILL
            self.raw.append(raw[off: off + GUARD + L + GUARD])
            self.rows.append(self.raw[-1][GUARD: GUARD + L])
            assert self.rows[-1].data_ptr() % 16 == 0
        self.randomise()
        return None

    def release(self) -> None:
        self.raw = self.rows = self.code = None
        for rs in self.rs.values():
            rs._plans.clear()
        torch.cuda.empty_cache()

    def randomise(self) -> None:
        from gpu_rscode_amd.ops import fill_random_

        for j, r in enumerate(self.rows):
            fill_random_(r, ac.SEED + 17 * j)
        self.code = None

    def stripe(self, code: str):
        """(the codec, the four rows) holding a consistent stripe of ``code``."""
        from gpu_rscode_amd.ops import GemmPlan

        rs = self.rs[code]
        if self.code != code:
            GemmPlan(self.rows[: rs.k], self.rows[rs.k:], rs.E).run()
            torch.cuda.synchronize()
            if code not in self.checked:
                got = ac.whole_row_mismatches(8, rs.E, self.rows[: rs.k], self.rows[rs.k:])
                assert got == (0, -1), (code, got)
                self.checked.add(code)
            self.code = code
            self.assert_consistent(rs, f"the fresh {code} stripe")
        return rs, self.rows

    def views(self, shift: int) -> list[torch.Tensor]:
        """The rows from byte ``shift`` on: shift = 1 gives rows one byte off alignment of L - 1 bytes."""
        return [r[shift:] for r in self.rows]

    def assert_guards(self, what) -> None:
        for j, raw in enumerate(self.raw):
            ok = (raw[:GUARD] == FILL).all() & (raw[GUARD + L:] == FILL).all()
            assert bool(ok.item()), f"{what}: a guard of row {j} was written"

    def assert_consistent(self, rs, what) -> None:
        """A zero syndrome mask over all 65,537 words of the aligned rows, and intact guards. A stripe
        found inconsistent is made anew for the tests that follow."""
        mask = rs.syndrome_mask(self.rows, BB)
        assert mask.numel() == NMASK
        dirty = torch.nonzero(mask).reshape(-1).cpu().numpy()
        if dirty.size:
            self.randomise()
            b = int(dirty[0])
            raise AssertionError(f"{what}: {dirty.size} inconsistent blocks, the first block {b} = columns "
                                 f"[{b * BB}, {min(L, (b + 1) * BB)}) ({b * BB:#x}), blocks {dirty[:8].tolist()}")
        self.assert_guards(what)
