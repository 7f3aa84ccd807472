"""Shared cases of tests/test_varlen_scrub.py (CPU) and tests/test_gpu_varlen_scrub.py (GPU): the scrub of
a batch of stripes of differing lengths (``VarlenCodec.syndrome_mask`` / ``scrub`` / ``heal``).

The batches, the guard-filled arena and the consistent stripes are those of tests/varlen_cases.py. What
is expected is always ``gf.scrub_oracle(rs.H, rows_b, block_bytes)`` of each stripe on its own, put side
by side and compared exactly; the oracle of the undamaged batch is computed once per (code, lengths,
block size) and shared. One sweep (a single flipped byte at hundreds of places, ``flip_sweep``) takes the
oracle of the 64 columns around the flipped byte instead of the whole stripe, which is the same thing:
the oracle classifies column by column, and the other columns are those of the undamaged stripe, whose
whole oracle is zero (asserted); its first site per column is checked against the whole stripe too.

Every row is a view of one arena whose guard value (nonzero) stands right after each row, so a read
past ``len[b]`` shows as a dirty bit that the oracle does not have; and after every call the whole arena
must still equal its host image: a scrub reads only.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import varlen_cases as vc
from gpu_rscode_amd import ReedSolomon, VarlenCodec, gf
from gpu_rscode_amd.ops.varlen import GROUP

FULL = vc.FULL
BLOCKS = (4096, 16384, 65536)  # block_bytes: below, at and above the cold pass's span

# the codes: name -> (k, n, matrix). Those that locate (p <= 16), and three for syndrome_mask only.
LOCATING = {
    "c10_14": (10, 14, "cauchy"),
    "c4_6": (4, 6, "cauchy"),
    "c3_4": (3, 4, "cauchy"),       # p = 1: every bad column is unlocated
    "c9_14": (9, 14, "cauchy"),     # p = 5: the 8-row tile
    "c3_19": (3, 19, "cauchy"),     # p = 16
    "v10_14": (10, 14, "vandermonde"),
}
MASK_ONLY = {
    "c19_36": (19, 36, "cauchy"),   # p = 17: two tiles of 16
    "c8_64": (8, 64, "cauchy"),     # p = 56: four tiles, bits 32.. fold onto bits 0..
    "c128_160": (128, 160, "cauchy"),
}
CODES = {**LOCATING, **MASK_ONLY}

# the stripes a single flipped byte is planted in are the first, a middle and the last of this batch;
# the first has columns 16383 and 16384, all three have 4095 and 4096 and a ragged tail
FLIP_LENGTHS = (4 * FULL + GROUP + 3, 300, 0, FULL + GROUP + 2, GROUP + 1, FULL + 3)
FLIP_STRIPES = (0, 3, 5)


@functools.lru_cache(maxsize=None)
def codec(code: str) -> ReedSolomon:
    k, n, matrix = CODES[code]
    return ReedSolomon(k, n, matrix=matrix)


def fresh(code: str) -> ReedSolomon:
    """A codec of the test's own (an empty plan cache)."""
    k, n, matrix = CODES[code]
    return ReedSolomon(k, n, matrix=matrix)


@functools.lru_cache(maxsize=None)
def consistent(code: str, lengths: tuple, seed: int = 0) -> tuple:
    """Consistent stripes ``[n, C_b]`` (read-only): tests/varlen_cases.py's for its codes, the same
    construction for the others."""
    if code in vc.CODES:
        return vc.consistent(code, tuple(lengths), seed)
    rs = codec(code)
    rng = np.random.default_rng([seed, rs.k, rs.n, len(lengths)])
    data = rng.integers(0, 256, size=(rs.k, int(sum(lengths))), dtype=np.uint8)
    full = np.concatenate([data, gf.GF256.gemm(rs.E, data).astype(np.uint8)])
    ends = np.cumsum(lengths)
    out = tuple(np.ascontiguousarray(full[:, e - c: e]) for c, e in zip(lengths, ends))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the oracle ----------------------------------------------------------------------------------------
class Want:
    """The oracle of a batch: ``words[b]`` int32, and ``votes [B, n]``, ``unlocated [B]``, ``bad [B]``."""

    def __init__(self, n: int, lengths, block_bytes: int):
        self.block_bytes = block_bytes
        self.words = [np.zeros(-(-int(c) // block_bytes), dtype=np.int32) for c in lengths]
        self.votes = np.zeros((len(lengths), n), dtype=np.int64)
        self.unlocated = np.zeros(len(lengths), dtype=np.int64)
        self.bad = np.zeros(len(lengths), dtype=np.int64)

    def copy(self) -> "Want":
        w = Want.__new__(Want)
        w.block_bytes, w.words = self.block_bytes, [x.copy() for x in self.words]
        w.votes, w.unlocated, w.bad = self.votes.copy(), self.unlocated.copy(), self.bad.copy()
        return w

    def set(self, b: int, stripe: np.ndarray, h: np.ndarray) -> None:
        """Stripe b's entry from ``gf.scrub_oracle`` of the whole stripe."""
        if stripe.shape[1] == 0:
            return
        self.words[b], self.votes[b], self.unlocated[b], self.bad[b] = gf.scrub_oracle(h, stripe, self.block_bytes)

    @property
    def offsets(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum([w.size for w in self.words])]).astype(np.int64)

    @property
    def blocks(self) -> np.ndarray:
        return np.concatenate(self.words + [np.zeros(0, dtype=np.int32)])

    @property
    def stripes(self) -> np.ndarray:
        return np.array([np.bitwise_or.reduce(w) if w.size else 0 for w in self.words], dtype=np.int32)


def oracle(code: str, stripes, block_bytes: int) -> Want:
    rs = codec(code)
    want = Want(rs.n, [s.shape[1] for s in stripes], block_bytes)
    for b, s in enumerate(stripes):
        want.set(b, s, rs.H)
    return want


@functools.lru_cache(maxsize=None)
def _clean_oracle(code: str, lengths: tuple, block_bytes: int, seed: int) -> Want:
    want = oracle(code, consistent(code, lengths, seed), block_bytes)
    assert not want.blocks.any() and not want.bad.any(), "the undamaged batch is consistent"
    return want


def damaged_oracle(code: str, lengths, block_bytes: int, bad: dict, seed: int = 0) -> Want:
    """The oracle of the consistent batch with the stripes ``bad`` (index -> damaged stripe) in place of
    its own: the shared oracle of the undamaged batch, and ``gf.scrub_oracle`` of each damaged stripe."""
    want = _clean_oracle(code, tuple(lengths), block_bytes, seed).copy()
    for b, s in bad.items():
        want.set(b, s, codec(code).H)
    return want


# ---- comparing --------------------------------------------------------------------------------------------
def check_mask(what: str, mask, want: Want) -> None:
    assert np.array_equal(mask.offsets, want.offsets), (what, mask.offsets, want.offsets)
    assert mask.blocks.dtype == torch.int32 and mask.stripes.dtype == torch.int32
    got, stripes = mask.blocks.cpu().numpy(), mask.stripes.cpu().numpy()
    assert got.shape == want.blocks.shape and stripes.shape == want.stripes.shape, (what, got.shape, stripes.shape)
    if not np.array_equal(got, want.blocks):
        w = int(np.flatnonzero(got != want.blocks)[0])
        b = int(np.searchsorted(want.offsets, w, side="right")) - 1
        raise AssertionError(f"{what}: block word {w} (stripe {b}, its word {w - int(want.offsets[b])}): got "
                             f"{int(got[w]):#x}, want {int(want.blocks[w]):#x}")
    assert np.array_equal(stripes, want.stripes), (what, "stripe words", stripes, want.stripes)
    for b in sorted({0, len(want.words) // 2, len(want.words) - 1}) if want.words else ():
        assert np.array_equal(mask.of(b).cpu().numpy(), want.words[b]), (what, "of", b)


def check_report(what: str, rep, want: Want) -> None:
    check_mask(what, rep.mask, want)
    assert np.array_equal(rep.votes, want.votes), (what, "votes", np.argwhere(rep.votes != want.votes)[:4])
    assert np.array_equal(rep.unlocated, want.unlocated), (what, "unlocated", rep.unlocated, want.unlocated)
    assert np.array_equal(rep.bad_columns, want.bad), (what, "bad columns", rep.bad_columns, want.bad)
    assert np.array_equal(rep.clean, want.bad == 0) and rep.dirty == np.flatnonzero(want.bad).tolist(), what
    assert rep.unhealed == [] and len(rep.report) == len(want.words)


def check_single(what: str, rs: ReedSolomon, rep, rows_of, stripes, block_bytes: int) -> None:
    """``report[b]`` field for field against ``rs.scrub`` on stripe b alone (``rows_of(b)``: its n rows),
    and ``report[b].mask`` against ``rs.syndrome_mask``."""
    for b in stripes:
        single, r = rs.scrub(rows_of(b), block_bytes=block_bytes), rep.report[b]
        assert (single.clean, single.bad_columns, single.unlocated, single.suspects) == \
            (r.clean, r.bad_columns, r.unlocated, r.suspects), (what, b)
        assert np.array_equal(single.votes, r.votes), (what, b)
        assert torch.equal(single.mask, r.mask), (what, b)
        assert torch.equal(rs.syndrome_mask(rows_of(b), block_bytes=block_bytes), r.mask), (what, b)


# ---- batches -------------------------------------------------------------------------------------------------
def upload(code: str, stripes, device: str, **kw) -> vc.Batch:
    """The stripes as views of one guard-filled arena, uploaded."""
    batch = vc.Batch(codec(code).n, [s.shape[1] for s in stripes], device, **kw)
    if batch.packed:
        batch.put_packed(np.concatenate(stripes, axis=1)) if len(stripes) else None
    else:
        batch.put(stripes)
    batch.upload()
    return batch


def rows_of(batch: vc.Batch):
    """b -> the n rows of stripe b of the batch, in whatever form it is."""
    if batch.packed:
        off = batch.offsets
        return lambda b: [batch.arg[j, int(off[b]): int(off[b + 1])] for j in range(batch.nrows)]
    return lambda b: list(batch.arg[b])


def noise(seed, *shape) -> np.ndarray:
    """Nonzero bytes: XORed in, every byte changes."""
    return np.random.default_rng(seed).integers(1, 256, size=shape, dtype=np.uint8)


def overwritten(good, b: int, chunk: int, seed: int = 7) -> np.ndarray:
    a = np.array(good[b])
    a[chunk] ^= noise([seed, b, chunk], a.shape[1])
    return a


def run_damage(device: str, code: str, lengths, block_bytes: int, locate: bool, **kw) -> None:
    """None, one overwritten chunk, two damaged chunks (in the first, a middle and the last stripe of
    some bytes at once: every OTHER stripe must come out with zero words and zero counts, which the
    shared oracle of the undamaged batch says)."""
    rs = fresh(code)
    vl = VarlenCodec(rs)
    good = consistent(code, tuple(lengths))
    live = [b for b, c in enumerate(lengths) if c]
    hit = sorted({live[0], live[len(live) // 2], live[-1]}) if live else []
    cases = {"none": {}}
    cases["one overwritten chunk"] = {b: overwritten(good, b, (3 * b + 1) % rs.n) for b in hit}
    two = {}
    for b in hit:
        a = overwritten(good, b, (5 * b) % rs.n)
        c = lengths[b]
        a[(5 * b + 2) % rs.n, c // 2:] ^= noise([9, b], c - c // 2)  # (the second half: both kinds of column)
        two[b] = a
    cases["two damaged chunks"] = two
    for name, bad in cases.items():
        what = f"{code} {tuple(lengths)[:6]} block {block_bytes}: {name}"
        batch = upload(code, [bad.get(b, good[b]) for b in range(len(good))], device, **kw)
        want = damaged_oracle(code, lengths, block_bytes, bad)
        check_mask(what, vl.syndrome_mask(batch.arg, block_bytes=block_bytes, **batch.kw()), want)
        batch.check(what + ": syndrome_mask wrote")
        if locate:
            rep = vl.scrub(batch.arg, block_bytes=block_bytes, **batch.kw())
            check_report(what, rep, want)
            check_single(what, rs, rep, rows_of(batch), hit[:1] + live[1:2], block_bytes)
            batch.check(what + ": scrub wrote")


def flip_columns(length: int) -> list:
    """The columns a single byte is flipped at, of those the stripe has."""
    groups = length // GROUP
    cols = [0, length - 1, groups * GROUP - 1, groups * GROUP, FULL - 1, FULL, 4 * FULL - 1, 4 * FULL]
    return sorted({c for c in cols if 0 <= c < length})


def flip_sweep(device: str, code: str, block_bytes: int, locate: bool = True) -> int:
    """One flipped byte in every chunk in turn, in the first, a middle and the last stripe of
    FLIP_LENGTHS, at every column of ``flip_columns``: per call one site in each of the three stripes
    (other chunks, so that a leak between them shows), flipped on the device and flipped back. Returns
    the number of calls."""
    rs = fresh(code)
    vl = VarlenCodec(rs)
    good = consistent(code, FLIP_LENGTHS)
    batch = upload(code, good, device)
    clean = _clean_oracle(code, FLIP_LENGTHS, block_bytes, 0)
    rows = rows_of(batch)
    calls, h = 0, rs.H
    ncols = max(len(flip_columns(FLIP_LENGTHS[b])) for b in FLIP_STRIPES)
    for t in range(ncols):
        for chunk in range(rs.n):
            want, sites = clean.copy(), []
            for i, b in enumerate(FLIP_STRIPES):
                cols = flip_columns(FLIP_LENGTHS[b])
                if t >= len(cols):
                    continue
                j, c, v = (chunk + 5 * i) % rs.n, cols[t], 1 + (chunk * 37 + 11 * t + i) % 255
                sites.append((b, j, c, v))
                lo = c // 64 * 64
                window = np.array(good[b][:, lo: lo + 64])
                window[j, c - lo] ^= v
                words, want.votes[b], want.unlocated[b], want.bad[b] = gf.scrub_oracle(h, window, block_bytes)
                want.words[b][c // block_bytes] = words[0]
                if chunk == 0:  # the same from the whole stripe
                    a = np.array(good[b])
                    a[j, c] ^= v
                    whole = gf.scrub_oracle(h, a, block_bytes)
                    assert np.array_equal(whole[0], want.words[b]) and np.array_equal(whole[1], want.votes[b])
                    assert whole[2:] == (want.unlocated[b], want.bad[b])
            for b, j, c, v in sites:
                rows(b)[j][c] ^= v
                batch.image[batch.off[b, j] + c] ^= v
            what = f"{code} block {block_bytes}: flips (stripe, chunk, column, value) {sites}"
            if locate:
                check_report(what, vl.scrub(batch.arg, block_bytes=block_bytes), want)
            else:
                check_mask(what, vl.syndrome_mask(batch.arg, block_bytes=block_bytes), want)
            calls += 1
            for b, j, c, v in sites:
                rows(b)[j][c] ^= v
                batch.image[batch.off[b, j] + c] ^= v
        batch.check(f"{code} block {block_bytes}: after the flips at column set {t}")
    return calls


def error_values(device: str, code: str, block_bytes: int) -> None:
    """Every error value 1..255 once: 255 columns of the last stripe of FLIP_LENGTHS and of the first,
    the chunk going round, one call."""
    rs = fresh(code)
    good = consistent(code, FLIP_LENGTHS)
    bad = {b: np.array(good[b]) for b in (FLIP_STRIPES[0], FLIP_STRIPES[-1])}
    for b, a in bad.items():
        cols = np.random.default_rng([b, 255]).permutation(a.shape[1])[:255]
        for v, c in enumerate(cols, start=1):
            a[(v + b) % rs.n, c] ^= v
    batch = upload(code, [bad.get(b, good[b]) for b in range(len(good))], device)
    want = damaged_oracle(code, FLIP_LENGTHS, block_bytes, bad)
    assert want.bad[FLIP_STRIPES[0]] == 255 and want.bad[FLIP_STRIPES[-1]] == 255
    what = f"{code} block {block_bytes}: every error value"
    check_report(what, VarlenCodec(rs).scrub(batch.arg, block_bytes=block_bytes), want)
    batch.check(what)
