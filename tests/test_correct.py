"""Correct on CPU tensors: ``ReedSolomon.correct`` and the plans' decoding rule against the numpy oracle
(``gf.correct_oracle``), exactly: the rows, every report field, the mask before correction and, where
nothing is uncorrectable, a clean and restored stripe afterwards. The case functions take the device,
so tests/test_gpu_correct.py runs the same cases through the gfx950 kernel."""
import itertools
from functools import lru_cache

import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, UnrecoverableError, flat_rows, gf
from gpu_rscode_amd.ops.correct import MAX_PAIR_N, CorrectPlan, CorrectReport, cpu_correct, make_correct_report
from test_scrub import GARBAGE, code_id, codec, host_stripe, mixed_check_matrix, stripe_bytes, to_device, unaligned_rows

assert MAX_PAIR_N >= 64
VAND, CAUCHY = (10, 14, "vandermonde"), (10, 14, "cauchy")
WIDE, TOO_WIDE = (MAX_PAIR_N - 4, MAX_PAIR_N, "cauchy"), (MAX_PAIR_N - 3, MAX_PAIR_N + 1, "cauchy")
# the rows-in-flight syndrome instance, twice | p = 4 and p = 2 (max_errors 1 only) | p = 5: the 8-row
# tile with padding rows | p = 16: the full tile | the widest pair search | one past it: singles only
CODES = [VAND, CAUCHY, (4, 8, "cauchy"), (4, 6, "cauchy"), (9, 14, "cauchy"), (3, 19, "cauchy"), WIDE, TOO_WIDE]
# a lone byte | around a 32-bit word | a wave | a mask block of 4096 | the locate span | a block of 65536
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 65538, 65539]
EDGES = [4, 64, 4096, 16384, 65536]
# the oracle's cost grows with n p C: the two wide codes keep one length of each kind
SINGLE_RUNS = [(c, s) for c in CODES for s in (LENGTHS if c[1] <= 19 else [1, 5, 65, 4097, 16385])]


def run_id(r):
    return f"{code_id(r[0])}-C{r[1]}"


def block_bytes_for(ncols: int) -> int:
    return 65536 if ncols > 16385 else 4096


def default_max_errors(p: int) -> int:
    return min(2, p // 2)


def correct_with(device, h, rows, max_errors, block_bytes) -> CorrectReport:
    """A stripe corrected under any p x n check matrix ``h``: a CorrectPlan on CUDA rows, cpu_correct
    on CPU rows."""
    h = np.asarray(h, dtype=np.uint8)
    rows = [rows[i] for i in range(len(rows))]
    if torch.device(device).type == "cuda":
        return CorrectPlan(rows, h, max_errors, block_bytes).correct()
    ncols = min(r.numel() for r in rows)
    mask, *counts = cpu_correct(h, rows, ncols, block_bytes, max_errors, codec(VAND)._cpu_gemm)
    return make_correct_report(*counts, mask)


def assert_report(rep: CorrectReport, h, bad: np.ndarray, max_errors: int, block_bytes: int, mask=True):
    """Every field of ``rep`` against the oracle's on the damaged stripe ``bad``; returns the oracle's
    result."""
    want = gf.correct_oracle(h, bad, max_errors)
    _, fixed, by_weight, uncorrectable, bad_columns = want
    assert isinstance(rep, CorrectReport)
    assert (rep.clean, rep.bad_columns, rep.uncorrectable) == (bad_columns == 0, bad_columns, uncorrectable)
    assert rep.fixed_bytes.dtype == np.int64 and np.array_equal(rep.fixed_bytes, fixed), (rep.fixed_bytes, fixed)
    assert rep.by_weight.dtype == np.int64 and np.array_equal(rep.by_weight, by_weight), (rep.by_weight, by_weight)
    if mask:
        assert rep.mask.dtype == torch.int32
        assert np.array_equal(rep.mask.cpu().numpy(), gf.scrub_oracle(h, bad, block_bytes)[0])
    return want


def assert_corrected(rs, stripe, bad, good, max_errors=None, block_bytes=4096):
    """``rs.correct`` on ``stripe`` (holding ``bad``): the oracle's rows and report; with nothing
    uncorrectable, a clean mask afterwards and the undamaged stripe."""
    me = default_max_errors(rs.p) if max_errors is None else max_errors
    rep = rs.correct(stripe, max_errors, block_bytes)
    want = assert_report(rep, rs.H, bad, me, block_bytes)
    after = stripe_bytes(stripe)
    assert np.array_equal(after, want[0])
    if rep.uncorrectable == 0:
        assert not rs.syndrome_mask(stripe, block_bytes).cpu().numpy().any()
        assert good is None or np.array_equal(after, good)  # (None: a planted miscorrection)
    return rep


def damage(stripe, bad: np.ndarray, j: int, cols, vals) -> None:
    """XOR ``vals`` into chunk j at ``cols``, on the device stripe and in its host copy."""
    cols, vals = np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.uint8)
    bad[j, cols] ^= vals
    row = stripe[j]
    row[torch.from_numpy(cols).to(row.device)] = torch.from_numpy(bad[j, cols]).to(row.device)


def edge_columns(ncols: int) -> list[int]:
    """The first and the last column and both sides of every edge inside the row."""
    return sorted({c for c in [0, ncols - 1] + [e - 1 for e in EDGES] + EDGES if 0 <= c < ncols})


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_clean(device, code, ncols):
    rs = codec(code)
    good = host_stripe(code, ncols)
    stripe = to_device(good, device)
    me = 1 if code == TOO_WIDE else None
    rep = assert_corrected(rs, stripe, good, good, me, block_bytes_for(ncols))
    assert rep.clean and not rep.fixed_bytes.any() and not rep.by_weight.any() and not rep.mask.cpu().numpy().any()


def case_singles(device, code, ncols):
    """One wrong chunk per column, for every chunk in turn: errors 1, 255 and random values at the
    first and last column and on each side of every edge. Each call restores the stripe, which the
    next chunk then damages again."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    stripe = to_device(good, device)
    cols = edge_columns(ncols)
    rng = np.random.default_rng(ncols + rs.n)
    me = 1 if code == TOO_WIDE else None
    chunks = range(rs.n) if rs.n <= 19 else sorted({0, 1, rs.k - 1, rs.k, rs.n - 1, *rng.choice(rs.n, 6).tolist()})
    for j in chunks:
        bad = np.array(good)
        vals = [(1, 255, int(rng.integers(1, 256)))[(t + j) % 3] for t in range(len(cols))]
        damage(stripe, bad, j, cols, vals)
        rep = assert_corrected(rs, stripe, bad, good, me, block_bytes_for(ncols))
        assert rep.uncorrectable == 0 and rep.by_weight.tolist() == [0, len(cols), 0]
        assert rep.fixed_bytes.tolist() == [len(cols) * int(i == j) for i in range(rs.n)]


def every_pair_stripe(good: np.ndarray):
    """All pairs of the n = 8 chunks, 37 columns each: chunk a's value in column u of its x-th pair is
    1 + (37 x + u) % 255, so every chunk sees every error value 1..255 (7 pairs of 37 columns)."""
    n = good.shape[0]
    pairs = list(itertools.combinations(range(n), 2))
    assert good.shape[1] == 37 * len(pairs) + 5
    bad = np.array(good)
    nth = [0] * n
    seen = [set() for _ in range(n)]
    for t, pair in enumerate(pairs):
        for j in pair:
            vals = 1 + (37 * nth[j] + np.arange(37)) % 255
            bad[j, 37 * t: 37 * t + 37] ^= vals.astype(np.uint8)
            seen[j].update(vals.tolist())
            nth[j] += 1
    assert all(s == set(range(1, 256)) for s in seen)
    return bad, 37 * len(pairs)


def case_every_pair_every_value(device, mixed: bool):
    """(4, 8), the check matrix handed to the plan: the codec's [E | I], or M . H without an identity
    block. All 28 pairs, every error value in every chunk: every column is a weight-2 correction."""
    code = (4, 8, "cauchy")
    h = mixed_check_matrix(code) if mixed else codec(code).H
    good = host_stripe(code, 37 * 28 + 5)
    bad, ndouble = every_pair_stripe(good)
    stripe = to_device(bad, device)
    rep = correct_with(device, h, stripe, 2, 4096)
    want = assert_report(rep, h, bad, 2, 4096)
    assert np.array_equal(stripe_bytes(stripe), want[0]) and np.array_equal(want[0], good)
    assert rep.by_weight.tolist() == [0, 0, ndouble] and rep.uncorrectable == 0
    assert rep.fixed_bytes.tolist() == [7 * 37] * 8


def doubles_stripe(code, ncols=4101):
    """(good, bad, counts): 14 singles, every chunk pair twice with random values (182 doubles) and
    40 random triples, each in a column of its own, spread over two mask blocks of 4096."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    rng = np.random.default_rng(14)
    cols = iter(rng.permutation(ncols)[: rs.n + 182 + 40].tolist())
    for j in range(rs.n):
        bad[j, next(cols)] ^= rng.integers(1, 256)
    for a, b in list(itertools.combinations(range(rs.n), 2)) * 2:
        c = next(cols)
        bad[a, c] ^= rng.integers(1, 256)
        bad[b, c] ^= rng.integers(1, 256)
    for _ in range(40):
        c = next(cols)
        for j in rng.choice(rs.n, 3, replace=False):
            bad[j, c] ^= rng.integers(1, 256)
    return good, bad


def case_doubles(device, code):
    """On (10, 14): singles and doubles are restored, triples left untouched; with max_errors=1 only
    the singles are."""
    rs = codec(code)
    good, bad = doubles_stripe(code)
    wrong = (bad != good).any(axis=0)
    assert int(wrong.sum()) == 14 + 182 + 40
    stripe = to_device(bad, device)
    rep = assert_corrected(rs, stripe, bad, good, None, 4096)
    assert rep.by_weight.tolist() == [0, 14, 182] and rep.uncorrectable == 40 and rep.bad_columns == 236
    after = stripe_bytes(stripe)
    triples = ((bad != good).sum(axis=0) == 3)
    assert np.array_equal(after[:, triples], bad[:, triples]) and np.array_equal(after[:, ~triples], good[:, ~triples])
    stripe = to_device(bad, device)
    rep = assert_corrected(rs, stripe, bad, good, 1, 4096)
    assert rep.by_weight.tolist() == [0, 14, 0] and rep.uncorrectable == 222
    singles = ((bad != good).sum(axis=0) == 1)
    after = stripe_bytes(stripe)
    assert np.array_equal(after[:, singles], good[:, singles]) and np.array_equal(after[:, ~singles], bad[:, ~singles])


def case_scattered(device, code=VAND, ncols=4101):
    """One wrong byte in each of five chunks, in different columns: five suspects are more than p = 4,
    so heal refuses; correct restores the stripe byte by byte."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    hits = {0: 17, 3: 1000, 7: 4095, 11: 4096, 13: ncols - 1}
    for t, (j, c) in enumerate(hits.items()):
        bad[j, c] ^= 0x11 * (t + 1)
    copy = to_device(bad, device)
    with pytest.raises(UnrecoverableError):
        rs.heal(copy)
    assert np.array_equal(stripe_bytes(copy), bad)
    stripe = to_device(bad, device)
    rep = assert_corrected(rs, stripe, bad, good)
    assert rep.fixed_bytes.tolist() == [int(j in hits) for j in range(rs.n)]
    assert rep.by_weight.tolist() == [0, 5, 0] and (rep.uncorrectable, rep.bad_columns, rep.clean) == (0, 5, False)
    assert np.array_equal(stripe_bytes(stripe), good)


def null_vector(a: np.ndarray) -> np.ndarray:
    """v with a . v = 0 and v[-1] = 1, for a p x m matrix whose first m - 1 columns are independent."""
    f = gf.GF256
    m = a.shape[1]
    for rows in itertools.combinations(range(a.shape[0]), m - 1):
        sub = a[list(rows), : m - 1]
        if f.is_invertible(sub):
            x = f.matmul(f.invert(sub), a[list(rows), m - 1:])[:, 0]
            v = np.concatenate([x, [1]]).astype(np.uint8)
            assert not f.gemm(a, v[:, None]).any()
            return v
    raise AssertionError("no independent m - 1 columns")


@lru_cache(maxsize=None)
def dependent_four_set(code):
    """The first four dependent columns of the code's H, found here; no three may be dependent."""
    h = codec(code).H
    f = gf.GF256
    for cols in itertools.combinations(range(h.shape[1]), 4):
        if not f.is_invertible(h[:, list(cols)]):
            return cols
    return None


def case_planted_ambiguity(device):
    """The reference Vandermonde H has dependent 4-sets of columns. The null vector's first two values
    on the first two chunks of one are also explained by the other two chunks: uncorrectable and
    unchanged. Other values at the same two chunks are corrected."""
    rs = codec(VAND)
    cols = dependent_four_set(VAND)
    assert cols is not None and dependent_four_set(CAUCHY) is None
    v = null_vector(rs.H[:, list(cols)])
    assert v.all()
    good = host_stripe(VAND, 4101)
    bad = np.array(good)
    bad[cols[0], 100] ^= v[0]
    bad[cols[1], 100] ^= v[1]
    bad[cols[0], 4097] ^= v[0] ^ 0x01 or 0x02
    bad[cols[1], 4097] ^= v[1]
    stripe = to_device(bad, device)
    rep = assert_corrected(rs, stripe, bad, good)
    assert (rep.uncorrectable, rep.bad_columns) == (1, 2) and rep.by_weight.tolist() == [0, 0, 1]
    after = stripe_bytes(stripe)
    assert np.array_equal(after[:, 100], bad[:, 100]) and np.array_equal(after[:, 4097], good[:, 4097])
    assert rep.fixed_bytes.tolist() == [int(j in cols[:2]) for j in range(rs.n)]


def case_planted_miscorrection(device):
    """Three errors beyond the code: any five columns of the Cauchy H are dependent, so three of a null
    vector's values on three chunks look like the other two values on the other two chunks. The
    column becomes consistent and wrong, as the oracle's does."""
    rs = codec(CAUCHY)
    v = null_vector(rs.H[:, :5])
    assert v.all()
    good = host_stripe(CAUCHY, 4101)
    bad = np.array(good)
    for j in range(3):
        bad[j, 4099] ^= v[j]
    stripe = to_device(bad, device)
    rep = assert_corrected(rs, stripe, bad, good=None)  # (uncorrectable == 0, but not restored: checked below)
    assert rep.by_weight.tolist() == [0, 0, 1] and rep.uncorrectable == 0
    assert rep.fixed_bytes.tolist() == [0, 0, 0, 1, 1] + [0] * 9
    after = stripe_bytes(stripe)
    want = np.array(bad)
    want[3, 4099] ^= v[3]
    want[4, 4099] ^= v[4]
    assert np.array_equal(after, want) and not np.array_equal(after, good)
    assert not gf.GF256.gemm(rs.H, after).any()


def guarded_rows(host, device, guard=64):
    """Separately allocated rows with ``guard`` bytes of garbage on either side; (rows, buffers)."""
    ncols = host.shape[1]
    bufs = [torch.full((guard + ncols + guard,), GARBAGE, dtype=torch.uint8, device=device) for _ in range(host.shape[0])]
    rows = [b[guard: guard + ncols] for b in bufs]
    for r, src in zip(rows, host):
        r.copy_(torch.from_numpy(np.array(src)))
    return rows, bufs


def case_untouched(device, code=VAND, ncols=65539):
    """Pitch padding keeps its fill and guarded buffers their guards; every byte outside the patched
    ones is as it was (the rows equal the oracle's, whose clean columns are the input's)."""
    rs = codec(code)
    good, bad = doubles_stripe(code, ncols)
    stripe = to_device(bad, device)
    flat_before = flat_rows(stripe).cpu().numpy().copy()
    rep = assert_corrected(rs, stripe, bad, good, None, 65536)
    assert rep.uncorrectable >= 40 and rep.by_weight[2] + rep.uncorrectable == 222  # (the triples stay)
    flat_after = flat_rows(stripe).cpu().numpy()
    pitch = stripe.stride(0)
    pad = np.ones(flat_after.size, dtype=bool)
    for j in range(rs.n):
        pad[j * pitch: j * pitch + ncols] = False
    assert pad.any() and (flat_after[pad] == GARBAGE).all()
    assert np.array_equal(flat_after[pad], flat_before[pad])
    rows, bufs = guarded_rows(bad, device)
    assert_corrected(rs, rows, bad, good, None, 4096)
    for b in bufs:
        host = b.cpu().numpy()
        assert (host[:64] == GARBAGE).all() and (host[-64:] == GARBAGE).all()


def short_damage(code, ncols):
    """(good, bad) for rows shorter than doubles_stripe needs: two singles and a double."""
    good = host_stripe(code, ncols)
    bad = np.array(good)
    bad[0, 0] ^= 1
    bad[13, ncols - 1] ^= 255
    bad[4, 7] ^= 0x31
    bad[9, 7] ^= 0x13
    return good, bad


def case_unaligned(device, code, ncols):
    """A row one byte off alignment puts the call on the byte form: the same result."""
    rs = codec(code)
    good, bad = doubles_stripe(code, ncols) if ncols >= 236 else short_damage(code, ncols)
    rows = unaligned_rows(bad, device)
    aligned = to_device(bad, device)
    for bb in (4096, 65536):
        rep = assert_corrected(rs, rows, bad, good, None, bb)
        ref = rs.correct(aligned, block_bytes=bb)
        assert np.array_equal(rep.fixed_bytes, ref.fixed_bytes) and np.array_equal(rep.by_weight, ref.by_weight)
        assert (rep.uncorrectable, rep.bad_columns) == (ref.uncorrectable, ref.bad_columns)
        assert rep.by_weight[2] > 0
        assert np.array_equal(rep.mask.cpu().numpy(), ref.mask.cpu().numpy())
        assert np.array_equal(stripe_bytes(rows), stripe_bytes(aligned))
        for j, r in enumerate(rows):  # damaged again for the second block size
            r.copy_(torch.from_numpy(bad[j]))
        aligned.copy_(torch.from_numpy(bad))


def case_refusals(device):
    """What correct refuses, with the buffers unchanged after each refusal."""
    for field in ("gf16", "gf65536"):
        rs = ReedSolomon(4, 8, matrix="cauchy", field=field)
        stripe = torch.full((8, 64), 7, dtype=torch.uint8, device=device)
        with pytest.raises(NotImplementedError, match=field):
            rs.correct(stripe)
        assert (stripe == 7).all()

    def refused(code, exc, ncols=4101, **kw):
        bad = np.array(host_stripe(code, ncols))
        bad[1, 9] ^= 0x10
        stripe = to_device(bad, device)
        with pytest.raises(exc):
            codec(code).correct(stripe, **kw)
        assert np.array_equal(stripe_bytes(stripe), bad)

    for me in (0, 3, -1, 1.5, "2", True):
        refused(VAND, ValueError, max_errors=me)
    refused((4, 6, "cauchy"), ValueError, max_errors=2)  # p = 2
    refused((3, 4, "vandermonde"), ValueError)  # p = 1
    refused((3, 4, "vandermonde"), ValueError, max_errors=1)
    refused((19, 36, "cauchy"), NotImplementedError, ncols=17)  # p = 17
    refused((19, 36, "cauchy"), NotImplementedError, ncols=17, max_errors=1)
    refused(TOO_WIDE, NotImplementedError, ncols=65)  # the default is 2
    refused(TOO_WIDE, NotImplementedError, ncols=65, max_errors=2)
    for bb in (0, 2048, 4097, 3 * 4096):
        refused(VAND, ValueError, block_bytes=bb)
    with pytest.raises(ValueError):  # p = 0
        ReedSolomon(4, 4).correct(torch.zeros((4, 64), dtype=torch.uint8, device=device))

    rs = codec(VAND)
    bad = np.array(host_stripe(VAND, 4101))
    bad[1, 9] ^= 0x10
    stripe = to_device(bad, device)
    rows = [stripe[j] for j in range(rs.n)]
    buf = torch.full((4101 + 100,), 3, dtype=torch.uint8, device=device)
    twice = rows[:5] + [rows[2]] + rows[6:]  # one row listed twice
    partly = rows[:12] + [buf[:4101], buf[100:]]  # two rows that share 4001 bytes
    for arg in (twice, partly, rows[:13], stripe[:, :4100].to(torch.int8)):
        with pytest.raises(ValueError):
            rs.correct(arg)
    assert np.array_equal(stripe_bytes(stripe), bad) and (buf == 3).all()
    rep = rs.correct(stripe)
    assert rep.fixed_bytes.tolist() == [0, 1] + [0] * 12 and rep.uncorrectable == 0


def case_empty(device):
    """A stripe of no bytes: an empty mask and zero counts."""
    rs = codec(VAND)
    rep = rs.correct(torch.zeros((14, 0), dtype=torch.uint8, device=device))
    assert rep.clean and rep.mask.numel() == 0 and not rep.fixed_bytes.any() and rep.uncorrectable == 0


def case_pairs_on(device, code, ncols=4101):
    """p = 5, p = 16 and n = MAX_PAIR_N: double errors in the first and last chunk, across the native /
    parity border and in neighbours, next to a single."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    rng = np.random.default_rng(rs.n)
    pairs = [(0, rs.n - 1), (rs.k - 1, rs.k), (0, 1), (rs.n - 2, rs.n - 1), (1, rs.k)]
    for t, (a, b) in enumerate(pairs):
        c = [0, 4095, 4096, 4100, 77][t]
        bad[a, c] ^= rng.integers(1, 256)
        bad[b, c] ^= rng.integers(1, 256)
    bad[2, 5] ^= 0xFF
    stripe = to_device(bad, device)
    rep = assert_corrected(rs, stripe, bad, good, 2, 4096)
    assert rep.by_weight.tolist() == [0, 1, 5] and rep.uncorrectable == 0


# ---- the CPU tests ------------------------------------------------------------------------------------
def test_oracle_on_a_hand_made_stripe():
    """The oracle itself, against values worked out from the definition."""
    rs = codec((4, 8, "cauchy"))
    good = host_stripe((4, 8, "cauchy"), 16)
    bad = np.array(good)
    bad[2, 3] ^= 0x55           # weight 1, a native
    bad[6, 5] ^= 0xAA           # weight 1, a parity chunk
    bad[0, 9] ^= 0x01           # weight 2
    bad[7, 9] ^= 0xFF
    bad[1, 12] ^= 0x10          # weight 3: beyond max_errors, left alone or miscorrected, never restored
    bad[2, 12] ^= 0x20
    bad[3, 12] ^= 0x30
    rows, fixed, by_weight, unc, nbad = gf.correct_oracle(rs.H, bad, 2)
    assert nbad == 4 and by_weight[1] == 2 and by_weight[0] == 0 and by_weight[2] + unc == 2 and by_weight[2] >= 1
    assert np.array_equal(rows[:, :12], good[:, :12]) and not np.array_equal(rows[:, 12], good[:, 12])
    assert fixed[6] == 1 and fixed[7] >= 1 and fixed.sum() == 2 + 2 * by_weight[2]
    rows1, fixed1, by_weight1, unc1, nbad1 = gf.correct_oracle(rs.H, bad, 1)
    assert (by_weight1.tolist(), unc1, nbad1) == ([0, 2, 0], 2, 4) and fixed1.tolist() == [0, 0, 1, 0, 0, 0, 1, 0]
    assert np.array_equal(rows1[:, 9], bad[:, 9]) and np.array_equal(rows1[:, :9], good[:, :9])
    assert np.array_equal(rows1[:, 12], bad[:, 12])
    for me in (0, 3):
        with pytest.raises(ValueError):
            gf.correct_oracle(rs.H, bad, me)
    p1 = codec((3, 4, "vandermonde")).H  # p = 1: nothing is correctable
    stripe = np.array(host_stripe((3, 4, "vandermonde"), 8))
    stripe[0, 0] ^= 1
    rows, fixed, by_weight, unc, nbad = gf.correct_oracle(p1, stripe, 1)
    assert (unc, nbad) == (1, 1) and not fixed.any() and not by_weight.any() and np.array_equal(rows, stripe)


def test_check_matrices_have_the_dependent_sets_the_rule_guards_against():
    """No three columns of either (10, 14) H are dependent; the Vandermonde H has dependent 4-sets
    ((0, 1, 2, 12) is one), the Cauchy H none."""
    f = gf.GF256
    for code in (VAND, CAUCHY):
        h = codec(code).H
        assert all(any(f.is_invertible(h[list(r)][:, list(c)]) for r in itertools.combinations(range(4), 3))
                   for c in itertools.combinations(range(14), 3))
    hv = codec(VAND).H
    dependent = [c for c in itertools.combinations(range(14), 4) if not f.is_invertible(hv[:, list(c)])]
    assert len(dependent) == 12 and (0, 1, 2, 12) in dependent and dependent[0] == dependent_four_set(VAND)
    assert dependent_four_set(CAUCHY) is None


@pytest.mark.parametrize("code,ncols", SINGLE_RUNS, ids=map(run_id, SINGLE_RUNS))
def test_single_errors_in_every_chunk(code, ncols):
    case_singles("cpu", code, ncols)


@pytest.mark.parametrize("code,ncols", [(c, s) for c in CODES for s in (1, 65, 4097)],
                         ids=lambda v: code_id(v) if isinstance(v, tuple) else f"C{v}")
def test_clean_stripe(code, ncols):
    case_clean("cpu", code, ncols)


@pytest.mark.parametrize("mixed", [False, True], ids=["identity", "mixed"])
def test_every_pair_and_every_error_value(mixed):
    case_every_pair_every_value("cpu", mixed)


@pytest.mark.parametrize("code", [VAND, CAUCHY], ids=code_id)
def test_singles_doubles_and_triples(code):
    case_doubles("cpu", code)


@pytest.mark.parametrize("code", [(9, 14, "cauchy"), (3, 19, "cauchy"), WIDE], ids=code_id)
def test_double_errors_on_other_tiles(code):
    """p = 5, p = 16 and n = MAX_PAIR_N: a double error in the first and last chunk and in two
    neighbours, next to singles."""
    case_pairs_on("cpu", code)


def test_scattered_corruption_that_heal_refuses():
    case_scattered("cpu")


def test_planted_ambiguity_is_left_alone():
    case_planted_ambiguity("cpu")


def test_planted_miscorrection_equals_the_oracle():
    case_planted_miscorrection("cpu")


def test_untouched_bytes():
    case_untouched("cpu")


@pytest.mark.parametrize("ncols", [15, 4101])
@pytest.mark.parametrize("code", [VAND, CAUCHY], ids=code_id)
def test_unaligned_rows(code, ncols):
    case_unaligned("cpu", code, ncols)


def test_refusals():
    case_refusals("cpu")


def test_empty_stripe():
    case_empty("cpu")
