"""Where in memory the bytes are, for the repair kernels (GPU): correct, checked repair, the batched
repair and the variable-length kernel on four REAL rows of 2^32 + 16,011 bytes, and the batched scrub,
correct, checked-repair and variable-length calls on stripes 2^32 + 4096 bytes apart.

tests/test_gpu_addressing.py runs the GEMM engines and scrub on such rows; it must come first (its last
test bounds the peak memory of everything before it), which this module's name sees to. Here the
cold passes patch single bytes at columns around 2^31, around and above 2^32 and around a 2^32 multiple
of a row's absolute address (tests/addressing_repair_cases.py: ``hit_groups``), the hot passes store
rebuilt rows over the whole length, and the variable-length kernel runs a stripe of 2^20 + 4 column
blocks between two short ones. A column or block index cut to 32 bits lands inside the same rows, so
the failure to expect is a wrong byte, not a fault. Every expected report is the numpy oracle on the
65,536-byte blocks that hold a hit, summed; every test restores the stripe and ends with a zero
``syndrome_mask`` over all 65,537 words of the whole stripe, which test_scrub_rows_longer_than_4gib
makes a trustworthy verifier: a store at a wrapped offset leaves its target and its landing column
inconsistent. Codes: n = 4, Cauchy, RS(2,4) (p = 2, a 2-row tile) and RS(1,4) (p = 3, a 4-row tile with
one padding check row). Aligned rows take the vector forms; views one byte off alignment, L - 1 bytes
long, the byte forms.

Not covered: a weight-2 repair at a column above 2^32. It needs r >= 4, so five or six rows of 4.3 GiB,
and runs the same ``patch`` twice; the pair search itself runs on the short rows of
test_stripes_4gib_apart.

The four rows and the scratch of the checks need about 19 GiB of device memory; the module skips
below that. The CPU tests at the top need no GPU.
"""
import contextlib

import numpy as np
import pytest
import torch

import addressing_cases as ac
import addressing_repair_cases as arc
from addressing_repair_cases import BB, ERASED, FILL, L, P32
from gpu_rscode_amd import ReedSolomon, VarlenCodec, gf
from gpu_rscode_amd.gf import GF256
from gpu_rscode_amd.ops import varlen as ov
from gpu_rscode_amd.ops.varlen import VarlenPlan

gpu = pytest.mark.gpu
LENGTHS = [4101, L, 17]  # the variable-length batch: the long stripe between two short ones


def bits(i: int) -> int:
    """The nonzero error value of hit i."""
    return 37 * (i + 1) % 255 + 1


# ---- CPU: the hit columns, the block sum, the work list ------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
def test_hit_columns_hold_their_classes(shift):
    """The shared hit list: 2^31 - 1, 2^31 + 7, 2^32 - 1, 2^32 + 5, the first tail byte and the last
    byte, and around each given row's 2^32 address crossing; distinct columns inside the row, at least
    two above 2^32, and no 65,536-byte block holds columns of two groups (a group: one column; the two
    adjacent columns of a crossing; the columns from 2^32 on, which all lie in the last, ragged
    block)."""
    length = L - shift
    for base in (0x7F12_1000_0000, 0x7F12_9000_0000, 0x7F12_FFF0_0000):
        ptrs = [base + 4096 + shift, base + 3 * (P32 + (2 << 20)) + 4096 + shift]
        groups = arc.hit_groups(length, ptrs)
        cols = arc.hit_columns(length, ptrs)
        assert cols[:6] == [2 ** 31 - 1, 2 ** 31 + 7, 2 ** 32 - 1, 2 ** 32 + 5, length - 11, length - 1]
        assert len(set(cols)) == len(cols) and all(0 <= c < length for c in cols)
        assert sum(c > P32 for c in cols) >= 2
        if not shift:
            assert (length - 11) % 16 == 0 and length - 11 == length // 16 * 16  # the first tail byte
        taken = [set(arc.blocks_of(g)) for g in groups]
        for a in range(len(taken)):
            for b in range(a + 1, len(taken)):
                assert not taken[a] & taken[b], (groups[a], groups[b])
        for g in groups[:3]:
            assert len(g) == 1
        assert all(c >= P32 for c in groups[3]) and arc.blocks_of(groups[3]) == [arc.NMASK - 1]
        for p, g in zip(ptrs, groups[4:]):  # (none of these addresses loses its pair)
            assert len(g) == 2 and g[1] == g[0] + 1 and (p + g[1]) % P32 == 0 and (p + g[0]) >> 32 != (p + g[1]) >> 32
        assert len(groups) == 6
    # a row whose crossing falls into a block already hit keeps the six columns only
    assert arc.hit_columns(L, [P32 - (2 ** 31 + 100)]) == arc.hit_columns(L, [])
    assert arc.crossing(3 * P32, L) == P32  # (a row that starts on a multiple crosses the next one)


@pytest.mark.parametrize("code", sorted(arc.CODES))
def test_block_sums_equal_the_whole_stripe(code):
    """The way the GPU tests build an expected report, the oracle on the hit blocks summed, equals
    the project's whole-stripe CPU paths on short rows (two full blocks and a ragged one)."""
    bb, length = 4096, 2 * 4096 + 1011
    rs = arc.codec(code)
    rng = np.random.default_rng(7)
    good = rng.integers(0, 256, size=(rs.n, length), dtype=np.uint8)
    good[rs.k:] = GF256.gemm(rs.E, good[: rs.k])
    cols = [5, bb - 1, 2 * bb + 1000, length - 1]
    hits = [(i % rs.n, c, bits(i)) for i, c in enumerate(cols)] + [(1, 2 * bb + 77, 0x42), (2, 2 * bb + 77, 0x99)]
    blocks = sorted({c // bb for _, c, _ in hits})
    assert blocks == [0, 2]  # (block 1 stays clean)
    nmask = -(-length // bb)

    def stripe(host):
        return [torch.from_numpy(np.array(r)) for r in host]

    whole = np.array(good)
    for j, c, v in hits:
        whole[j, c] ^= v
    rows = stripe(whole)
    bad = arc.damaged(arc.fetch(stripe(good), blocks, bb), hits, bb)
    assert all(np.array_equal(bad[b], whole[:, b * bb: (b + 1) * bb]) for b in blocks)
    want = arc.expect_correct(rs.H, bad, 1, nmask, bb)
    arc.assert_report(rs.correct(rows, 1, bb), want, code)
    assert not arc.wrong_bytes(arc.fetch(rows, blocks, bb), want[0], bb)
    assert want[4] == len(cols) + 1 and int(want[1].sum()) + want[3] >= len(cols)
    # ... and the checked repair, one row erased
    x = [0]
    s = [j for j in range(rs.n) if j not in x]
    hits = [(s[i % len(s)], c, bits(i)) for i, c in enumerate(cols)]
    bad = arc.damaged(arc.fetch(stripe(good), blocks, bb), hits, bb)
    whole = np.array(good)
    for j, c, v in hits:
        whole[j, c] ^= v
    for d in list(bad.values()) + [whole]:
        d[x] = ERASED
    rows = stripe(whole)
    want = arc.expect_checked(rs.H, bad, x, None, nmask, bb)
    arc.assert_report(rs.reconstruct_checked(rows, x, block_bytes=bb), want, code)
    assert not arc.wrong_bytes(arc.fetch(rows, blocks, bb), want[0], bb)
    assert want[4] == len(cols)
    # a wrong byte is named with its row and column
    rows[1][2 * bb + 3] ^= 1
    assert arc.wrong_bytes(arc.fetch(rows, blocks, bb), want[0], bb) == [(1, 2 * bb + 3)]
    assert "row 1 column 4294967301 (0x100000005, above 2^32)" == arc.describe([(1, P32 + 5)])


@pytest.mark.parametrize("bytewise", [False, True], ids=["vector", "byte"])
def test_work_list_of_a_stripe_of_a_million_blocks(bytewise):
    """``varlen_blocks([4101, L, 17])`` against the closed form: nb, its exclusive prefix sum, the block
    map piecewise constant with those run lengths; the third stripe starts above block 2^20; and the
    lane rule replayed on the first and last two blocks of the long stripe covers exactly its first
    and last bytes, each once, the last block holding the tail lanes."""
    lengths = [c - (1 if bytewise else 0) for c in LENGTHS]
    nb, first, blk = ov.varlen_blocks(lengths, bytewise)
    want = arc.closed_form_blocks(lengths, bytewise)
    assert want.tolist() == ([17, 2 ** 24 + 63, 1] if bytewise else [2, 2 ** 20 + 4, 1])
    assert nb.dtype == np.int64 and np.array_equal(nb, want)
    assert first.dtype == np.int64 and first.tolist() == [0, int(want[0]), int(want[0] + want[1])]
    assert first[2] > 1 << 20
    assert blk.dtype == np.int32 and blk.size == int(want.sum())
    edges = np.nonzero(np.diff(blk))[0] + 1
    assert edges.tolist() == first[1:].tolist() and blk[0] == 0 and blk[-1] == 2
    assert blk[first[1]] == 1 and blk[first[2] - 1] == 1
    long = lengths[1]
    last = int(nb[1]) - 1
    for blocks, lo, hi in (((0, 1), 0, 512 * (1 if bytewise else 16)),
                           ((last - 1, last), (last - 1) * 256 * (1 if bytewise else 16), long)):
        spans = [s for cb in blocks for s in arc.lane_bytes(long, cb, bytewise)]
        covered = np.zeros(hi - lo, dtype=np.int64)
        for a, b in spans:
            assert lo <= a < b <= hi, (a, b)
            covered[a - lo: b - lo] += 1
        assert (covered == 1).all()
    if not bytewise:
        tail = arc.lane_bytes(long, last, False)
        assert len(tail) == 1000 % 256 + 11 and [b - a for a, b in tail[-11:]] == [1] * 11
        assert tail[-11][0] == long - 11 and tail[-1][1] == long


# ---- stripes 2^32 + 4096 bytes apart (before the four rows are made: it needs 4.3 GiB of its own) ----------
def _scrub_want(h, host, bb):
    return [gf.scrub_oracle(h, host[b], bb) for b in range(host.shape[0])]


@gpu
@pytest.mark.parametrize("form", ["vector", "byte"])
def test_stripes_4gib_apart(form):
    """B = 2 stripes of the Cauchy (4, 8) code, C = 4101, rows 8,192 bytes apart, the second stripe
    2^32 + 4096 bytes after the first in one 0x5A-filled buffer, as one strided [2, n, C] tensor and as
    a list of stripes: syndrome_mask_batch, scrub_batch, correct_batch (stripe 1 holds a weight-2
    column), reconstruct_checked_batch and VarlenCodec (encode, and a repair with a pattern per stripe),
    each stripe with damage or erasures of its own. Every per-stripe result equals the oracle's, and
    every byte of the buffer outside the rows is still 0x5A. The byte form: the same one byte off
    alignment."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of device memory, {free >> 20} MiB are free")
    k, n, c, gap, bb = 4, 8, 4101, 8192, 4096
    shift = 0 if form == "vector" else 1
    total = arc.APART + (1 << 20)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf.fill_(FILL)
    base = (-buf.data_ptr()) % 16 + shift
    assert base + arc.APART + (n - 1) * gap + c <= total
    tensor = buf.as_strided((2, n, c), (arc.APART, gap, 1), base)
    assert tensor[1, 0].data_ptr() - tensor[0, 0].data_ptr() == arc.APART and tensor.data_ptr() % 16 == shift
    rng = np.random.default_rng(48)
    good = rng.integers(0, 256, size=(2, n, c), dtype=np.uint8)
    h = ReedSolomon(k, n, matrix="cauchy").H
    e = h[:, :k]
    for b in range(2):
        good[b, k:] = GF256.gemm(e, good[b, :k])
    bad = np.array(good)
    bad[0, 2, 7] ^= 0x31          # stripe 0: two single errors, one in the ragged tail
    bad[0, 6, 4100] ^= 0x01
    bad[1, 0, 4096] ^= 0x80       # stripe 1: a weight-2 column and a single error
    bad[1, 3, 4096] ^= 0x11
    bad[1, 7, 15] ^= 0xFF

    def check(want, what):
        torch.cuda.synchronize()
        got = tensor.cpu().numpy()
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())
        tensor.fill_(FILL)
        at = ac.first_other(buf, FILL)
        assert at < 0, f"{what}: a byte outside the rows was written, the first at {at} ({at:#x})"

    for kind in ("tensor", "list"):
        rs = ReedSolomon(k, n, matrix="cauchy")  # (a fresh plan cache per argument form)
        arg = tensor if kind == "tensor" else [[tensor[b, j] for j in range(n)] for b in range(2)]
        # scrub
        tensor.copy_(torch.from_numpy(bad))
        want = _scrub_want(h, bad, bb)
        mask = rs.syndrome_mask_batch(arg, block_bytes=bb)
        assert np.array_equal(mask.cpu().numpy(), np.stack([w[0] for w in want])), kind
        rep = rs.scrub_batch(arg, block_bytes=bb)
        assert np.array_equal(rep.mask.cpu().numpy(), np.stack([w[0] for w in want])), kind
        for b in range(2):
            assert np.array_equal(rep.votes[b], want[b][1]), (kind, b)
            assert (int(rep.unlocated[b]), int(rep.bad_columns[b])) == want[b][2:], (kind, b)
        assert rep.dirty == [0, 1] and [w[3] for w in want] == [2, 2]
        check(bad, f"{kind}: scrub")
        # correct, the pair search in stripe 1
        tensor.copy_(torch.from_numpy(bad))
        rep = rs.correct_batch(arg, max_errors=2, block_bytes=bb)
        for b in range(2):
            rows, fixed, by_weight, unc, nbad = gf.correct_oracle(h, bad[b], 2)
            assert np.array_equal(rows, good[b]) and by_weight.tolist() == [[0, 2, 0], [0, 1, 1]][b] and unc == 0
            r = rep.report[b]
            assert (r.bad_columns, r.uncorrectable, r.fixed_bytes.tolist(), r.by_weight.tolist()) == \
                (nbad, unc, fixed.tolist(), by_weight.tolist()), (kind, b)
            assert np.array_equal(r.mask.cpu().numpy(), want[b][0]), (kind, b)
        check(good, f"{kind}: correct_batch")
        # checked repair: chunks 1 and 6 lost in both stripes, a wrong survivor in each (r = 2)
        x = [1, 6]
        s = [j for j in range(n) if j not in x]
        work = np.array(good)
        work[0, 2, 7] ^= 0x31
        work[1, 7, 4100] ^= 0x80
        work[:, x] = ERASED
        tensor.copy_(torch.from_numpy(work))
        rep = rs.reconstruct_checked_batch(arg, x, block_bytes=bb)
        for b in range(2):
            rows, fixed, by_weight, unc, nbad, t = gf.reconstruct_checked_oracle(h, work[b], x)
            assert np.array_equal(rows, good[b]) and by_weight.tolist() == [0, 1, 0] and (unc, nbad) == (0, 1)
            r = rep.report[b]
            assert (r.bad_columns, r.uncorrectable, r.fixed_bytes.tolist(), r.by_weight.tolist()) == \
                (nbad, unc, fixed.tolist(), by_weight.tolist()), (kind, b)
            assert np.array_equal(r.mask.cpu().numpy(), gf.scrub_oracle(t[2:][:, s], work[b][s], bb)[0]), (kind, b)
        check(good, f"{kind}: reconstruct_checked_batch")
        # the variable-length kernel: encode, then a repair with a pattern per stripe
        stripes = [tensor[b] for b in range(2)] if kind == "tensor" else arg
        work = np.array(good)
        work[:, k:] = ERASED
        tensor.copy_(torch.from_numpy(work))
        VarlenCodec(rs).encode([st[:k] for st in stripes], [st[k:] for st in stripes])
        check(good, f"{kind}: VarlenCodec.encode")
        erased = [[1, 4, 7], [0]]
        work = np.array(good)
        for b in range(2):
            work[b, erased[b]] = ERASED
            assert np.array_equal(gf.reconstruct_oracle(rs.G, work[b], erased[b]), good[b])
        tensor.copy_(torch.from_numpy(work))
        VarlenCodec(rs).reconstruct(stripes, erased)
        check(good, f"{kind}: VarlenCodec.reconstruct")
        forms = [p.bytewise for p in rs._plans.values() if hasattr(p, "bytewise")]
        assert len(forms) >= 5 and all(f == (shift != 0) for f in forms), (kind, forms)
    del buf, tensor, arg, stripes
    torch.cuda.empty_cache()


# ---- the four rows ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def holder():
    torch.cuda.reset_peak_memory_stats()  # (the 16 GiB bound of test_gpu_addressing.py was asserted there)
    h = arc.Rows()
    yield h
    h.release()


@pytest.fixture
def big(holder):
    why = holder.acquire()
    if why:
        pytest.skip(why)
    return holder


@contextlib.contextmanager
def restored(big, rs, rows, good, what):
    """The body hits the stripe; whatever becomes of it, the saved blocks ``good`` are written back and
    the whole stripe is checked: a zero mask over all 65,537 words and intact guards. A stripe found
    inconsistent is made anew for the tests that follow; the body's own failure comes first."""
    problem = None
    try:
        yield
    finally:
        arc.store(rows, good)
        try:
            big.assert_consistent(rs, what)
        except AssertionError as err:
            problem = str(err)
    assert problem is None, problem


def _rows(big, form):
    """The four rows as the form takes them, and whether that is the byte form."""
    rows = big.views(0 if form == "aligned" else 1)
    assert all(r.data_ptr() % 16 == (form != "aligned") for r in rows)
    return rows, form != "aligned", rows[0].numel()


def _ran(rs, kind, bytewise, length) -> bool:
    """A plan of class ``kind`` over rows of ``length`` bytes in that form is in the codec's cache."""
    return any(type(p).__name__ == kind and p.bytewise == bytewise and p.ncols == length for p in rs._plans.values())


def _assert_blocks(rows, blocks, want, what):
    at = arc.wrong_bytes(arc.fetch(rows, blocks), want)
    assert not at, f"{what}: wrong bytes at {arc.describe(at)}"


# ---- 1. correct -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", ["aligned", "byte"])
@pytest.mark.parametrize("call", ["correct", "correct_batch"])
@pytest.mark.parametrize("code", sorted(arc.CODES))
def test_correct_rows_longer_than_4gib(big, code, call, form):
    """One flipped byte per hit column, the chunks in turn, so natives and parity are both patched above
    2^32; one more column above 2^32 with two flips, beyond max_errors = 1: whatever the oracle makes
    of it (uncorrectable, or a miscorrection) the kernel makes too. Report and mask equal the
    oracle's on the hit blocks, the flipped bytes read back as the originals."""
    rs, _ = big.stripe(code)
    rows, bytewise, length = _rows(big, form)
    n = rs.n
    cols = arc.hit_columns(length, [rows[0].data_ptr(), rows[n - 1].data_ptr()])
    hits = [(i % n, c, bits(i)) for i, c in enumerate(cols)]
    high = {j for j, c, _ in hits if c > P32}
    assert high & set(range(rs.k)) and high & set(range(rs.k, n))
    double = [(1, arc.DOUBLE_COL, 0x42), (2, arc.DOUBLE_COL, 0x99)]
    assert arc.DOUBLE_COL not in cols and arc.DOUBLE_COL < length
    blocks = arc.blocks_of(cols + [arc.DOUBLE_COL])
    good = arc.fetch(rows, blocks)
    want = arc.expect_correct(rs.H, arc.damaged(good, hits + double), 1, -(-length // BB))
    for b in blocks:  # the oracle undoes every single flip; the double column is its own affair
        same = want[0][b] == good[b]
        if b == arc.DOUBLE_COL // BB:
            same[:, arc.DOUBLE_COL % BB] = True
        assert same.all()
    assert want[4] == len(cols) + 1 and want[2][1] + want[3] == want[4]
    what = f"{call} {code} {form}"
    with restored(big, rs, rows, good, what):
        for j, c, v in hits + double:
            arc.flip(rows[j], c, v)
        if call == "correct":
            rep = rs.correct(rows, 1, BB)
        else:
            rep = rs.correct_batch([rows], max_errors=1, block_bytes=BB).report[0]
        arc.assert_report(rep, want, what)
        _assert_blocks(rows, blocks, want[0], what)
        assert _ran(rs, "CorrectPlan" if call == "correct" else "BatchCorrectPlan", bytewise, length)


# ---- 2. checked repair ----------------------------------------------------------------------------------
CHECKED = [("rs14", (0,)), ("rs14", (3,)), ("rs14", (0, 2)), ("rs14", (0, 1, 2)), ("rs24", (1,)), ("rs24", (0, 3))]
CHECKED = [(c, x, "aligned") for c, x in CHECKED] + [(c, x, "byte") for c, x in CHECKED[:2]]  # byte: e = 1, r = 2


@gpu
@pytest.mark.parametrize("call", ["single", "batch"])
@pytest.mark.parametrize("code,erased,form", CHECKED, ids=[f"{c}-x{''.join(map(str, x))}-{f}" for c, x, f in CHECKED])
def test_reconstruct_checked_rows_longer_than_4gib(big, code, erased, form, call):
    """The erased rows prefilled with 0xA5 and rebuilt over the whole length; with r >= 1 one wrong
    survivor byte per hit column, the survivors in turn. RS(1,4): e = 1 (r = 2: the cold pass patches the
    survivor and the erased row at the column; a native lost, a parity row lost), e = 2 (r = 1: detection
    only), e = 3 (r = 0: three rows from one); RS(2,4): e = 1 (r = 1), e = 2 (r = 0). Every report field
    and the mask equal the oracle's on the hit blocks and so do the bytes: where it corrects, the
    originals; where it only detects, the survivors as damaged. The byte form runs for e = 1, r = 2."""
    rs, _ = big.stripe(code)
    x = list(erased)
    r = rs.p - len(x)
    rows, bytewise, length = _rows(big, form)
    s = [j for j in range(rs.n) if j not in x]
    cols = arc.hit_columns(length, [rows[s[0]].data_ptr(), rows[x[0]].data_ptr()])
    hits = [(s[i % len(s)], c, bits(i)) for i, c in enumerate(cols)] if r else []
    blocks = arc.blocks_of(cols)
    good = arc.fetch(rows, blocks)
    work = arc.damaged(good, hits)
    for d in work.values():
        d[x] = ERASED
    want = arc.expect_checked(rs.H, work, x, None, -(-length // BB))
    assert want[4] == len(hits)
    if r >= 2:  # everything is corrected: the originals
        assert want[3] == 0 and want[2][1] == len(hits) and all(np.array_equal(want[0][b], good[b]) for b in blocks)
    else:  # nothing is: the survivors as damaged
        assert want[3] == len(hits) and all(np.array_equal(want[0][b][s], work[b][s]) for b in blocks)
    what = f"reconstruct_checked {call} {code} erased {x} {form}"
    with restored(big, rs, rows, good, what):
        for j in x:
            rows[j].fill_(ERASED)
        for j, c, v in hits:
            arc.flip(rows[j], c, v)
        if call == "single":
            rep = rs.reconstruct_checked(rows, x, block_bytes=BB)
        else:
            rep = rs.reconstruct_checked_batch([rows], x, block_bytes=BB).report[0]
        arc.assert_report(rep, want, what)
        _assert_blocks(rows, blocks, want[0], what)
        assert _ran(rs, "CheckedRepairPlan" if call == "single" else "BatchCheckedRepairPlan", bytewise, length)
        if r >= 2 or not hits:  # the hot pass's stores over the whole length, before anything is put back
            big.assert_consistent(rs, what + ", before the restore")


# ---- 3. reconstruct -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", ["aligned", "byte"])
@pytest.mark.parametrize("call", ["reconstruct", "reconstruct_batch"])
def test_reconstruct_rows_longer_than_4gib(big, call, form):
    """RS(2,4), native 1 and parity row 2 erased and prefilled with 0xA5: the rebuilt rows equal the
    torch reference applied to the two survivors with the host coefficients G[erased] . inv(G[survivors])
    over the whole length, then the mask is zero and the guards are intact. ``reconstruct`` is one
    GemmPlan, ``reconstruct_batch`` (B = 1) gf_repair.hip, whose header promises rows longer than 2^32
    bytes."""
    rs, _ = big.stripe("rs24")
    rows, bytewise, length = _rows(big, form)
    x, s = [1, 2], [0, 3]
    coeff = GF256.matmul(rs.G[x], GF256.invert(rs.G[s])).astype(np.uint8)
    what = f"{call} {form}"
    with restored(big, rs, rows, {}, what):
        for j in x:
            rows[j].fill_(ERASED)
        if call == "reconstruct":
            rs.reconstruct(rows, x)
        else:
            rs.reconstruct_batch([rows], x)
            assert _ran(rs, "BatchRepairPlan", bytewise, length)
        torch.cuda.synchronize()
        bad, at = ac.whole_row_mismatches(8, coeff, [rows[j] for j in s], [rows[j] for j in x])
        assert bad == 0, f"{what}: {bad} wrong bytes, the first in the chunk at column {at} ({at:#x})"


# ---- 4. the variable-length kernel ------------------------------------------------------------------------
class Short:
    """A stripe of four short rows in a FILL-filled allocation of its own, a host image beside it."""

    def __init__(self, ncols: int, shift: int, seed: int, rs):
        self.pitch = (ncols + 255) // 256 * 256 + 256
        raw = torch.full((arc.GUARD + 4 * self.pitch + arc.GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
        self.buf = raw[(-raw.data_ptr()) % 16:]
        self.image = np.full(self.buf.numel(), FILL, dtype=np.uint8)
        self.starts = [arc.GUARD + j * self.pitch + shift for j in range(4)]
        self.rows = [self.buf[a: a + ncols] for a in self.starts]
        self.good = np.random.default_rng(seed).integers(0, 256, size=(4, ncols), dtype=np.uint8)
        self.good[rs.k:] = GF256.gemm(rs.E, self.good[: rs.k])

    def load(self, host) -> None:
        for j, a in enumerate(self.starts):
            self.image[a: a + host.shape[1]] = host[j]
        self.buf.copy_(torch.from_numpy(self.image))

    def check(self, want, what) -> None:
        for j, a in enumerate(self.starts):
            self.image[a: a + want.shape[1]] = want[j]
        got = self.buf.cpu().numpy()
        assert np.array_equal(got, self.image), (what, np.nonzero(got != self.image)[0][:4].tolist())


@gpu
@pytest.mark.parametrize("grid", [0, 1024], ids=["default-grid", "max_blocks-1024"])
@pytest.mark.parametrize("form", ["aligned", "byte"])
def test_varlen_stripe_of_a_million_blocks(big, form, grid):
    """Three RS(2,4) stripes in one launch, of 4,101, L and 17 bytes, the short ones in allocations of
    their own: the long stripe's work items are column blocks 0 .. 2^20 + 3, the last holds the tail
    lanes, and the third stripe's first block lies above 2^20. Encode (parity prefilled with 0xA5), then
    a repair with a pattern per stripe. The long stripe is compared on its hit blocks and by a zero mask
    over the whole length, the short ones with GF256.gemm and gf.reconstruct_oracle, their whole
    allocations included. At the default grid through VarlenCodec; with max_blocks = 1024, about 1,025
    laps over the work list, through the plan."""
    rs, _ = big.stripe("rs24")
    rows, bytewise, length = _rows(big, form)
    shift = int(bytewise)
    k, n = rs.k, rs.n
    lengths = [LENGTHS[0], length, LENGTHS[2]]
    shorts = {0: Short(lengths[0], shift, 1, rs), 2: Short(lengths[2], shift, 2, rs)}
    stripes = [shorts[0].rows, rows, shorts[2].rows]
    ptrs = np.array([[r.data_ptr() for r in st] for st in stripes], dtype=np.uint64)
    nb, first, _ = ov.varlen_blocks(lengths, bytewise)
    assert first[2] > 1 << 20 and int(nb.sum()) == int(arc.closed_form_blocks(lengths, bytewise).sum())
    cols = arc.hit_columns(length, [rows[0].data_ptr(), rows[n - 1].data_ptr()])
    blocks = arc.blocks_of(cols)
    good = arc.fetch(rows, blocks)
    what = f"varlen {form} max_blocks={grid}"

    def run(pat, patterns, codec_call):
        if not grid:
            codec_call()
            plan = [p for p in rs._plans.values() if isinstance(p, VarlenPlan)][-1]
        else:
            plan = VarlenPlan(ptrs, lengths, pat, patterns, "cuda")
            plan.run(max_blocks=grid)
        assert plan.bytewise == bytewise and plan.nblk == int(nb.sum()) and plan.batch == 3
        torch.cuda.synchronize()

    with restored(big, rs, rows, good, what):
        # encode
        for b, sh in shorts.items():
            host = np.array(sh.good)
            host[k:] = ERASED
            sh.load(host)
        for j in range(k, n):
            rows[j].fill_(ERASED)
        run(np.zeros(3, dtype=np.int64), [(tuple(range(k)), tuple(range(k, n)), rs.E)],
            lambda: VarlenCodec(rs).encode([st[:k] for st in stripes], [st[k:] for st in stripes]))
        for b, sh in shorts.items():
            sh.check(sh.good, f"{what}: encode, stripe {b}")
        _assert_blocks(rows, blocks, good, what + ": encode, the long stripe")
        big.assert_consistent(rs, what + ": encode, the long stripe")
        # repair, a pattern per stripe
        erased = [[0], [1, 2], [3]]
        for b, sh in shorts.items():
            host = np.array(sh.good)
            host[erased[b]] = ERASED
            assert np.array_equal(gf.reconstruct_oracle(rs.G, host, erased[b]), sh.good)
            sh.load(host)
        for j in erased[1]:
            rows[j].fill_(ERASED)
        pat, patterns = rs._erased_patterns(rs._erased_raw(erased, n), 3)
        full = [(sv, er, rs.gf.matmul(rs.G[list(er)], rs.decode_matrix(sv)).astype(np.uint8)) for sv, er in patterns]
        run(pat, full, lambda: VarlenCodec(rs).reconstruct(stripes, erased))
        for b, sh in shorts.items():
            sh.check(sh.good, f"{what}: repair, stripe {b}")
        _assert_blocks(rows, blocks, good, what + ": repair, the long stripe")
        big.assert_consistent(rs, what + ": repair, the long stripe")


@gpu
def test_zz_peak_device_memory_of_the_module(holder):
    """Last in the module: the four rows, the scratch of the checks and the short stripes stayed within
    what the module asks to be free."""
    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory of the module: {peak} bytes ({peak / 2**30:.2f} GiB)")
    assert peak <= arc.NEED
