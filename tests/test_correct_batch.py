"""Batched correct on CPU tensors: ``correct_batch`` against the numpy oracle (``gf.correct_oracle``)
applied stripe by stripe, exactly, and against ``correct`` on each stripe alone. The case functions
take the device, so tests/test_gpu_correct_batch.py runs the same cases through the batched gfx950
kernel."""
import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, flat_rows, gf
from gpu_rscode_amd.ops.correct import BatchCorrectReport
from test_correct import CAUCHY, TOO_WIDE, VAND, WIDE, assert_report, default_max_errors
from test_scrub import GARBAGE, code_id, codec, stripe_bytes, unaligned_rows
from test_scrub_batch import batch_to_device, host_batch

BB = 4096
# (B, C): every B of {1, 2, 3, 257}; a short row, one span with a tail, two mask words
RUNS = [(1, 1), (2, 15), (3, 4101), (257, 17), (3, 8192 + 3), (257, 4101)]
CODES = [VAND, CAUCHY, (4, 6, "cauchy"), (9, 14, "cauchy"), (3, 19, "cauchy")]
MIXED_RUNS = [(c, b, s) for c in CODES for b, s in RUNS if c[1] <= 14 or (b, s) != (257, 4101)]


def run_id(r):
    return f"{code_id(r[0])}-B{r[1]}-C{r[2]}"


def damaged_batch(code, nstripes: int, ncols: int):
    """(good, bad): stripe b is clean (b % 4 == 0), has single errors in two chunks (1), a double error
    and a single (2), or a triple error next to a single (3); a batch of one holds a double. Chunks,
    columns and values depend on b."""
    rs = codec(code)
    good = host_batch(code, nstripes, ncols)
    bad = np.array(good)
    rng = np.random.default_rng(nstripes * 1000 + ncols)
    for b in range(nstripes):
        kind = 2 if nstripes == 1 else b % 4
        cols = rng.permutation(ncols)[:2].tolist() if ncols > 1 else [0]
        js = rng.permutation(rs.n)[:4].tolist()
        if kind == 1:
            for j, c in zip(js, cols):
                bad[b, j, c] ^= rng.integers(1, 256)
        elif kind >= 2:
            for j in js[: kind]:
                bad[b, j, cols[0]] ^= rng.integers(1, 256)
            if len(cols) > 1:
                bad[b, js[3], cols[1]] ^= rng.integers(1, 256)
    return good, bad


def oracle_batch(code, bad: np.ndarray, max_errors: int, block_bytes: int):
    """gf.correct_oracle stripe by stripe (clean stripes, found by one syndrome of the whole batch,
    are not handed to it): (rows [B, n, C], fixed [B, n], by_weight [B, 3], unc [B], bad [B], mask)."""
    h = codec(code).H
    nstripes, n, ncols = bad.shape
    nmask = -(-ncols // block_bytes)
    rows, fixed, by_weight = np.array(bad), np.zeros((nstripes, n), np.int64), np.zeros((nstripes, 3), np.int64)
    unc, nbad, mask = np.zeros(nstripes, np.int64), np.zeros(nstripes, np.int64), np.zeros((nstripes, nmask), np.int32)
    syn = gf.GF256.gemm(h, bad.transpose(1, 0, 2).reshape(n, nstripes * ncols)).reshape(-1, nstripes, ncols)
    for b in np.nonzero(syn.any(axis=(0, 2)))[0]:
        rows[b], fixed[b], by_weight[b], unc[b], nbad[b] = gf.correct_oracle(h, bad[b], max_errors)
        mask[b] = gf.scrub_oracle(h, bad[b], block_bytes)[0]
    return rows, fixed, by_weight, unc, nbad, mask


def assert_batch_corrected(code, stripes, bad, good, parity=None, max_errors=None, block_bytes=BB, rows_of=None):
    """``correct_batch`` on ``stripes`` (holding ``bad``): every field and every row against the
    oracle's; stripes with nothing uncorrectable are clean afterwards, and restored unless a column
    held more errors than ``max_errors`` (which may be miscorrected: inherent to the code)."""
    rs = codec(code)
    me = default_max_errors(rs.p) if max_errors is None else max_errors
    rows, fixed, by_weight, unc, nbad, mask = oracle_batch(code, bad, me, block_bytes)
    rep = rs.correct_batch(stripes, parity, max_errors, block_bytes)
    assert isinstance(rep, BatchCorrectReport)
    assert rep.mask.dtype == torch.int32 and np.array_equal(rep.mask.cpu().numpy(), mask)
    assert rep.fixed_bytes.dtype == np.int64 and np.array_equal(rep.fixed_bytes, fixed)
    assert rep.by_weight.dtype == np.int64 and np.array_equal(rep.by_weight, by_weight)
    assert rep.uncorrectable.dtype == np.int64 and np.array_equal(rep.uncorrectable, unc)
    assert rep.bad_columns.dtype == np.int64 and np.array_equal(rep.bad_columns, nbad)
    assert rep.clean.dtype == np.bool_ and np.array_equal(rep.clean, nbad == 0)
    assert rep.dirty == [int(b) for b in np.nonzero(nbad)[0]] and len(rep.report) == bad.shape[0]
    after = rows_of() if rows_of else (stripes if parity is None else torch.cat([stripes, parity], dim=1)).cpu().numpy()
    assert np.array_equal(after, rows)
    ok = unc == 0
    within = ((bad != good).sum(axis=1).max(axis=1) <= me) if bad.shape[2] else np.ones(len(ok), dtype=bool)
    assert np.array_equal(after[ok & within], good[ok & within])
    after_mask = rs.syndrome_mask_batch(stripes, parity, block_bytes).cpu().numpy()
    assert not after_mask[ok].any() and (unc == 0).tolist() == (~after_mask.any(axis=1)).tolist()
    return rep


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_mixed(device, code, nstripes, ncols):
    """Clean, single, double and uncorrectable stripes in one batch; ``report[b]`` equals ``correct`` on
    a copy of stripe b alone, for the first, the last and a few dirty stripes."""
    rs = codec(code)
    good, bad = damaged_batch(code, nstripes, ncols)
    stripes = batch_to_device(bad, device)
    pad_before = flat_rows(stripes.view(-1, ncols)).cpu().numpy().copy()
    rep = assert_batch_corrected(code, stripes, bad, good)
    flat = flat_rows(stripes.view(-1, ncols)).cpu().numpy()
    pitch = stripes.stride(1)
    pad = (np.arange(flat.size) % pitch) >= ncols
    assert (flat[pad] == GARBAGE).all() and np.array_equal(flat[pad], pad_before[pad])
    if nstripes >= 3 and rs.p >= 4:
        assert rep.by_weight[:, 1].any() and rep.by_weight[:, 2].any() and not rep.clean.all() and rep.clean.any()
    for b in sorted({0, nstripes - 1, *rep.dirty[:6]}):
        alone = batch_to_device(bad[b: b + 1], device)[0]
        one = rs.correct(alone, block_bytes=BB)
        assert_report(one, rs.H, bad[b], default_max_errors(rs.p), BB)
        got = rep.report[b]
        assert (got.clean, got.bad_columns, got.uncorrectable) == (one.clean, one.bad_columns, one.uncorrectable)
        assert np.array_equal(got.fixed_bytes, one.fixed_bytes) and np.array_equal(got.by_weight, one.by_weight)
        assert np.array_equal(got.mask.cpu().numpy(), one.mask.cpu().numpy())
        assert np.array_equal(stripe_bytes(alone), stripes[b].cpu().numpy())


def case_other_stripes_untouched(device, code=VAND, ncols=4101):
    """Every second stripe of a larger tensor is the batch; the stripes in between are dirty and must
    stay bit for bit as they are."""
    good, bad = damaged_batch(code, 4, ncols)
    wide = np.array(host_batch(code, 8, ncols))
    wide[::2] = bad
    wide[1::2, 0, 7] ^= 0xFF
    whole = batch_to_device(wide, device)
    every_second = whole[::2]
    assert every_second.stride(0) == 2 * whole.stride(0)
    assert_batch_corrected(code, every_second, bad, good)
    assert np.array_equal(whole[1::2].cpu().numpy(), wide[1::2])


def case_input_forms(device, code, ncols=4101):
    """One batch as a [B, n, C] tensor, as row lists with the stripes in reverse, as a sequence of
    [n, C] tensors, and as natives and parity in two allocations: one result."""
    rs = codec(code)
    nstripes = 3
    good, bad = damaged_batch(code, nstripes, ncols)
    whole = batch_to_device(bad, device)
    ref = assert_batch_corrected(code, whole, bad, good)

    def same(rep, order=(0, 1, 2)):
        order = list(order)
        assert np.array_equal(rep.fixed_bytes, ref.fixed_bytes[order]) and np.array_equal(rep.by_weight, ref.by_weight[order])
        assert np.array_equal(rep.uncorrectable, ref.uncorrectable[order])
        assert np.array_equal(rep.mask.cpu().numpy(), ref.mask.cpu().numpy()[order])

    whole.copy_(torch.from_numpy(bad))
    lists = [[whole[b, j] for j in range(rs.n)] for b in reversed(range(nstripes))]
    same(assert_batch_corrected(code, lists, bad[::-1], good[::-1], rows_of=lambda: whole.cpu().numpy()[::-1]), (2, 1, 0))
    whole.copy_(torch.from_numpy(bad))
    per_stripe = [whole[b] for b in range(nstripes)]
    same(assert_batch_corrected(code, per_stripe, bad, good, rows_of=lambda: whole.cpu().numpy()))
    data = batch_to_device(bad[:, : rs.k], device)
    parity = batch_to_device(bad[:, rs.k:], device)
    assert parity.data_ptr() != data.data_ptr()
    same(assert_batch_corrected(code, data, bad, good, parity=parity))


def case_unaligned(device, code, ncols):
    """One row of one stripe starts at an odd address (the whole batch takes the byte form)."""
    rs = codec(code)
    good, bad = damaged_batch(code, 3, ncols)
    aligned = batch_to_device(bad, device)
    lists = [[aligned[b, j] for j in range(rs.n)] for b in range(3)]
    lists[1] = unaligned_rows(bad[1], device)
    assert sum(r.data_ptr() % 16 != 0 for rows in lists for r in rows) == 1
    rep = assert_batch_corrected(code, lists, bad, good,
                                 rows_of=lambda: np.stack([stripe_bytes(rows) for rows in lists]))
    aligned2 = batch_to_device(bad, device)
    ref = rs.correct_batch(aligned2, block_bytes=BB)
    assert np.array_equal(rep.fixed_bytes, ref.fixed_bytes) and np.array_equal(rep.by_weight, ref.by_weight)
    assert np.array_equal(rep.mask.cpu().numpy(), ref.mask.cpu().numpy())


def case_slice_boundary(device, code=(4, 8, "cauchy"), nstripes=65537, ncols=16):
    """More stripes than one launch's grid.y holds (65535): damage in the last two stripes of the first
    slice, the first of the second and stripe 0; everything else clean and unchanged. The CPU form,
    which has no slices and takes a stripe at a time, runs it with fewer stripes."""
    edge = nstripes - 2
    good = host_batch(code, nstripes, ncols)
    bad = np.array(good)
    bad[edge - 1, 1, 3] ^= 0x5A
    bad[edge, 5, 0] ^= 0x01
    bad[edge, 6, 0] ^= 0xFF
    bad[edge + 1, 2, 15] ^= 0x80
    bad[0, 7, 8] ^= 0x33
    stripes = torch.from_numpy(bad).to(device)
    rep = assert_batch_corrected(code, stripes, bad, good)
    assert rep.dirty == [0, edge - 1, edge, edge + 1] and not rep.uncorrectable.any()
    assert rep.by_weight[rep.dirty].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0]]
    assert np.array_equal(stripes.cpu().numpy(), good)


def case_wide(device):
    """n = MAX_PAIR_N in a batch; n = MAX_PAIR_N + 1 is refused with max_errors=2 and right with 1."""
    good, bad = damaged_batch(WIDE, 3, 65)
    rep = assert_batch_corrected(WIDE, batch_to_device(bad, device), bad, good)
    assert rep.by_weight[2].tolist() == [0, 1, 1]
    good, bad = damaged_batch(TOO_WIDE, 3, 65)
    stripes = batch_to_device(bad, device)
    for me in (None, 2):
        with pytest.raises(NotImplementedError):
            codec(TOO_WIDE).correct_batch(stripes, max_errors=me)
    assert np.array_equal(stripes.cpu().numpy(), bad)
    rep = assert_batch_corrected(TOO_WIDE, stripes, bad, good, max_errors=1)
    assert rep.by_weight.tolist() == [[0, 0, 0], [0, 2, 0], [0, 1, 0]] and rep.uncorrectable.tolist() == [0, 0, 1]


def case_refusals(device):
    """What correct_batch refuses, with the buffers unchanged after each refusal."""
    for field in ("gf16", "gf65536"):
        rs = ReedSolomon(4, 8, matrix="cauchy", field=field)
        stripes = torch.full((2, 8, 64), 7, dtype=torch.uint8, device=device)
        with pytest.raises(NotImplementedError, match=field):
            rs.correct_batch(stripes)
        assert (stripes == 7).all()
    rs = codec(VAND)
    good, bad = damaged_batch(VAND, 3, 4101)
    stripes = batch_to_device(bad, device)
    lists = [[stripes[b, j] for j in range(rs.n)] for b in range(3)]
    for me in (0, 3):
        with pytest.raises(ValueError):
            rs.correct_batch(stripes, max_errors=me)
    for bb in (0, 2048, 4097, 3 * 4096):
        with pytest.raises(ValueError):
            rs.correct_batch(stripes, block_bytes=bb)
    twice = [lists[0], lists[1], lists[0]]  # a stripe listed twice
    shared = [list(rows) for rows in lists]
    shared[2][4] = lists[0][9]  # one row in two stripes
    buf = torch.full((4101 + 50,), 3, dtype=torch.uint8, device=device)
    partly = [list(rows) for rows in lists]
    partly[0][0], partly[1][13] = buf[:4101], buf[50:]  # rows of two stripes that share bytes
    short = [list(rows) for rows in lists]
    short[2][5] = short[2][5][:4100]
    for arg in (twice, shared, partly, short, stripes[:, :13], stripes[0]):
        with pytest.raises(ValueError):
            rs.correct_batch(arg)
    for d, p in ((stripes[:, : rs.k], stripes[:, rs.k:][:2]), (stripes, stripes[:, rs.k:]),
                 (stripes[:, : rs.k], stripes[:, rs.k - 1: rs.n - 1])):  # (the last: parity overlapping the natives)
        with pytest.raises(ValueError):
            rs.correct_batch(d, p)
    for code, exc, kw in (((4, 6, "cauchy"), ValueError, dict(max_errors=2)), ((3, 4, "vandermonde"), ValueError, {}),
                          ((19, 36, "cauchy"), NotImplementedError, {})):
        host = host_batch(code, 2, 17)
        small = batch_to_device(host, device)
        with pytest.raises(exc):
            codec(code).correct_batch(small, **kw)
        assert np.array_equal(small.cpu().numpy(), host)
    assert np.array_equal(stripes.cpu().numpy(), bad) and (buf == 3).all()
    assert rs.correct_batch(stripes).dirty == [1, 2]


def case_trivial(device):
    """B = 0 and rows of no bytes: empty and zero results."""
    rs = codec(VAND)
    for empty in (torch.zeros((0, 14, 4101), dtype=torch.uint8, device=device), []):
        rep = rs.correct_batch(empty, block_bytes=BB)
        assert rep.clean.shape == (0,) and rep.fixed_bytes.shape == (0, 14) and rep.by_weight.shape == (0, 3)
        assert rep.dirty == [] and len(rep.report) == 0 and rep.mask.numel() == 0
    rep = rs.correct_batch(torch.zeros((3, 14, 0), dtype=torch.uint8, device=device))
    assert rep.clean.tolist() == [True] * 3 and tuple(rep.mask.shape) == (3, 0) and not rep.fixed_bytes.any()


# ---- the CPU tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,nstripes,ncols", MIXED_RUNS, ids=map(run_id, MIXED_RUNS))
def test_mixed_batch(code, nstripes, ncols):
    case_mixed("cpu", code, nstripes, ncols)


def test_other_stripes_are_untouched():
    case_other_stripes_untouched("cpu")


@pytest.mark.parametrize("code", [VAND, (9, 14, "cauchy")], ids=code_id)
def test_input_forms(code):
    case_input_forms("cpu", code)


@pytest.mark.parametrize("ncols", [15, 4101])
@pytest.mark.parametrize("code", [VAND, (9, 14, "cauchy")], ids=code_id)
def test_unaligned_rows(code, ncols):
    case_unaligned("cpu", code, ncols)


def test_many_tiny_stripes():
    case_slice_boundary("cpu", nstripes=2051)


def test_widest_pair_search_and_one_past_it():
    case_wide("cpu")


def test_refusals():
    case_refusals("cpu")


def test_trivial_batches():
    case_trivial("cpu")
