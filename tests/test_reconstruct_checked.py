"""Checked repair (ReedSolomon.reconstruct_checked / reconstruct_checked_batch) on CPU tensors: every
result, rows, report fields and mask, compared exactly with the numpy oracle
(``gf.reconstruct_checked_oracle``), and with the clean stripe wherever the code's distance promises
it. The cases take a device; tests/test_gpu_reconstruct_checked.py runs them through the kernels."""
import itertools
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, alloc_rows, flat_rows, gf
from gpu_rscode_amd.models.rs import UnrecoverableError
from gpu_rscode_amd.ops.correct import BatchCorrectReport, CorrectReport
from test_correct import dependent_four_set, null_vector
from test_scrub import GARBAGE, code_id, codec, host_stripe, stripe_bytes, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAND, CAUCHY = (10, 14, "vandermonde"), (10, 14, "cauchy")
MDS = [CAUCHY, (4, 8, "cauchy"), (9, 14, "cauchy"), (3, 19, "cauchy")]
LENGTHS = [1, 3, 4, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537, 65538, 65539]
FILLS = (0x00, 0xFF, None)  # what the erased rows hold when the call comes: zeros, ones, random bytes


# ---- the oracle's side ------------------------------------------------------------------------------
def default_max_errors(r: int) -> int:
    return max(1, min(2, r // 2))


def oracle(h, work: np.ndarray, erased, max_errors, block_bytes: int):
    """(rows, fixed_bytes, by_weight, uncorrectable, bad_columns, mask) of the oracle; the mask from
    its T: bit i where check row i, T[e + i, S] . work[S], is nonzero in the block."""
    rows, fixed, by_weight, unc, bad, t = gf.reconstruct_checked_oracle(h, work, erased, max_errors)
    x = sorted(set(int(e) for e in erased))
    s = [i for i in range(h.shape[1]) if i not in x]
    nmask = -(-work.shape[1] // block_bytes)
    mask = np.zeros(nmask, dtype=np.int32)
    if len(x) < h.shape[0] and work.shape[1]:
        mask = gf.scrub_oracle(t[len(x):][:, s], work[s], block_bytes)[0]
    return rows, fixed, by_weight, unc, bad, mask


def spoil(work: np.ndarray, erased, fill, seed=7) -> np.ndarray:
    """``work`` with its erased rows overwritten: they are outputs, never inputs."""
    out = np.array(work)
    for j in erased:
        out[j] = np.random.default_rng(seed + j).integers(0, 256, out.shape[1], dtype=np.uint8) if fill is None else fill
    return out


def assert_report(rep, want, stripe_now: np.ndarray):
    rows, fixed, by_weight, unc, bad, mask = want
    assert isinstance(rep, CorrectReport)
    assert np.array_equal(stripe_now, rows)
    assert rep.fixed_bytes.dtype == np.int64 and np.array_equal(rep.fixed_bytes, fixed)
    assert rep.by_weight.dtype == np.int64 and np.array_equal(rep.by_weight, by_weight)
    assert (rep.uncorrectable, rep.bad_columns, rep.clean) == (unc, bad, bad == 0)
    assert rep.mask.dtype == torch.int32 and np.array_equal(rep.mask.cpu().numpy(), mask)


def check(device, code, bad: np.ndarray, erased, max_errors=None, block_bytes=4096, good=None, fill=0xA5, stripe=None):
    """One call on ``bad`` with its erased rows spoiled, compared with the oracle on the same bytes;
    with ``good`` the result must also be the clean stripe with nothing uncorrectable."""
    rs = codec(code)
    work = spoil(bad, erased, fill)
    if stripe is None:
        stripe = to_device(work, device)
    else:
        for r, src in zip(stripe, work):
            r.copy_(torch.from_numpy(src))
    rep = rs.reconstruct_checked(stripe, erased, max_errors, block_bytes)
    r = rs.p - len(set(erased))
    want = oracle(rs.H, work, erased, default_max_errors(r) if max_errors is None else max_errors, block_bytes)
    now = stripe_bytes(stripe)
    assert_report(rep, want, now)
    if good is not None:
        assert np.array_equal(now, good) and rep.uncorrectable == 0
    if isinstance(stripe, torch.Tensor) and stripe.dim() == 2:  # alloc_rows storage: the pitch padding keeps its fill
        flat = flat_rows(stripe).cpu().numpy()
        pad = np.ones(flat.size, dtype=bool)
        for j in range(stripe.shape[0]):
            pad[j * stripe.stride(0): j * stripe.stride(0) + stripe.shape[1]] = False
        assert (flat[pad] == GARBAGE).all()
    return rep


def patterns(k: int, n: int, e: int):
    """Erasure patterns of e ids: natives only, parity only and mixed, as far as e allows."""
    p = n - k
    if e == 0:
        return [[]]
    out = []
    if e <= k:
        out.append(list(range(k - e, k)))  # natives only
    if e <= p:
        out.append(list(range(n - e, n)))  # parity only
    a = min(k, e // 2)
    if a >= 1 and e - a <= p:
        out.append(list(range(0, k, max(1, k // a)))[:a] + list(range(k, k + e - a)))  # mixed
    assert all(len(set(x)) == e for x in out)
    return out


def plant(bad: np.ndarray, survivors, col: int, count: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    for j in rng.choice(len(survivors), size=count, replace=False):
        bad[survivors[int(j)], col] ^= int(rng.integers(1, 256))


# ---- cases (device-generic) -------------------------------------------------------------------------
def case_ground_truth(device, code, ncols=333):
    """Every e, every kind of pattern: at most r // 2 (and at most max_errors) wrong survivors per
    column are corrected, the result is the clean stripe."""
    k, n, _ = code
    good = host_stripe(code, ncols)
    for e in range(n - k + 1):
        r = n - k - e
        for x in patterns(k, n, e):
            s = [i for i in range(n) if i not in x]
            bad = np.array(good)
            if r >= 2:
                for t, col in enumerate(range(0, ncols, 37)):
                    plant(bad, s, col, 1, 100 * e + t)
            if r >= 4:
                for t, col in enumerate(range(5, ncols, 41)):
                    plant(bad, s, col, 2, 900 * e + t)
            rep = check(device, code, bad, x, None, 4096, good)
            if r >= 2:
                assert rep.by_weight[1] == len(range(0, ncols, 37)) and rep.bad_columns == rep.by_weight.sum()
            if r >= 4:
                assert rep.by_weight[2] == len(range(5, ncols, 41))


def case_pair_search_at_63_survivors(device):
    code = (59, 64, "cauchy")
    good = host_stripe(code, 70)
    bad = np.array(good)
    s = [i for i in range(64) if i != 7]
    for t, col in enumerate((0, 13, 69)):
        plant(bad, s, col, 2, t)
    bad[62, 33] ^= 0x80
    bad[63, 34] ^= 0x01
    rep = check(device, code, bad, [7], 2, 4096, good)
    assert rep.by_weight.tolist() == [0, 2, 3]
    wide = (60, 65, "cauchy")
    stripe = to_device(host_stripe(wide, 70), device)
    with pytest.raises(NotImplementedError):
        codec(wide).reconstruct_checked(stripe, [], 2)
    assert np.array_equal(stripe_bytes(stripe), host_stripe(wide, 70))


def edge_columns(ncols: int) -> list[int]:
    """First and last column of the row, of each 4096-byte block and of each 16 KiB span."""
    cols = {0, ncols - 1}
    for step in (4096, 16384):
        for b in range(0, ncols, step):
            cols |= {b, min(b + step, ncols) - 1}
    return sorted(cols)


def case_lengths(device, ncols, code=CAUCHY, erased=(3,)):
    """A single error at every edge column in every survivor, K and R members alike: one call per
    rotation of the survivors over the edges. The oracle runs on the edge columns (it works column
    by column); every other column must be the clean stripe's."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    x = list(erased)
    s = [i for i in range(rs.n) if i not in x]
    cols = edge_columns(ncols)
    bb = 4096
    for rot in range(len(s)):
        bad = np.array(good)
        for t, c in enumerate(cols):
            bad[s[(t + rot) % len(s)], c] ^= 1 + (37 * t + rot) % 255
        work = spoil(bad, x, None, rot)
        stripe = to_device(work, device)
        rep = rs.reconstruct_checked(stripe, x, block_bytes=bb)
        rows, fixed, by_weight, unc, nbad, t_mat = gf.reconstruct_checked_oracle(rs.H, work[:, cols], x)
        want = np.array(good)
        want[:, cols] = rows
        now = stripe_bytes(stripe)
        assert np.array_equal(now, want) and np.array_equal(now, good)
        assert np.array_equal(rep.fixed_bytes, fixed) and np.array_equal(rep.by_weight, by_weight)
        assert (rep.uncorrectable, rep.bad_columns) == (unc, nbad) == (0, len(cols))
        u = gf.GF256.gemm(t_mat[len(x):][:, s], work[s][:, cols])
        mask = np.zeros(-(-ncols // bb), dtype=np.uint32)
        for i in range(u.shape[0]):
            mask[np.unique(np.array(cols)[u[i] != 0] // bb)] |= np.uint32(1 << i)
        assert np.array_equal(rep.mask.cpu().numpy(), mask.view(np.int32))


def case_every_error_value(device, code=CAUCHY, ncols=4097):
    """Every error value 1..255 at one position (one stripe of a batch per value), and across 255
    columns of one stripe."""
    rs = codec(code)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    bad[12, 3840: 4095] ^= np.arange(1, 256, dtype=np.uint8)
    check(device, code, bad, [0, 5], None, 4096, good)
    small = host_stripe(code, 17)
    hosts = np.repeat(small[None], 255, axis=0).copy()
    hosts[:, 6, 16] ^= np.arange(1, 256, dtype=np.uint8)
    hosts[:, 11] = 0xEE
    batch = torch.from_numpy(hosts).to(device)
    rep = rs.reconstruct_checked_batch(batch, [11])
    assert np.array_equal(batch.cpu().numpy(), np.repeat(small[None], 255, axis=0))
    assert (rep.by_weight == [0, 1, 0]).all() and (rep.fixed_bytes[:, 6] == 1).all() and rep.fixed_bytes.sum() == 255


def case_detection_only(device):
    """(4, 6): e = 1 leaves one check row, which detects and corrects nothing; e = 2 leaves none."""
    code = (4, 6, "cauchy")
    rs = codec(code)
    good = host_stripe(code, 4101)
    bad = np.array(good)
    bad[0, 0] ^= 1
    bad[2, 4096] ^= 0x55
    bad[5, 4100] ^= 0xFF
    rep = check(device, code, bad, [1])
    assert (rep.bad_columns, rep.uncorrectable, rep.fixed_bytes.sum()) == (3, 3, 0)
    rep = check(device, code, bad, [4])  # survivor 5 is the check row itself
    assert (rep.bad_columns, rep.uncorrectable) == (3, 3) and rep.mask.tolist() == [1, 1]
    rep = check(device, code, bad, [1, 4])
    assert rep.clean and rep.mask.tolist() == [0, 0]
    for x in ([1], [4], [1, 4], [3, 5]):
        work = spoil(bad, x, 0x00)
        stripe = to_device(work, device)
        rs.reconstruct_checked(stripe, x)
        now = stripe_bytes(stripe)
        assert np.array_equal(now[x], gf.reconstruct_oracle(rs.G, work, x)[x])
        s = [i for i in range(6) if i not in x]
        assert np.array_equal(now[s], work[s])  # the survivors untouched


def case_too_many_errors(device):
    """r = 2 and two wrong survivors in a column: beyond the code. Whatever the oracle does."""
    good = host_stripe(CAUCHY, 4101)
    bad = np.array(good)
    for t, col in enumerate(range(3, 4101, 97)):
        plant(bad, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13], col, 2, t)
    bad[4, 0] ^= 9  # and one it can correct
    rep = check(device, CAUCHY, bad, [2, 12])
    assert rep.bad_columns == 1 + len(range(3, 4101, 97)) and rep.by_weight[1] >= 1


@lru_cache(maxsize=None)
def singular_pattern(code):
    """The first erasure pattern of natives whose first k survivors do not determine the data."""
    rs = codec(code)
    for e in range(1, rs.p + 1):
        for x in itertools.combinations(range(rs.n), e):
            if not rs.is_recoverable([i for i in range(rs.n) if i not in x][: rs.k]):
                return list(x)
    return None


def case_reference_vandermonde(device):
    """The reference Vandermonde code is not MDS: a singular pattern is refused with the buffers
    unchanged, and a column with two explanations is left uncorrectable. The oracle is the contract."""
    rs = codec(VAND)
    x = singular_pattern(VAND)
    assert x is not None and singular_pattern(CAUCHY) is None
    good = host_stripe(VAND, 333)
    stripe = to_device(good, device)
    with pytest.raises(UnrecoverableError):
        rs.reconstruct_checked(stripe, x)
    with pytest.raises(UnrecoverableError):
        rs.reconstruct_checked_batch([stripe], x)
    assert np.array_equal(stripe_bytes(stripe), good)
    cols = dependent_four_set(VAND)
    v = null_vector(rs.H[:, list(cols)])
    bad = np.array(good)
    bad[cols[0], 100] ^= v[0]
    bad[cols[1], 100] ^= v[1]
    bad[cols[0], 200] ^= v[0] ^ 0x01 or 0x02
    bad[cols[1], 200] ^= v[1]
    rep = check(device, VAND, bad, [], 2)
    assert (rep.uncorrectable, rep.bad_columns) == (1, 2) and rep.by_weight.tolist() == [0, 0, 1]
    # degraded, on every recoverable single erasure outside the set: the oracle decides
    for j in [i for i in range(14) if i not in cols][:3]:
        if rs.is_recoverable([i for i in range(14) if i != j][:10]):
            check(device, VAND, bad, [j])


def case_erased_rows_are_not_inputs(device):
    good = host_stripe(CAUCHY, 4101)
    bad = np.array(good)
    bad[1, 5] ^= 3
    bad[13, 4100] ^= 0x81
    results = []
    for fill in FILLS:
        work = spoil(bad, [6, 11], fill)
        stripe = to_device(work, device)
        rep = codec(CAUCHY).reconstruct_checked(stripe, [11, 6, 6])
        results.append((stripe_bytes(stripe), rep))
        check(device, CAUCHY, bad, [6, 11], None, 4096, good, fill)
    for rows, rep in results[1:]:
        assert np.array_equal(rows, results[0][0]) and np.array_equal(rep.fixed_bytes, results[0][1].fixed_bytes)
        assert np.array_equal(rep.mask.cpu().numpy(), results[0][1].mask.cpu().numpy())


def unaligned_rows(host: np.ndarray, device, which: int):
    """Separately allocated rows, 16-byte aligned but for row ``which``, one byte off."""
    rows = []
    for j, src in enumerate(host):
        buf = torch.full((src.size + 32,), GARBAGE, dtype=torch.uint8, device=device)
        off = (-buf.data_ptr()) % 16 + (1 if j == which else 0)
        rows.append(buf[off: off + src.size])
        rows[-1].copy_(torch.from_numpy(np.array(src)))
    return rows


def case_unaligned(device, ncols):
    """One row a byte off alignment, a survivor or an erased row: the byte form, the same result."""
    good = host_stripe(CAUCHY, ncols)
    bad = np.array(good)
    bad[0, 0] ^= 1
    bad[12, ncols - 1] ^= 0xFE
    ref = check(device, CAUCHY, bad, [3])
    for which in (3, 7, 13):
        rows = unaligned_rows(spoil(bad, [3], 0xA5), device, which)
        rep = check(device, CAUCHY, bad, [3], None, 4096, good, 0xA5, rows)
        assert np.array_equal(rep.fixed_bytes, ref.fixed_bytes) and np.array_equal(rep.mask.cpu().numpy(),
                                                                                   ref.mask.cpu().numpy())


def batch_hosts(code, nstripes: int, ncols: int, erased):
    """(good, bad, work): stripe b clean (b % 3 == 0), correctable (1) or, where r allows, beyond the
    code (2); the erased rows spoiled."""
    rs = codec(code)
    rng = np.random.default_rng(nstripes * 131 + ncols)
    data = rng.integers(0, 256, size=(nstripes, rs.k, ncols), dtype=np.uint8)
    par = np.stack([gf.GF256.gemm(rs.E, data[:, :, c].T).T for c in range(ncols)], axis=2)
    good = np.concatenate([data, par], axis=1)
    bad = good.copy()
    s = [i for i in range(rs.n) if i not in erased]
    r = rs.p - len(erased)
    b1 = np.arange(1, nstripes, 3)
    bad[b1, s[1], b1 % ncols] ^= 0x21
    b2 = np.arange(2, nstripes, 3)
    for t in range(r // 2 + 1):
        bad[b2, s[2 + t], b2 % ncols] ^= 0x40 + t
    work = bad.copy()
    work[:, erased] = 0xC3
    return good, bad, work


def batch_forms(work: np.ndarray, k: int, device):
    """The batch in each input form: (stripes, parity, read back as [B, n, C])."""
    t = torch.from_numpy(work.copy()).to(device)
    yield t, None, lambda: t.cpu().numpy()
    nat, par = torch.from_numpy(work[:, :k].copy()).to(device), torch.from_numpy(work[:, k:].copy()).to(device)
    yield nat, par, lambda: np.concatenate([nat.cpu().numpy(), par.cpu().numpy()], axis=1)
    if work.shape[0] <= 300:
        lst = [torch.from_numpy(work[b].copy()).to(device) for b in range(work.shape[0])]
        yield lst, None, lambda: np.stack([x.cpu().numpy() for x in lst])


def case_batch(device, nstripes, ncols, code=CAUCHY, erased=(2,)):
    """``report[b]`` and the rows of stripe b equal the single call on stripe b (and the oracle)."""
    rs = codec(code)
    x = list(erased)
    good, bad, work = batch_hosts(code, nstripes, ncols, x)
    sample = sorted(set(range(min(nstripes, 7))) | {nstripes - 1, nstripes // 2, min(nstripes - 1, 65535)})
    wants = {b: oracle(rs.H, work[b], x, default_max_errors(rs.p - len(x)), 4096) for b in sample}
    first = None
    for stripes, parity, read in batch_forms(work, rs.k, device):
        rep = rs.reconstruct_checked_batch(stripes, x, parity, block_bytes=4096)
        assert isinstance(rep, BatchCorrectReport) and len(rep.report) == nstripes
        now = read()
        for b in sample:
            assert_report(rep.report[b], wants[b], now[b])
        if first is None:
            first = (now, rep)
            clean = np.arange(0, nstripes, 3)
            assert rep.clean[clean].all() and not rep.clean[np.arange(1, nstripes, 3)].any()
            assert np.array_equal(now[clean], good[clean])
            fix = np.arange(1, nstripes, 3)
            assert np.array_equal(now[fix], good[fix]) and (rep.by_weight[fix, 1] == 1).all()
            assert rep.dirty == [b for b in range(nstripes) if b % 3]
        else:
            assert np.array_equal(now, first[0]) and np.array_equal(rep.fixed_bytes, first[1].fixed_bytes)
            assert np.array_equal(rep.uncorrectable, first[1].uncorrectable)
            assert np.array_equal(rep.mask.cpu().numpy(), first[1].mask.cpu().numpy())
    # the single call, stripe by stripe
    for b in sample[:6]:
        stripe = torch.from_numpy(work[b].copy()).to(device)
        one = rs.reconstruct_checked(stripe, x, block_bytes=4096)
        assert_report(one, wants[b], stripe.cpu().numpy())
    return first[1]


def case_refusals(device):
    """Every refusal comes before anything is written."""
    rs = codec(CAUCHY)
    host = np.array(host_stripe(CAUCHY, 4101))
    host[2, 9] ^= 1
    stripe = to_device(host, device)
    rows = [stripe[j] for j in range(14)]
    for erased in ([14], [-1], [0, 1, 2, 3, 4], [1.5], "ab", 3):
        with pytest.raises(ValueError):
            rs.reconstruct_checked(stripe, erased)
        with pytest.raises(ValueError):
            rs.reconstruct_checked_batch([stripe], erased)
    for kw in (dict(max_errors=0), dict(max_errors=3), dict(max_errors=True), dict(block_bytes=2048),
               dict(block_bytes=5000)):
        with pytest.raises(ValueError):
            rs.reconstruct_checked(stripe, [1], **kw)
    with pytest.raises(ValueError):  # r = 3 < 4
        rs.reconstruct_checked(stripe, [1], 2)
    with pytest.raises(ValueError):  # r = 4 but e > 0 asked for more
        rs.reconstruct_checked(stripe, [1, 2], 2)
    with pytest.raises(ValueError):
        rs.reconstruct_checked(rows[:5] + [rows[2]] + rows[6:], [1])  # a row listed twice
    with pytest.raises(ValueError):
        rs.reconstruct_checked(rows[:13] + [stripe[12][1:]], [1])  # two rows overlap
    with pytest.raises(ValueError):
        rs.reconstruct_checked_batch([stripe, stripe], [1])  # a stripe listed twice
    with pytest.raises(ValueError):
        rs.reconstruct_checked(rows[:13], [1])  # 13 rows
    with pytest.raises(ValueError):
        rs.reconstruct_checked(rows[:13] + [stripe[13].to(torch.int8)], [1])
    with pytest.raises(ValueError):
        rs.reconstruct_checked(rows[:13] + [flat_rows(stripe)[:8202:2]], [1])  # not contiguous
    if device != "cpu":
        with pytest.raises(ValueError):
            rs.reconstruct_checked(rows[:13] + [stripe[13].cpu()], [1])
    for field, k, n in (("gf65536", 10, 14), ("gf16", 4, 6)):
        with pytest.raises(NotImplementedError):
            ReedSolomon(k, n, "cauchy", field=field).reconstruct_checked(stripe[:n], [1])
    big = (19, 36, "cauchy")
    with pytest.raises(NotImplementedError):
        codec(big).reconstruct_checked(to_device(host_stripe(big, 17), device), [1])
    if device != "cpu":
        torch.cuda.synchronize()
    assert np.array_equal(stripe_bytes(stripe), host)


def case_end_to_end(device):
    """encode, lose e chunks, corrupt a survivor, reconstruct_checked: the syndrome is zero afterwards."""
    rs = ReedSolomon(10, 14, "cauchy")
    ncols = 20011
    stripe = alloc_rows(14, ncols, device, fill=GARBAGE)
    stripe[:10].copy_(torch.from_numpy(np.random.default_rng(5).integers(0, 256, (10, ncols), dtype=np.uint8)))
    rs.encode(stripe[:10], stripe[10:])
    good = stripe_bytes(stripe)
    for x in ([4], [0, 13]):
        for j in x:
            stripe[j].fill_(0)
        stripe[7, 12345] ^= 0x5A
        stripe[12, 3] ^= 0x01
        rep = rs.reconstruct_checked(stripe, x)
        assert rep.by_weight.tolist() == [0, 2, 0] and rep.uncorrectable == 0 and not rep.clean
        assert not rs.syndrome_mask(stripe).cpu().numpy().any()
        assert np.array_equal(stripe_bytes(stripe), good)
        assert rs.reconstruct_checked(stripe, x).clean


def case_empty(device):
    rs = codec(CAUCHY)
    stripe = torch.empty((14, 0), dtype=torch.uint8, device=device)
    rep = rs.reconstruct_checked(stripe, [1])
    assert rep.clean and rep.mask.numel() == 0 and rep.fixed_bytes.tolist() == [0] * 14
    rep = rs.reconstruct_checked_batch(torch.empty((3, 14, 0), dtype=torch.uint8, device=device), [1])
    assert rep.clean.tolist() == [True] * 3 and rep.mask.shape == (3, 0)


# ---- the oracle pinned to the existing oracles --------------------------------------------------------
@pytest.mark.parametrize("code", MDS + [VAND], ids=code_id)
def test_oracle_agrees_with_the_existing_oracles(code):
    rs = codec(code)
    k, n, p = rs.k, rs.n, rs.p
    good = host_stripe(code, 257)
    for e in range(p + 1):
        for x in patterns(k, n, e):
            s = [i for i in range(n) if i not in x]
            if not rs.is_recoverable(s[:k]):
                with pytest.raises(gf.SingularMatrixError):
                    gf.checked_matrix(rs.H, x)
                continue
            t, xs, ss, r_ids = gf.checked_matrix(rs.H, x)
            assert (xs, ss, r_ids) == (x, s, s[k:])
            assert np.array_equal(t[:, x + s[k:]], np.eye(p, dtype=np.uint8))
            work = spoil(good, x, None)
            rows, fixed, by_weight, unc, bad, t2 = gf.reconstruct_checked_oracle(rs.H, work, x)
            assert np.array_equal(t2, t) and (unc, bad, int(fixed.sum()), int(by_weight.sum())) == (0, 0, 0, 0)
            assert np.array_equal(rows, gf.reconstruct_oracle(rs.G, work, x)) and np.array_equal(rows, good)
    # e = 0: T = H, rows and counts are correct_oracle's
    if p >= 2:
        bad = np.array(good)
        bad[0, 3] ^= 7
        bad[n - 1, 200] ^= 0x80
        if p >= 4:
            bad[1, 100] ^= 1
            bad[2, 100] ^= 2
        m = default_max_errors(p)
        got = gf.reconstruct_checked_oracle(rs.H, bad, [], m)
        want = gf.correct_oracle(rs.H, bad, m)
        assert np.array_equal(got[5], rs.H)
        for a, b in zip(got[:5], want):
            assert np.array_equal(a, b)


# ---- the cases on CPU tensors -------------------------------------------------------------------------
@pytest.mark.parametrize("code", MDS, ids=code_id)
def test_ground_truth_on_mds_codes(code):
    case_ground_truth("cpu", code)


def test_pair_search_at_63_survivors():
    case_pair_search_at_63_survivors("cpu")


@pytest.mark.parametrize("ncols", LENGTHS)
def test_row_lengths_and_edges(ncols):
    case_lengths("cpu", ncols)


def test_every_error_value():
    case_every_error_value("cpu")


def test_detection_only_and_nothing_to_check():
    case_detection_only("cpu")


def test_too_many_errors_equal_the_oracle():
    case_too_many_errors("cpu")


def test_reference_vandermonde():
    case_reference_vandermonde("cpu")


def test_erased_rows_are_not_inputs():
    case_erased_rows_are_not_inputs("cpu")


@pytest.mark.parametrize("ncols", [15, 4101])
def test_unaligned_rows(ncols):
    case_unaligned("cpu", ncols)


BATCHES = [(1, 17), (2, 16), (3, 4097), (257, 5)]  # (the GPU module adds 65,537 stripes: two launches)


@pytest.mark.parametrize("nstripes,ncols", BATCHES)
def test_batches(nstripes, ncols):
    case_batch("cpu", nstripes, ncols)


def test_batch_with_uncorrectable_stripes():
    rep = case_batch("cpu", 10, 33, CAUCHY, (1, 2))  # r = 2: two wrong survivors are beyond it
    assert rep.uncorrectable[np.arange(2, 10, 3)].all()


def test_refusals():
    case_refusals("cpu")


def test_end_to_end():
    case_end_to_end("cpu")


def test_empty_stripe():
    case_empty("cpu")


def test_bench_script_runs_on_the_cpu():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "checked_repair_bench.py"), "--device", "cpu"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    import json

    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["device"] == "cpu" and res["results"] and all(r["checked_ms"] > 0 for r in res["results"])
