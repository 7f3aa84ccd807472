"""Checked repair on the MI355X (csrc/kernels/gf_checked.hip): the cases of
tests/test_reconstruct_checked.py on CUDA tensors, every result compared exactly with the numpy oracle
(``gf.reconstruct_checked_oracle``); then stray writes over a guard-filled arena, the plan cache, a
side stream and the launchers called directly."""
import numpy as np
import pytest
import torch

import test_reconstruct_checked as cases
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import BatchCheckedRepairPlan, CheckedRepairPlan
from gpu_rscode_amd.ops.correct import MAX_PAIR_N
from test_reconstruct_checked import CAUCHY, MDS
from test_scrub import code_id, codec, host_stripe, stripe_bytes, to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("code", MDS, ids=code_id)
def test_ground_truth_on_mds_codes(code):
    cases.case_ground_truth("cuda", code)


def test_pair_search_at_63_survivors():
    cases.case_pair_search_at_63_survivors("cuda")


@pytest.mark.parametrize("ncols", cases.LENGTHS)
def test_row_lengths_and_edges(ncols):
    cases.case_lengths("cuda", ncols)


@pytest.mark.parametrize("code,erased", [((4, 8, "cauchy"), (0, 6)), ((9, 14, "cauchy"), (13,)), ((3, 19, "cauchy"), (1, 4, 18))],
                         ids=["4-8-e2", "9-14-e1", "3-19-e3"])
def test_edges_on_the_other_tiles(code, erased):
    cases.case_lengths("cuda", 16385, code, erased)


def test_every_error_value():
    cases.case_every_error_value("cuda")


def test_detection_only_and_nothing_to_check():
    cases.case_detection_only("cuda")


def test_too_many_errors_equal_the_oracle():
    cases.case_too_many_errors("cuda")


def test_reference_vandermonde():
    cases.case_reference_vandermonde("cuda")


def test_erased_rows_are_not_inputs():
    cases.case_erased_rows_are_not_inputs("cuda")


@pytest.mark.parametrize("ncols", [15, 4101])
def test_unaligned_rows(ncols):
    cases.case_unaligned("cuda", ncols)


@pytest.mark.parametrize("nstripes,ncols", cases.BATCHES + [(65537, 1), (65537, 17)])
def test_batches(nstripes, ncols):
    cases.case_batch("cuda", nstripes, ncols)


def test_batch_with_uncorrectable_stripes():
    rep = cases.case_batch("cuda", 10, 33, CAUCHY, (1, 2))
    assert rep.uncorrectable[np.arange(2, 10, 3)].all()


def test_refusals():
    cases.case_refusals("cuda")


def test_end_to_end():
    cases.case_end_to_end("cuda")


def test_empty_stripe():
    cases.case_empty("cuda")


# ---- stray writes: every row a view of one guard-filled arena -------------------------------------------
GUARD_BYTE = 0x6B


class Arena:
    """B stripes of n rows of C bytes at a 256-byte-aligned pitch inside one buffer filled with
    GUARD_BYTE, a guard of 4096 bytes on either side; ``rows(b)`` are views."""

    def __init__(self, nstripes: int, n: int, ncols: int, guard: int = 4096):
        self.pitch = (ncols + 255) // 256 * 256 + 256  # at least 256 bytes of padding after every row
        self.n, self.ncols, self.guard, self.nstripes = n, ncols, guard, nstripes
        raw = torch.full((guard + nstripes * n * self.pitch + guard + 256,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.off = (-raw.data_ptr()) % 256
        self.buf = raw[self.off:]
        self.image = np.full(self.buf.numel(), GUARD_BYTE, dtype=np.uint8)

    def row(self, b: int, j: int) -> torch.Tensor:
        start = self.guard + (b * self.n + j) * self.pitch
        return self.buf[start: start + self.ncols]

    def rows(self, b: int):
        return [self.row(b, j) for j in range(self.n)]

    def load(self, b: int, host: np.ndarray) -> None:
        for j in range(self.n):
            self.row(b, j).copy_(torch.from_numpy(np.array(host[j])))

    def expect(self, b: int, host: np.ndarray) -> None:
        for j in range(self.n):
            start = self.guard + (b * self.n + j) * self.pitch
            self.image[start: start + self.ncols] = host[j]

    def assert_image(self) -> None:
        torch.cuda.synchronize()
        assert np.array_equal(self.buf.cpu().numpy(), self.image)


@pytest.mark.parametrize("ncols", [17, 4101, 16385])
def test_no_stray_writes(ncols):
    """A damaged stripe between two untouched ones: after the call the arena holds the oracle's rows
    for it and every other byte, the other stripes, the pitch padding and the guards, as before."""
    rs = codec(CAUCHY)
    arena = Arena(3, 14, ncols)
    good = host_stripe(CAUCHY, ncols)
    other = np.array(good)
    other[5, 1] ^= 0xFF  # damage in a stripe the call does not name stays
    bad = np.array(good)
    bad[0, 0] ^= 3
    bad[13, ncols - 1] ^= 0x70
    for x in ([2], [9, 10], [0, 1, 12, 13]):
        work = cases.spoil(bad, x, None)
        for b, host in enumerate((other, work, other)):
            arena.load(b, host)
            arena.expect(b, host)
        rep = rs.reconstruct_checked(arena.rows(1), x, block_bytes=4096)
        want = cases.oracle(rs.H, work, x, cases.default_max_errors(4 - len(x)), 4096)
        cases.assert_report(rep, want, stripe_bytes(arena.rows(1)))
        arena.expect(1, want[0])
        arena.assert_image()


def test_no_stray_writes_in_a_batch():
    rs = codec(CAUCHY)
    ncols = 4101
    arena = Arena(4, 14, ncols)
    good = host_stripe(CAUCHY, ncols)
    works = []
    for b in range(4):
        bad = np.array(good)
        if b != 2:
            bad[b, 4096 + b] ^= 1 + b
        works.append(cases.spoil(bad, [7], None, b))
        arena.load(b, works[-1])
    arena.expect(2, works[2])  # stripe 2 is not in the batch
    rep = rs.reconstruct_checked_batch([arena.rows(b) for b in (0, 1, 3)], [7], block_bytes=4096)
    for i, b in enumerate((0, 1, 3)):
        want = cases.oracle(rs.H, works[b], [7], 1, 4096)
        cases.assert_report(rep.report[i], want, stripe_bytes(arena.rows(b)))
        assert np.array_equal(want[0], good)
        arena.expect(b, want[0])
    arena.assert_image()


# ---- plumbing -----------------------------------------------------------------------------------------
def test_plan_cache_keys_on_erased_max_errors_and_block_bytes():
    """Calls that share every base pointer and differ in one argument: the second must miss and be
    right; the first, repeated, must hit."""
    code = (9, 14, "cauchy")  # p = 5: e = 1 leaves r = 4, so max_errors may be 1 or 2
    rs = ReedSolomon(*code[:2], matrix=code[2])
    ncols = 8200
    arena = Arena(1, 14, ncols)
    good = host_stripe(code, ncols)
    bad = np.array(good)
    bad[3, 10] ^= 1
    bad[4, 5000] ^= 2
    bad[8, 5000] ^= 4
    rows = arena.rows(0)

    def call(x, **kw):
        work = cases.spoil(bad, x, None)
        arena.load(0, work)
        before = len(rs._plans)
        rep = rs.reconstruct_checked(rows, x, **kw)
        r = 5 - len(x)
        want = cases.oracle(rs.H, work, x, kw.get("max_errors") or cases.default_max_errors(r), kw.get("block_bytes", 65536))
        cases.assert_report(rep, want, stripe_bytes(rows))
        return len(rs._plans) - before

    assert call([1]) == 1
    assert call([1]) == 0  # a hit
    assert call([2]) == 1  # erased
    assert call([1, 2]) == 1
    assert call([1], max_errors=1) == 1  # max_errors (the default was 2)
    assert call([1], max_errors=2) == 0
    assert call([1], block_bytes=4096) == 1  # block_bytes
    assert call([1], block_bytes=4096) == 0
    assert call([1]) == 0
    plan = next(iter(rs._plans.values()))
    assert isinstance(plan, CheckedRepairPlan) and (plan.e, plan.r, plan.ns, plan.max_errors) == (1, 4, 13, 2)
    assert not any(isinstance(v, torch.Tensor) and v.dim() > 1 for v in vars(plan).values())  # no hold on the buffers
    # batched: the same buffer as one stripe of a batch is another entry, and so is another erasure list
    t = arena.buf[arena.guard: arena.guard + 14 * arena.pitch].view(1, 14, arena.pitch)[:, :, :ncols]
    before = len(rs._plans)
    for x, grew in (([1], 1), ([1], 0), ([3], 1)):
        work = cases.spoil(bad, x, None)
        arena.load(0, work)
        n0 = len(rs._plans)
        rep = rs.reconstruct_checked_batch(t, x)
        assert len(rs._plans) - n0 == grew
        cases.assert_report(rep.report[0], cases.oracle(rs.H, work, x, 2, 65536), stripe_bytes(rows))
    assert len(rs._plans) - before == 2
    assert isinstance(list(rs._plans.values())[-1], BatchCheckedRepairPlan)


def test_an_unaligned_row_puts_the_plan_on_the_byte_form():
    rs = codec(CAUCHY)
    host = host_stripe(CAUCHY, 4101)
    assert not CheckedRepairPlan(to_device(host, "cuda"), rs.H, [3]).bytewise
    for which in (3, 9):  # the erased row, a survivor
        assert CheckedRepairPlan(cases.unaligned_rows(host, "cuda", which), rs.H, [3]).bytewise


def test_side_stream_and_plan_reuse():
    """Two calls on one side stream, no sync in between: one cache entry, the second call finds the
    stripe the first one repaired."""
    rs = ReedSolomon(10, 14, "cauchy")
    good = host_stripe(CAUCHY, 20011)
    bad = np.array(good)
    bad[5, 7] ^= 0x11
    bad[11, 20010] ^= 0x22
    work = cases.spoil(bad, [0, 13], 0x00)
    stripe = to_device(work, "cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    r1 = rs.reconstruct_checked(stripe, [0, 13], block_bytes=4096, stream=side)
    r2 = rs.reconstruct_checked(stripe, [13, 0], block_bytes=4096, stream=side)
    assert len(rs._plans) == 1 and r1.mask.data_ptr() != r2.mask.data_ptr()
    side.synchronize()
    cases.assert_report(r1, cases.oracle(rs.H, work, [0, 13], 1, 4096), good)
    assert r2.clean and not r2.mask.cpu().numpy().any()
    assert np.array_equal(stripe_bytes(stripe), good)


def test_plans_refuse_what_the_codec_refuses():
    rs = codec(CAUCHY)
    host = np.array(host_stripe(CAUCHY, 4101))
    stripe = to_device(host, "cuda")
    rows = [stripe[j] for j in range(14)]
    for kw in (dict(max_errors=0), dict(max_errors=2), dict(block_bytes=2048)):
        with pytest.raises(ValueError):
            CheckedRepairPlan(rows, rs.H, [1], **kw)
    for erased in ([14], [0, 1, 2, 3, 4]):
        with pytest.raises(ValueError):
            CheckedRepairPlan(rows, rs.H, erased)
    with pytest.raises(ValueError):
        CheckedRepairPlan(rows[:5] + [rows[2]] + rows[6:], rs.H, [1])
    with pytest.raises(ValueError):
        CheckedRepairPlan([r.cpu() for r in rows], rs.H, [1])
    with pytest.raises(gf.SingularMatrixError):
        vand = codec(cases.VAND)
        CheckedRepairPlan(rows, vand.H, cases.singular_pattern(cases.VAND))
    torch.cuda.synchronize()
    assert np.array_equal(stripe_bytes(stripe), host)


# ---- the launchers, called directly -------------------------------------------------------------------
FILL64 = 0x5A5A5A5A5A5A5A5A
FILL32 = 0x5A5A5A5A
GUARD = 8


class Launch:
    """A valid plan of a damaged degraded stripe, with 0x5A-filled mask and counts buffers of their
    own and guard words around both."""

    def __init__(self, code=(9, 14, "cauchy"), erased=(2,), ncols=4101):
        self.rs = codec(code)
        self.bad = np.array(host_stripe(code, ncols))
        self.bad[1, 9] ^= 0x31
        self.bad[0, 4097] ^= 0x0F
        self.bad[13, 4097] ^= 0xF0
        self.work = cases.spoil(self.bad, erased, 0x00)
        self.stripe = to_device(self.work, "cuda")
        self.plan = CheckedRepairPlan(self.stripe, self.rs.H, list(erased), None, 4096)
        self.ncols, self.nmask = ncols, self.plan.nmask
        self.mask = torch.full((GUARD + self.nmask + GUARD,), FILL32, dtype=torch.int32, device="cuda")
        self.counts = torch.full((GUARD + self.plan.ns + 4 + GUARD,), FILL64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def args(self, kw):
        p = self.plan
        a = dict(ns=p.ns, e=p.e, r=p.r, ncols=self.ncols, bytewise=False, block_bytes=4096, locatable=p.locatable,
                 max_errors=p.max_errors, desc=int(p.desc.data_ptr()), mask=int(self.mask.data_ptr()) + 4 * GUARD,
                 loc=int(p.loc.data_ptr()), counts=int(self.counts.data_ptr()) + 8 * GUARD)
        a.update(kw)
        return a

    def hot(self, **kw):
        a = self.args(kw)
        return hip().checked(a["desc"], a["ns"], a["e"], a["r"], a["ncols"], a["bytewise"], a["block_bytes"], a["mask"],
                             torch.cuda.current_stream().cuda_stream)

    def fix(self, **kw):
        a = self.args(kw)
        return hip().checked_fix(a["desc"], a["ns"], a["e"], a["r"], a["ncols"], a["bytewise"], a["block_bytes"],
                                 a["mask"], a["loc"], a["locatable"], a["max_errors"], a["counts"],
                                 torch.cuda.current_stream().cuda_stream)

    def batched(self, which, batch, **kw):
        a = self.args(kw)
        lead = (a["desc"], a["ns"], a["e"], a["r"], batch, a["ncols"], a["bytewise"], a["block_bytes"], a["mask"])
        st = torch.cuda.current_stream().cuda_stream
        if which == "hot":
            return hip().checked_batched(*lead, st)
        return hip().checked_fix_batched(*lead, a["loc"], a["locatable"], a["max_errors"], a["counts"], st)

    def assert_untouched(self):
        torch.cuda.synchronize()
        assert (self.mask.cpu().numpy() == FILL32).all() and (self.counts.cpu().numpy() == FILL64).all()
        assert np.array_equal(stripe_bytes(self.stripe), self.work)


def test_launchers_write_their_outputs_only():
    r = Launch()
    r.hot()
    r.fix()
    torch.cuda.synchronize()
    mask, counts = r.mask.cpu().numpy(), r.counts.cpu().numpy()
    for buf, fill in ((mask, FILL32), (counts, FILL64)):
        assert (buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all()
    rows, fixed, by_weight, unc, nbad, want_mask = cases.oracle(r.rs.H, r.work, [2], 2, 4096)
    assert np.array_equal(mask[GUARD:-GUARD], want_mask)
    got = counts[GUARD:-GUARD]
    s = r.plan.survivors
    assert np.array_equal(got[: len(s)], fixed[s]) and got[len(s):].tolist() == [by_weight[1], by_weight[2], unc, nbad]
    assert by_weight.tolist() == [0, 1, 1] and np.array_equal(stripe_bytes(r.stripe), rows)


def test_launcher_refusals():
    r = Launch()
    bad_common = (dict(block_bytes=2048), dict(block_bytes=12288), dict(ncols=-1), dict(ns=0), dict(ns=257), dict(e=-1),
                  dict(r=-1), dict(e=0, r=0), dict(e=13, r=4), dict(r=13), dict(desc=0), dict(mask=0))
    for kw in bad_common:
        with pytest.raises(RuntimeError, match="gf_checked"):
            r.hot(**kw)
        with pytest.raises(RuntimeError, match="gf_checked_batched"):
            r.batched("hot", 1, **kw)
        r.assert_untouched()
    for kw in bad_common + (dict(max_errors=0), dict(max_errors=3), dict(r=3, max_errors=2), dict(e=5, r=0),
                            dict(ns=MAX_PAIR_N + 1, max_errors=2), dict(loc=0), dict(counts=0)):
        with pytest.raises(RuntimeError, match="gf_checked_fix"):
            r.fix(**kw)
        with pytest.raises(RuntimeError, match="gf_checked_fix_batched"):
            r.batched("fix", 1, **kw)
        r.assert_untouched()
    for which in ("hot", "fix"):
        for batch in (0, -1):
            with pytest.raises(RuntimeError, match="invalid argument"):
                r.batched(which, batch)
    r.assert_untouched()
