"""Correct on the MI355X (csrc/kernels/gf_correct.hip): the cases of tests/test_correct.py on CUDA
tensors, every result compared exactly with the numpy oracle (``gf.correct_oracle``); then the plan, a
side stream and the launcher called directly."""
import numpy as np
import pytest
import torch

import test_correct as cases
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import CorrectPlan, CorrectReport
from gpu_rscode_amd.ops.correct import MAX_PAIR_N
from test_correct import CAUCHY, TOO_WIDE, VAND, WIDE
from test_scrub import code_id, codec, host_stripe, stripe_bytes, to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("code,ncols", cases.SINGLE_RUNS, ids=map(cases.run_id, cases.SINGLE_RUNS))
def test_single_errors_in_every_chunk(code, ncols):
    cases.case_singles("cuda", code, ncols)


@pytest.mark.parametrize("code,ncols", [(c, s) for c in cases.CODES for s in (1, 65, 4097)],
                         ids=lambda v: code_id(v) if isinstance(v, tuple) else f"C{v}")
def test_clean_stripe(code, ncols):
    cases.case_clean("cuda", code, ncols)


@pytest.mark.parametrize("mixed", [False, True], ids=["identity", "mixed"])
def test_every_pair_and_every_error_value(mixed):
    cases.case_every_pair_every_value("cuda", mixed)


@pytest.mark.parametrize("code", [VAND, CAUCHY], ids=code_id)
def test_singles_doubles_and_triples(code):
    cases.case_doubles("cuda", code)


@pytest.mark.parametrize("code", [(9, 14, "cauchy"), (3, 19, "cauchy"), WIDE], ids=code_id)
def test_double_errors_on_other_tiles(code):
    cases.case_pairs_on("cuda", code)


def test_scattered_corruption_that_heal_refuses():
    cases.case_scattered("cuda")


def test_planted_ambiguity_is_left_alone():
    cases.case_planted_ambiguity("cuda")


def test_planted_miscorrection_equals_the_oracle():
    cases.case_planted_miscorrection("cuda")


def test_untouched_bytes():
    cases.case_untouched("cuda")


@pytest.mark.parametrize("ncols", [15, 4101])
@pytest.mark.parametrize("code", [VAND, CAUCHY], ids=code_id)
def test_unaligned_rows(code, ncols):
    cases.case_unaligned("cuda", code, ncols)


def test_refusals():
    cases.case_refusals("cuda")


def test_empty_stripe():
    cases.case_empty("cuda")


def test_an_unaligned_row_puts_the_plan_on_the_byte_form():
    rs = codec(VAND)
    good, bad = cases.doubles_stripe(VAND)
    aligned = to_device(bad, "cuda")
    assert not CorrectPlan(aligned, rs.H).bytewise
    rows = cases.unaligned_rows(bad, "cuda")
    plan = CorrectPlan(rows, rs.H, block_bytes=4096)
    assert plan.bytewise and (plan.max_errors, plan.ncols, plan.nmask, plan.ident) == (2, 4101, 2, 4)
    rep = plan.correct()
    assert isinstance(rep, CorrectReport) and rep.by_weight.tolist() == [0, 14, 182]
    assert np.array_equal(stripe_bytes(rows), gf.correct_oracle(rs.H, bad, 2)[0])


def test_plans_refuse_what_the_codec_refuses():
    rs = codec(VAND)
    bad = np.array(host_stripe(VAND, 4101))
    bad[3, 5] ^= 1
    stripe = to_device(bad, "cuda")
    rows = [stripe[j] for j in range(14)]
    for kw in (dict(max_errors=0), dict(max_errors=3), dict(block_bytes=2048)):
        with pytest.raises(ValueError):
            CorrectPlan(rows, rs.H, **kw)
    with pytest.raises(ValueError):
        CorrectPlan(rows[:5] + [rows[2]] + rows[6:], rs.H)  # a row listed twice
    with pytest.raises(ValueError):
        CorrectPlan(rows, rs.H[:1])  # p = 1 (and the wrong n)
    with pytest.raises(ValueError):
        CorrectPlan(rows, codec((4, 6, "cauchy")).H, 2)  # p = 2
    wide = to_device(host_stripe(TOO_WIDE, 65), "cuda")
    with pytest.raises(NotImplementedError):
        CorrectPlan(wide, codec(TOO_WIDE).H, 2)
    assert CorrectPlan(wide, codec(TOO_WIDE).H, 1).correct().clean
    with pytest.raises(NotImplementedError):
        CorrectPlan(to_device(host_stripe((19, 36, "cauchy"), 17), "cuda"), codec((19, 36, "cauchy")).H)
    with pytest.raises(ValueError):
        CorrectPlan([r.cpu() for r in rows], rs.H)
    torch.cuda.synchronize()
    assert np.array_equal(stripe_bytes(stripe), bad)


def test_correct_on_a_side_stream_and_plan_reuse():
    """Two calls on one side stream, no sync in between: one cache entry, the second call finds the
    stripe the first one repaired."""
    rs = ReedSolomon(10, 14)  # a codec of its own: the shared one may hold a plan for these very addresses
    good, bad = cases.doubles_stripe(VAND)
    stripe = to_device(bad, "cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    r1 = rs.correct(stripe, block_bytes=4096, stream=side)
    r2 = rs.correct(stripe, block_bytes=4096, stream=side)
    assert len(rs._plans) == 1 and r1.mask.data_ptr() != r2.mask.data_ptr()
    plan = next(iter(rs._plans.values()))
    assert isinstance(plan, CorrectPlan) and not any(isinstance(v, torch.Tensor) and v.dim() > 1
                                                     for v in vars(plan).values())  # no hold on the buffers
    side.synchronize()
    cases.assert_report(r1, rs.H, bad, 2, 4096)
    cases.assert_report(r2, rs.H, gf.correct_oracle(rs.H, bad, 2)[0], 2, 4096)
    assert r2.by_weight.tolist() == [0, 0, 0] and r2.uncorrectable == 40 == r2.bad_columns
    rs.correct(stripe, max_errors=1, block_bytes=4096)
    assert len(rs._plans) == 2  # max_errors is part of the key


# ---- the launcher, called directly ------------------------------------------------------------------
FILL64 = 0x5A5A5A5A5A5A5A5A
GUARD = 8  # guard words before and after the range the launcher may write


class Launch:
    """A valid plan of a damaged stripe and a 0x5A-filled counts buffer with guard words around the
    n + 4 words, for direct launcher calls after the plan's own syndrome launch."""

    def __init__(self, code, ncols=4101, max_errors=None):
        self.rs = codec(code)
        self.n, self.p, self.ncols = self.rs.n, self.rs.p, ncols
        self.bad = np.array(host_stripe(code, ncols))
        self.bad[1, 9] ^= 0x31
        self.bad[0, 4097] ^= 0x0F
        self.bad[self.n - 1, 4097] ^= 0xF0
        self.stripe = to_device(self.bad, "cuda")
        self.plan = CorrectPlan(self.stripe, self.rs.H, max_errors, 4096)
        self.mask = self.plan.syndrome_mask()
        self.counts = torch.full((GUARD + self.n + 4 + GUARD,), FILL64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def correct(self, refused=True, **kw):
        a = dict(n=self.n, p=self.p, ncols=self.ncols, bytewise=False, block_bytes=4096, locatable=True,
                 max_errors=self.plan.max_errors)
        a.update(kw)
        args = (int(self.plan.desc.data_ptr()), a["n"], a["p"], a["ncols"], a["bytewise"], a["block_bytes"],
                int(self.mask.data_ptr()), int(self.plan.loc.data_ptr()), a["locatable"], a["max_errors"],
                int(self.counts.data_ptr()) + 8 * GUARD, torch.cuda.current_stream().cuda_stream)
        if not refused:
            return hip().correct(*args)
        with pytest.raises(RuntimeError, match="gf_correct"):
            hip().correct(*args)
        torch.cuda.synchronize()
        assert (self.counts.cpu().numpy() == FILL64).all()
        assert np.array_equal(stripe_bytes(self.stripe), self.bad)


@pytest.mark.parametrize("code", [VAND, (9, 14, "cauchy"), (4, 6, "cauchy")], ids=code_id)
def test_launcher_writes_its_counts_and_the_patched_bytes_only(code):
    r = Launch(code)
    r.correct(refused=False)
    torch.cuda.synchronize()
    counts = r.counts.cpu().numpy()
    assert (counts[:GUARD] == FILL64).all() and (counts[-GUARD:] == FILL64).all()
    rows, fixed, by_weight, unc, nbad = gf.correct_oracle(r.rs.H, r.bad, r.plan.max_errors)
    got = counts[GUARD:-GUARD]
    assert np.array_equal(got[: r.n], fixed) and got[r.n:].tolist() == [by_weight[1], by_weight[2], unc, nbad]
    assert np.array_equal(stripe_bytes(r.stripe), rows)


def test_launcher_leaves_every_bad_column_alone_when_not_locatable():
    r = Launch(VAND)
    r.correct(refused=False, locatable=False)
    torch.cuda.synchronize()
    got = r.counts.cpu().numpy()[GUARD:-GUARD]
    assert got.tolist() == [0] * r.n + [0, 0, 2, 2] and np.array_equal(stripe_bytes(r.stripe), r.bad)


def test_launcher_refusals():
    r = Launch(VAND)
    for kw in (dict(max_errors=0), dict(max_errors=3), dict(block_bytes=2048), dict(block_bytes=12288),
               dict(p=14), dict(p=0), dict(p=1), dict(p=3, max_errors=2), dict(p=17), dict(ncols=-1), dict(n=0)):
        r.correct(**kw)
    r.correct(n=MAX_PAIR_N + 1, max_errors=2)
    small = Launch((4, 6, "cauchy"))  # p = 2
    assert small.plan.max_errors == 1
    small.correct(max_errors=2)
