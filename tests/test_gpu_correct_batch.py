"""Batched correct on the MI355X (the BATCH instantiations of csrc/kernels/gf_correct.hip): the cases
of tests/test_correct_batch.py on CUDA tensors, every result compared exactly with the numpy oracle
(``gf.correct_oracle``) stripe by stripe and with ``correct`` on copies of single stripes; then a side
stream and the batched launcher called directly."""
import numpy as np
import pytest
import torch

import test_correct_batch as cases
from gpu_rscode_amd import ReedSolomon
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.ops import BatchCorrectPlan, BatchCorrectReport
from test_correct import VAND
from test_scrub import code_id, codec
from test_scrub_batch import batch_to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("code,nstripes,ncols", cases.MIXED_RUNS, ids=map(cases.run_id, cases.MIXED_RUNS))
def test_mixed_batch(code, nstripes, ncols):
    cases.case_mixed("cuda", code, nstripes, ncols)


def test_other_stripes_are_untouched():
    cases.case_other_stripes_untouched("cuda")


@pytest.mark.parametrize("code", [VAND, (9, 14, "cauchy")], ids=code_id)
def test_input_forms(code):
    cases.case_input_forms("cuda", code)


@pytest.mark.parametrize("ncols", [15, 4101])
@pytest.mark.parametrize("code", [VAND, (9, 14, "cauchy")], ids=code_id)
def test_unaligned_rows(code, ncols):
    cases.case_unaligned("cuda", code, ncols)


def test_slice_boundary_at_65537_stripes():
    cases.case_slice_boundary("cuda")


def test_widest_pair_search_and_one_past_it():
    cases.case_wide("cuda")


def test_refusals():
    cases.case_refusals("cuda")


def test_trivial_batches():
    cases.case_trivial("cuda")


def test_correct_batch_on_a_side_stream_and_plan_reuse():
    """Two calls on one side stream, no sync in between: one cache entry; the second call finds the
    batch the first one repaired."""
    rs = ReedSolomon(10, 14)  # a codec of its own: the shared one may hold a plan for these very addresses
    good, bad = cases.damaged_batch(VAND, 3, 8192 + 3)
    stripes = batch_to_device(bad, "cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    r1 = rs.correct_batch(stripes, block_bytes=4096, stream=side)
    r2 = rs.correct_batch(stripes, block_bytes=4096, stream=side)
    assert len(rs._plans) == 1 and r1.mask.data_ptr() != r2.mask.data_ptr()
    plan = next(iter(rs._plans.values()))
    assert isinstance(plan, BatchCorrectPlan) and not any(isinstance(v, torch.Tensor) and v.dim() > 1
                                                          for v in vars(plan).values())  # no hold on the buffers
    side.synchronize()
    assert isinstance(r1, BatchCorrectReport) and r1.dirty == [1, 2] and r1.by_weight.tolist() == [[0, 0, 0], [0, 2, 0], [0, 1, 1]]
    assert r2.clean.all() and not r2.mask.cpu().numpy().any()
    assert np.array_equal(stripes.cpu().numpy(), good)


# ---- the batched launcher, called directly ------------------------------------------------------------
FILL64 = 0x5A5A5A5A5A5A5A5A
GUARD = 8


class Launch:
    """A valid plan of a damaged batch and a 0x5A-filled counts buffer with guard words around the
    [B * (n + 4)] range, for direct launcher calls after the plan's own syndrome launch."""

    def __init__(self, code, nstripes=3, ncols=4101):
        self.rs = codec(code)
        self.n, self.p, self.nstripes, self.ncols = self.rs.n, self.rs.p, nstripes, ncols
        self.good, self.bad = cases.damaged_batch(code, nstripes, ncols)
        self.stripes = batch_to_device(self.bad, "cuda")
        self.plan = BatchCorrectPlan(self.stripes, self.rs.H, None, 4096)
        self.mask = self.plan.syndrome_mask()
        self.counts = torch.full((GUARD + nstripes * (self.n + 4) + GUARD,), FILL64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def correct(self, refused=True, **kw):
        a = dict(p=self.p, batch=self.nstripes, block_bytes=4096, max_errors=self.plan.max_errors)
        a.update(kw)
        args = (int(self.plan.desc.data_ptr()), self.n, a["p"], a["batch"], self.ncols, False, a["block_bytes"],
                int(self.mask.data_ptr()), int(self.plan.loc.data_ptr()), True, a["max_errors"],
                int(self.counts.data_ptr()) + 8 * GUARD, torch.cuda.current_stream().cuda_stream)
        if not refused:
            return hip().correct_batched(*args)
        with pytest.raises(RuntimeError, match="gf_correct_batched"):
            hip().correct_batched(*args)
        torch.cuda.synchronize()
        assert (self.counts.cpu().numpy() == FILL64).all()
        assert np.array_equal(self.stripes.cpu().numpy(), self.bad)


@pytest.mark.parametrize("code", [VAND, (9, 14, "cauchy"), (4, 6, "cauchy")], ids=code_id)
def test_batched_launcher_writes_its_range_only(code):
    r = Launch(code)
    r.correct(refused=False)
    torch.cuda.synchronize()
    counts = r.counts.cpu().numpy()
    assert (counts[:GUARD] == FILL64).all() and (counts[-GUARD:] == FILL64).all()
    rows, fixed, by_weight, unc, nbad, _ = cases.oracle_batch(code, r.bad, r.plan.max_errors, 4096)
    got = counts[GUARD:-GUARD].reshape(r.nstripes, r.n + 4)
    assert np.array_equal(got[:, : r.n], fixed) and np.array_equal(got[:, r.n: r.n + 2], by_weight[:, 1:])
    assert np.array_equal(got[:, r.n + 2], unc) and np.array_equal(got[:, r.n + 3], nbad)
    assert np.array_equal(r.stripes.cpu().numpy(), rows)


def test_batched_launcher_refusals():
    r = Launch(VAND)
    for kw in (dict(batch=0), dict(batch=-1), dict(block_bytes=2048), dict(max_errors=0), dict(max_errors=3),
               dict(p=1), dict(p=3), dict(p=14), dict(p=17)):
        r.correct(**kw)
    small = Launch((4, 6, "cauchy"))
    small.correct(max_errors=2)
