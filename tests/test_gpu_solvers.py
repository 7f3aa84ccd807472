"""The four device Gauss-Jordan solvers on systems that make them pivot (tests/solver_cases.py):
gf_invert_kernel and gf_decode_system_kernel (gf_invert.hip), the one-workgroup
gf_decode_system16_kernel and the blocked multi-workgroup solve at every panel width
(gf_decode16.hip). X = M^-1 B' is unique whatever the pivot order, so every comparison is exact:
against the numpy oracle for w = 8 and against the host solve (gfrs::gf16w::decode_rows) for w = 16,
which tests/test_solver_cases.py pins to the oracle on the same cases."""
import numpy as np
import pytest
import torch

import solver_cases as sc
from gpu_rscode_amd import ReedSolomon, alloc_rows, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.gf import GF256
from gpu_rscode_amd.ops import Gemm16Plan, GemmPlan, PatternDecoder, gf_invert, invert_into_plan
from gpu_rscode_amd.ops.gemm import perm_tables_from_coeff
from gpu_rscode_amd.ops.inverse import decode_system16_into_plan, decode_system_into_plan

pytestmark = pytest.mark.gpu

ST_FILL, DM_FILL, OUT_FILL = -7, 0x5A5A, 0x6B


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _rs(case) -> ReedSolomon:
    G = sc.system(case)[0]
    rs = ReedSolomon(case.k, case.n, matrix="cauchy", field="gf256" if case.w == 8 else "gf65536")
    rs.E = np.array(G[case.k:])
    rs.G = np.array(G)
    return rs


def _g_dev(case) -> torch.Tensor:
    G = sc.system(case)[0]
    if case.w == 8:
        return torch.from_numpy(np.array(G)).cuda()
    return torch.from_numpy(np.array(G, dtype="<u2").view(np.int16)).cuda()


def _desc_ptrs(plan):
    """(in[k], copy[k], out[m_pad]) of the plan's descriptor."""
    lay, k = plan.layout, plan.k
    d = plan.desc.cpu().numpy()
    word = lambda off, cnt: d[off : off + 8 * cnt].view("<u8").astype(np.uint64).tolist()  # noqa: E731
    return word(lay.in_off, k), word(lay.copy_off, k), word(lay.out_off, plan.m_pad)


def _want_ptrs(dec, rows, erased, ok=True):
    k = dec.k
    p = dec.ptrs.cpu().numpy().astype(np.uint64).tolist()
    chunk, out = p[: dec.n], p[dec.n :]
    return ([chunk[r] for r in rows], [out[r] if ok and r < k else 0 for r in rows],
            [out[erased[i]] if ok and i < len(erased) else 0 for i in range(dec.plan.m_pad)])


# ---- gf_invert ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.INVERT, ids=str)
def test_invert_planted(case):
    """The 64-thread form (n = 4, 32) and the 256-thread form (33 and up; 255 and 256 past 64 KiB of
    LDS) where the lowest row with a nonzero is almost never row c, so nearly every column swaps."""
    m = sc.matrix(case)[0]
    inv, status = gf_invert(torch.from_numpy(np.array(m)).cuda(), check=False)
    assert int(status.item()) == 0
    assert np.array_equal(inv.cpu().numpy(), sc.oracle_inverse(case))


def test_invert_batch_mixes_good_and_late_singular():
    """One launch, one workgroup per matrix: good planted matrices between ones that run out of
    pivots in column 0, n / 2 and n - 1. Exact statuses, singular inverses zeroed, good ones exact."""
    mats = np.stack([sc.matrix(c)[0] for c in sc.INVERT_BATCH])
    assert [c.dep_col for c in sc.INVERT_BATCH] == [None, 0, None, sc.INVERT_BATCH_N // 2, sc.INVERT_BATCH_N - 1]
    inv, status = gf_invert(torch.from_numpy(mats).cuda(), check=False)
    inv = inv.cpu().numpy()
    assert status.cpu().tolist() == [0 if c.good else 1 for c in sc.INVERT_BATCH]
    for b, c in enumerate(sc.INVERT_BATCH):
        assert np.array_equal(inv[b], sc.oracle_inverse(c) if c.good else np.zeros_like(inv[b])), c.id
    with pytest.raises(gf.SingularMatrixError):
        gf_invert(torch.from_numpy(mats).cuda())


def test_invert_into_plan_planted():
    """invert_into_plan with the planted 97 x 97 matrix as G[rows]: the tables of the selected
    inverse rows, in the order selected, equal the oracle rows' records."""
    case = next(c for c in sc.INVERT if c.e == 97)
    n = case.e
    sel = [96, 0, 33, 32, 5, 64, 31, 77, 1, 50, 95, 12, 63]
    plan = GemmPlan(alloc_rows(n, 64, "cuda"), alloc_rows(len(sel), 64, "cuda"), device_tables=True, engine="valu")
    status = invert_into_plan(torch.from_numpy(np.array(sc.matrix(case)[0])).cuda(), plan, sel)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    want = np.transpose(perm_tables_from_coeff(sc.oracle_inverse(case)[sel]), (1, 0, 2))
    got = plan.table_view().cpu().numpy()
    assert np.array_equal(got[:, : len(sel)].view(np.uint32), want.astype(np.uint32))
    assert not got[:, len(sel) :].any()


# ---- decode_system, w = 8 -----------------------------------------------------------------------------
def _tables8(plan, e):
    t = plan.table_view().cpu().numpy()
    return t[:, :e].view(np.uint32), t[:, e:]


def _want_tables8(x):
    return np.transpose(perm_tables_from_coeff(x), (1, 0, 2)).astype(np.uint32)


def _decoder(case, C=64, engine="valu", fill=OUT_FILL):
    k, n, e = case.k, case.n, case.e
    chunks = alloc_rows(n, C, "cuda", fill=0)
    out = alloc_rows(k, C, "cuda", fill=fill)
    dec = PatternDecoder(_g_dev(case), [chunks[i] for i in range(n)], [out[i] for i in range(k)], e, engine=engine)
    dec.erased.fill_(-1)
    dec.status.fill_(ST_FILL)
    return dec, chunks, out


@pytest.mark.parametrize("case", sc.DS8, ids=str)
def test_decode_system8_planted(case):
    """w = 8 decode_system on planted systems up to k = e = 128 (no native survivor in B') and
    n = 256 (ids fill the byte): the tables equal the oracle rows' records, with the erased natives
    given and, from the survivor list alone, derived with the row pointers."""
    G, rows, erased = sc.system(case)
    k, e = case.k, case.e
    want = _want_tables8(sc.oracle_rows(case))
    plan = GemmPlan(alloc_rows(k, 64, "cuda"), alloc_rows(e, 64, "cuda"), device_tables=True, engine="valu")
    status = torch.full((1,), ST_FILL, dtype=torch.int32, device="cuda")
    decode_system_into_plan(_g_dev(case), _i32(rows), _i32(erased), plan, status=status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got, pad = _tables8(plan, e)
    assert np.array_equal(got, want) and not pad.any()

    dec, _, _ = _decoder(case)
    dec.rows.copy_(_i32(rows))
    dec.solve()
    torch.cuda.synchronize()
    assert int(dec.status.item()) == 0
    assert dec.erased.tolist() == list(erased)
    got, pad = _tables8(dec.plan, e)
    assert np.array_equal(got, want) and not pad.any()
    assert _desc_ptrs(dec.plan) == _want_ptrs(dec, rows, erased)


@pytest.mark.parametrize("case", sc.DS8_SINGULAR, ids=str)
def test_decode_system8_singular_at_its_column(case):
    """No pivot in column 0, 1, e / 2 or e - 1 of the k = 100, e = 70 system: status 1; the
    device-built plan keeps its input pointers and the derived natives and names no output."""
    G, rows, erased = sc.system(case)
    plan = GemmPlan(alloc_rows(case.k, 64, "cuda"), alloc_rows(case.e, 64, "cuda"), device_tables=True, engine="valu")
    status = torch.full((1,), ST_FILL, dtype=torch.int32, device="cuda")
    decode_system_into_plan(_g_dev(case), _i32(rows), _i32(erased), plan, status=status)
    dec, _, out = _decoder(case)
    dec.rows.copy_(_i32(rows))
    dec.solve()
    dec.run()
    torch.cuda.synchronize()
    assert int(status.item()) == 1 and int(dec.status.item()) == 1
    assert dec.erased.tolist() == list(erased)
    assert _desc_ptrs(dec.plan) == _want_ptrs(dec, rows, erased, ok=False)
    assert bool((out == OUT_FILL).all())


# ---- decode_system16 ------------------------------------------------------------------------------------
class Solver16:
    """One plan (tables, workspace) and one set of result buffers for repeated w = 16 solves."""

    def __init__(self, case):
        self.case, self.g = case, _g_dev(case)
        k, e = case.k, case.e
        self.plan = Gemm16Plan(alloc_rows(k, 64, "cuda"), alloc_rows(e, 64, "cuda"), device_tables=True,
                               engine="valu16")
        self.erased = torch.zeros(e, dtype=torch.int32, device="cuda")
        self.dm = torch.zeros((e, k), dtype=torch.int16, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def solve(self, rows=None, g=None, **kw):
        """(status, erased, dm, tables[k, e, 4, 8]) with every result buffer refilled first."""
        rows = sc.system(self.case)[1] if rows is None else rows
        self.erased.fill_(-1)
        self.dm.fill_(DM_FILL)
        self.status.fill_(ST_FILL)
        decode_system16_into_plan(self.g if g is None else g, _i32(rows), self.erased, self.plan,
                                  status=self.status, dm=self.dm, **kw)
        torch.cuda.synchronize()
        k, e = self.case.k, self.case.e
        tab = self.plan.desc[self.plan.layout.tab_off :].view(torch.int32).view(k, self.plan.m_pad, 4, 8)
        return (int(self.status.item()), self.erased.tolist(), self.dm.cpu().numpy().view(np.uint16),
                tab[:, :e].cpu().numpy().view(np.uint32))

    def untouched(self):
        torch.cuda.synchronize()
        return (int(self.status.item()) == ST_FILL and bool((self.dm.view(torch.uint8) == 0x5A).all())
                and bool((self.erased == -1).all()))


def _want16(case):
    G, rows, erased = sc.system(case)
    x = _rs(case)._erased_rows(rows, erased)
    return x, np.transpose(gf.perm_quads16(x), (1, 0, 2, 3)).astype(np.uint32)


def _assert_solved(got, case, want=None):
    x, tabs = _want16(case) if want is None else want
    status, erased, dm, tab = got
    assert status == 0
    assert erased == list(sc.system(case)[2])
    assert np.array_equal(dm, x), np.argwhere(dm != x)[:4].tolist()
    assert np.array_equal(tab, tabs)


@pytest.mark.parametrize("case", sc.DS16, ids=str)
def test_decode_system16_one_workgroup_planted(case):
    """The one-workgroup kernel with 64, 32, 16, 8 and 4 lanes per row (e = 1 .. 128) and at
    e = k = 64: decode rows, tables, derived natives and status equal the host solve."""
    assert hip().decode_system16_supported(case.n, case.k, case.e)
    _assert_solved(Solver16(case).solve(), case)


def test_decode_system16_at_and_past_the_one_workgroup_limit():
    """The largest e = k (n = 2 e) the one-workgroup kernel takes, found by asking
    decode_system16_supported: more than 64 KiB of dynamic LDS (the opt-in path), 2 lanes per row.
    One more erasure at the same shape is routed to the blocked solve without being forced."""
    sup = hip().decode_system16_supported
    e = sc.limit_e(sup)
    at, past = sc.limit_case(e), sc.limit_case(e + 1)
    assert sup(at.n, at.k, at.e) and not sup(past.n, past.k, past.e)
    for case in (at, past):
        seq, failed = sc.sequence(case)
        assert failed is None and not sc.sequence_gaps(seq, case.e, case.panels)
    want = _want16(at)
    s = Solver16(at)
    _assert_solved(s.solve(), at, want)
    assert getattr(s.plan, "_solve_ws", None) is None
    _assert_solved(s.solve(force_blocked=True), at, want)
    s = Solver16(past)
    _assert_solved(s.solve(), past)
    assert s.plan._solve_ws is not None  # (the blocked solve's workspace)


# ---- blocked solve --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.DS16 + [sc.BLOCKED_ODD], ids=str)
def test_blocked16_planted_at_its_own_panel_width(case):
    """The same systems forced onto the blocked solve (panel width 32: one panel up to e = 20, a
    ragged second one at e = 40, four at e = 128), and k = 220, e = 37: e % 8 != 0 with W = 257, so
    the row stride is padded and the first panel's y / update grids have a second, one-column block
    that the second panel's do not. Equal to the host solve and to the one-workgroup kernel."""
    want = _want16(case)
    s = Solver16(case)
    one = s.solve()
    blk = s.solve(force_blocked=True)
    _assert_solved(blk, case, want)
    _assert_solved(one, case, want)


@pytest.mark.parametrize("case,P", sc.BLOCKED, ids=lambda v: str(v))
def test_blocked16_every_panel_width(case, P):
    """ds16_panel / y / update <4>, <8>, <16> and <32> (force_panel) at one panel, one panel and a
    column, two panels, two and a column, and e = 70 and 97, where every panel after the first takes
    pivot rows from above and below its own rows. Equal to the host solve and the one-workgroup
    kernel. (The narrow instantiations are what panel_of picks past e of about 2,200, where the
    plan's tables alone are e k 128 bytes: they never run at their natural size here.)"""
    assert case.panels == (P,)
    want = _want16(case)
    s = Solver16(case)
    _assert_solved(s.solve(force_blocked=True, force_panel=P), case, want)
    _assert_solved(s.solve(), case, want)
    _assert_solved(s.solve(force_blocked=True), case, want)  # the same workspace at the default width


def test_blocked16_panel_knob_refusals():
    """force_panel values that name no instantiation (3, 64), and a panel width on a solve that the
    one-workgroup kernel takes, raise with nothing launched: status, dm and erased keep their fill.

    32 where panel_of(e) is narrower: e = 2,400 picks 16 (the e x 32 panel no longer fits the LDS).
    A plan for it would hold e k 128 bytes of tables, so the launcher is called without one: a
    survivor list of zeros is refused by the prep kernel (status 2) and every later kernel returns
    at once, so width 16 is accepted and runs empty, and width 32 is refused."""
    case = sc.LATE
    s = Solver16(case)
    rows = sc.system(case)[1]
    for kw in (dict(force_blocked=True, force_panel=3), dict(force_blocked=True, force_panel=64),
               dict(force_blocked=True, force_panel=-4), dict(force_panel=32)):
        s.erased.fill_(-1)
        s.dm.fill_(DM_FILL)
        s.status.fill_(ST_FILL)
        with pytest.raises(RuntimeError):
            decode_system16_into_plan(s.g, _i32(rows), s.erased, s.plan, status=s.status, dm=s.dm, **kw)
        assert s.untouched(), kw
    _assert_solved(s.solve(force_blocked=True, force_panel=8), case)

    e = k = 2400
    n = 2 * e
    ws_bytes = hip().decode_system16_workspace(n, k, e)
    assert ws_bytes > 0 and not hip().decode_system16_supported(n, k, e)
    g = torch.zeros((n, k), dtype=torch.int16, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    zeros, erased = torch.zeros(k, dtype=torch.int32, device="cuda"), torch.full((e,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((1,), ST_FILL, dtype=torch.int32, device="cuda")

    def launch(panel):
        hip().decode_system16(g.data_ptr(), n, k, zeros.data_ptr(), erased.data_ptr(), e, 0, status.data_ptr(), 0, 0,
                              torch.cuda.current_stream().cuda_stream, 0, ws.data_ptr(), False, panel)
        torch.cuda.synchronize()

    with pytest.raises(RuntimeError):
        launch(32)
    torch.cuda.synchronize()
    assert int(status.item()) == ST_FILL
    launch(16)
    assert int(status.item()) == 2 and bool((erased == -1).all())


# ---- late singularity -----------------------------------------------------------------------------------
def _stripe(case, C, seed):
    """Random natives and their parity under the case's generator, on the device."""
    rs = _rs(case)
    data = alloc_rows(case.k, C, "cuda")
    data.copy_(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(case.k, C), dtype=np.uint8)))
    par = rs.encode(data)
    torch.cuda.synchronize()
    return data, par


def _dec_solve(dec, dm=None, **kw):
    """PatternDecoder.solve with the test knobs of the w = 16 solve (the same decoder state)."""
    if not kw and dm is None:
        return dec.solve()
    return decode_system16_into_plan(dec.g, dec.rows, dec.erased, dec.plan, status=dec.status, ptrs=dec.ptrs, dm=dm, **kw)


_SOLVERS = [("one", {})] + [(f"p{P}", dict(force_blocked=True, force_panel=P)) for P in sc.PANELS]
_LATE = [(name, kw, c) for name, kw in _SOLVERS
         for c in (sc.LATE_COLS[kw["force_panel"]] if kw else sorted(sc.LATE_SINGULAR))]


@pytest.mark.parametrize("name,kw,col", _LATE, ids=[f"{n}-col{c}" for n, _, c in _LATE])
def test_decode_system16_late_singularity_then_good_solve(name, kw, col):
    """The e = 70 system with no pivot in column 0, 1, P - 1, P, P + 1 or e - 1, after the earlier
    panels have updated every row (the one-workgroup kernel: every one of those columns): status 1,
    decode rows all zero, the derived natives still written, and run() stores nothing. The good
    system solved next through the same decoder, plan and workspace decodes exactly (the flags and
    the used / pivot arrays start over)."""
    good, bad = sc.LATE, sc.LATE_SINGULAR[col]
    G, rows, erased = sc.system(good)
    assert sc.system(bad)[1:] == (rows, erased)
    k, n, e, C = good.k, good.n, good.e, 2 * 515
    data, par = _stripe(good, C, col)
    out = alloc_rows(k, C, "cuda", fill=OUT_FILL)
    dec = PatternDecoder(_g_dev(bad), [data[i] for i in range(k)] + [par[i] for i in range(n - k)],
                         [out[i] for i in range(k)], e, engine="valu16")
    dm = torch.full((e, k), DM_FILL, dtype=torch.int16, device="cuda")
    dec.erased.fill_(-1)
    dec.status.fill_(ST_FILL)
    dec.rows.copy_(_i32(rows))
    _dec_solve(dec, dm=dm, **kw)
    dec.run()
    torch.cuda.synchronize()
    assert int(dec.status.item()) == 1
    assert not dm.cpu().numpy().any()
    assert dec.erased.tolist() == list(erased)
    assert _desc_ptrs(dec.plan) == _want_ptrs(dec, rows, erased, ok=False)
    assert bool((out == OUT_FILL).all())

    dec.g.copy_(_g_dev(good))
    _dec_solve(dec, dm=dm, **kw)
    dec.run()
    torch.cuda.synchronize()
    assert int(dec.status.item()) == 0
    assert np.array_equal(dm.cpu().numpy().view(np.uint16), _want16(good)[0])
    assert torch.equal(out, data)


@pytest.mark.parametrize("P", (0,) + sc.PANELS)
def test_blocked16_invalid_pattern_then_good_solve(P):
    """Status 2 on the blocked solve: an id out of range, a negative id, a duplicate. dm is zeroed,
    nothing else is derived, and the good pattern solved next in the same workspace is exact."""
    case = sc.LATE
    rows = list(sc.system(case)[1])
    want = _want16(case)
    s = Solver16(case)
    kw = dict(force_blocked=True, force_panel=P)
    for j, v in ((3, case.n), (case.k - 1, -1), (0, rows[1])):
        bad = list(rows)
        bad[j] = v
        status, erased, dm, _ = s.solve(rows=bad, **kw)
        assert status == 2 and not dm.any() and erased == [-1] * case.e, (j, v)
        _assert_solved(s.solve(**kw), case, want)


# ---- end to end -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,engine,C", [(sc.E2E[0], "valu", 256 * 9 + 77), (sc.E2E[0], "mfma", 256 * 9 + 77),
                                           (sc.E2E[1], "valu16", 512 * 5 + 6), (sc.E2E[1], "mfma", 512 * 5 + 6)],
                         ids=lambda v: str(v))
def test_pattern_decoder_planted_end_to_end(case, engine, C):
    """Encode with the planted generator, hand the decoder the shuffled survivors, and the rebuilt
    and the copied natives equal the data; on the matrix-core engines the bit-matrix is built from
    the device-solved rows (k = 128, e = 26 for w = 8; k = 64, e = 16 for w = 16)."""
    G, rows, erased = sc.system(case)
    k, n, e = case.k, case.n, case.e
    data, par = _stripe(case, C, e)
    out = alloc_rows(k, C, "cuda", fill=OUT_FILL)
    dec = PatternDecoder(_g_dev(case), [data[i] for i in range(k)] + [par[i] for i in range(n - k)],
                         [out[i] for i in range(k)], e, engine=engine)
    assert dec.engine == engine
    dec.rows.copy_(_i32(rows))
    dec.solve()
    dec.run()
    torch.cuda.synchronize()
    assert int(dec.status.item()) == 0
    assert dec.erased.tolist() == list(erased)
    assert torch.equal(out, data)
