"""The device repair solve on the MI355X (csrc/kernels/gf_repair_solve.hip) and what is built on it:
``solve_patterns``, device-solved ``BatchRepairPlan``s, and ``device_solve=True`` of ``reconstruct``,
``reconstruct_batch`` and ``heal_batch``. The coefficients are unique, so every comparison is exact:
with the host's ``G[erased] . inv(G[survivors])`` (tests/repair_solve_cases.py), with the descriptor
the host path builds, with ``gf.reconstruct_oracle`` and with the default call on copies of the same
bytes. Every launch gets valid pointers; the id lists that the kernel must refuse are small buffers of
ids, checked before any id is used as an index."""
import numpy as np
import pytest
import torch

import repair_solve_cases as rc
import solver_cases as sc
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip
from gpu_rscode_amd.models.rs import UnrecoverableError
from gpu_rscode_amd.ops import BatchRepairPlan
from gpu_rscode_amd.ops import repair as repair_ops
from gpu_rscode_amd.ops.gemm import pad_m
from gpu_rscode_amd.ops.repair import repair_batch_layout, solve_patterns

pytestmark = pytest.mark.gpu

FILL = 0x5A
C1014 = (10, 14, "cauchy")
V1014 = (10, 14, "vandermonde")


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _solve(g: np.ndarray, survivors, erased, m_pad=None, coeff=True, tables=True, fill=FILL):
    """One launch over the patterns ``(survivors[q], erased[q])``: (status list, coeff ``[npat, m_pad,
    k]``, tables ``[npat, k, m_pad, 8]``) as numpy, the outputs prefilled with ``fill`` bytes."""
    sv, er = rc.id_arrays(survivors, erased, m_pad)
    npat, k, mp = sv.shape[0], g.shape[1], er.shape[1]
    co = torch.full((npat, mp, k), fill, dtype=torch.uint8, device="cuda") if coeff else None
    tb = torch.full((npat, k, mp, 32), fill, dtype=torch.uint8, device="cuda") if tables else None
    status = solve_patterns(_dev(g), _dev(sv), _dev(er), mp, coeff_out=co, tables_out=tb)
    assert status.dtype == torch.int32 and status.shape == (npat,) and status.is_cuda
    return (status.cpu().tolist(), None if co is None else co.cpu().numpy(),
            None if tb is None else tb.cpu().numpy().view("<u4").reshape(npat, k, mp, 8))


def _untouched(a: np.ndarray) -> bool:
    return bool((a.view(np.uint8) == FILL).all())


@pytest.fixture(scope="module")
def every_1014():
    """All 1,470 patterns of (10, 14) with their default survivors (shared; do not modify)."""
    pats = rc.all_patterns(14, 4)
    return pats, [rc.first_survivors(14, 10, er) for er in pats]


# ---- exhaustive (10, 14): all 1,470 patterns in one launch ---------------------------------------------
def test_every_pattern_cauchy_in_one_launch(every_1014):
    """Statuses all 0, every coefficient block the host's, and the whole descriptor of a device-solved
    plan byte for byte the one ``build_repair_batch_desc`` makes from host tables: header, pointers,
    pattern ids, padding rows and the gaps between blocks."""
    pats, survs = every_1014
    g = rc.codec(*C1014).G
    status, co, _ = _solve(g, survs, pats, tables=False)
    assert len(pats) == 1470 and status == [0] * 1470
    host = [rc.host_coeff(C1014, sv, er) for sv, er in zip(survs, pats)]
    for q, er in enumerate(pats):
        assert np.array_equal(co[q], rc.coeff_block(host[q], 10, 4)), er
    stripes = torch.zeros((1470, 14, 16), dtype=torch.uint8, device="cuda")
    pat = np.arange(1470)
    solved = BatchRepairPlan(stripes, pat, [(sv, er, None) for sv, er in zip(survs, pats)], g_dev=_dev(g))
    hosted = BatchRepairPlan(stripes, pat, [(sv, er, host[q]) for q, (sv, er) in enumerate(zip(survs, pats))])
    assert solved.status.tolist() == [0] * 1470 and (solved.npat, solved.m_pad, solved.batch) == (1470, 4, 1470)
    assert solved.desc.numel() == repair_batch_layout(10, 4, 1470, 1470)["bytes"]
    assert torch.equal(solved.desc, hosted.desc)


def test_every_pattern_vandermonde_in_one_launch(every_1014):
    """Status 1 on exactly the host's singular set, those blocks untouched, every other block the host's."""
    pats, survs = every_1014
    sing = rc.vandermonde_singular()
    assert len(sing) == 12
    status, co, tb = _solve(rc.codec(*V1014).G, survs, pats)
    assert [er for er, s in zip(pats, status) if s] == sing and set(status) == {0, 1}
    for q, (sv, er) in enumerate(zip(survs, pats)):
        if status[q]:
            assert _untouched(co[q]) and _untouched(tb[q]), er
        else:
            want = rc.host_coeff(V1014, sv, er)
            assert np.array_equal(co[q], rc.coeff_block(want, 10, 4)), er
            assert np.array_equal(tb[q], rc.table_block(want, 10, 4)), er


@pytest.mark.parametrize("npat", [1, 2, 257])
def test_pattern_counts(every_1014, npat):
    """grid.x = pattern (up to 2^31 - 1 of them), so the launcher never splits a launch: 1, 2 and 257
    workgroups, the patterns spread over all 1,470 so that every count of erasures takes part."""
    pats, survs = every_1014
    pick = [int(i) for i in np.linspace(0, 1469, npat)] if npat > 1 else [1469]
    status, co, tb = _solve(rc.codec(*C1014).G, [survs[i] for i in pick], [pats[i] for i in pick])
    assert status == [0] * npat
    for q, i in enumerate(pick):
        want = rc.host_coeff(C1014, survs[i], pats[i])
        assert np.array_equal(co[q], rc.coeff_block(want, 10, 4)) and np.array_equal(tb[q], rc.table_block(want, 10, 4))


# ---- the smallest shapes that can go wrong -------------------------------------------------------------
SHAPES = [
    ("k1-native", (1, 3, "cauchy"), None, (0,), None),
    ("k1-parity", (1, 3, "cauchy"), None, (2,), None),
    ("k1-both", (1, 3, "cauchy"), None, (0, 1), None),
    ("a0-parity-only", C1014, None, (10, 13), None),
    ("a0-all-parity", C1014, None, (10, 11, 12, 13), None),
    ("a1", C1014, None, (4,), None),
    ("a1-and-parity", C1014, None, (4, 12), None),
    ("e=p-natives", C1014, None, (0, 3, 6, 9), None),
    ("e=p-mixed", C1014, None, (1, 2, 11, 13), None),
    ("product-term", C1014, None, (0, 9, 10), None),
    ("m_pad-above-e", C1014, None, (5,), 4),
    ("m_pad-16-for-3", C1014, None, (12, 5, 0), 16),
    ("3-19-e16-natives-gone", (3, 19, "cauchy"), None, tuple(range(16)), None),
    ("3-19-e16-parity-only", (3, 19, "cauchy"), None, tuple(range(3, 19)), None),
    ("128-256-a128", (128, 256, "cauchy"), None, tuple(range(128)), None),
    ("128-256-a127-b1", (128, 256, "cauchy"), None, tuple(range(1, 128)) + (255,), None),
]
SHAPES += [(f"128-160-e{len(er)}-{i}", (128, 160, "cauchy"), None, er, None)
           for i, er in enumerate(rc.WIDE[(128, 160, "cauchy")])]
SHAPES += [(f"60-64-e{len(er)}-{i}", (60, 64, "cauchy"), None, er, None)
           for i, er in enumerate(rc.WIDE[(60, 64, "cauchy")][:4])]
SHAPES += [(f"chosen-{i}", code, sv, er, None) for i, (code, sv, er) in enumerate(rc.CHOSEN)]


@pytest.mark.parametrize("name,code,survivors,erased,m_pad", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(name, code, survivors, erased, m_pad):
    k, n, _ = code
    sv = rc.first_survivors(n, k, erased) if survivors is None else survivors
    mp = pad_m(len(erased)) if m_pad is None else m_pad
    want = rc.host_coeff(code, sv, erased)
    status, co, tb = _solve(rc.codec(*code).G, [sv], [erased], mp)
    assert status == [0]
    assert np.array_equal(co[0], rc.coeff_block(want, k, mp))
    assert np.array_equal(tb[0], rc.table_block(want, k, mp))
    assert np.array_equal(want, gf.repair_coeff_oracle(rc.codec(*code).G, sv, erased))


def test_patterns_of_different_sizes_share_a_launch():
    """a = 0, 1 and 4 and b = 0..4 in one launch at m_pad = 4: the LDS is sized for the largest, every
    workgroup uses its own pitch."""
    erased = [(13,), (0,), (0, 1, 2, 3), (10, 11, 12, 13), (9, 10), (3, 12, 13)]
    survs = [rc.first_survivors(14, 10, er) for er in erased]
    status, co, tb = _solve(rc.codec(*C1014).G, survs, erased, 4)
    assert status == [0] * 6
    for q, (sv, er) in enumerate(zip(survs, erased)):
        want = rc.host_coeff(C1014, sv, er)
        assert np.array_equal(co[q], rc.coeff_block(want, 10, 4)) and np.array_equal(tb[q], rc.table_block(want, 10, 4))


# ---- pivoting: the planted systems of tests/solver_cases.py --------------------------------------------
@pytest.mark.parametrize("case", rc.PIVOT_GOOD, ids=str)
def test_pivoting_systems(case):
    """Scattered pivot order (almost no column picks row c), the survivors shuffled; the erased natives
    alone, then with three lost parity rows among them, whose rows are eliminated but never pivot."""
    g, rows, erased = sc.system(case)
    g = np.array(g)
    lost = [i for i in range(case.k, case.n) if i not in rows][:3]
    both = tuple(lost[:1] + list(erased)[::-1] + lost[1:])
    for er in (tuple(erased), both):
        mp = pad_m(len(er))
        status, co, tb = _solve(g, [rows], [er], mp)
        want = rc.host_coeff_g(g, rows, er)
        assert status == [0]
        assert np.array_equal(co[0], rc.coeff_block(want, case.k, mp)), len(er)
        assert np.array_equal(tb[0], rc.table_block(want, case.k, mp)), len(er)
    first = len(lost[:1])  # (e = 128 at (128, 256): every parity row survives, none is lost)
    assert np.array_equal(co[0][first: first + len(erased)][::-1], sc.oracle_rows(case))


def test_late_singularity_then_a_good_solve_into_the_same_buffers():
    """e = 70 with a dependent column at 0, 1, 35 (the middle) and 69 (e - 1): status 1 at each position
    with the buffers untouched. Every case has a generator of its own, so each is a launch; all write
    into the same buffers, and the good system solved last, after four failed solves, is exact."""
    good = rc.PIVOT_GOOD[1]
    cases = list(rc.PIVOT_SINGULAR) + [good]
    assert [c.dep_col for c in cases] == [0, 1, 35, 69, None] and good.e == 70
    mp = pad_m(70)
    want = None
    co = torch.full((1, mp, good.k), FILL, dtype=torch.uint8, device="cuda")
    tb = torch.full((1, good.k, mp, 32), FILL, dtype=torch.uint8, device="cuda")
    for c in cases:
        g, rows, erased = sc.system(c)
        assert (c.k, c.n, c.e) == (good.k, good.n, good.e)
        sv, er = rc.id_arrays([rows], [erased], mp)
        status = solve_patterns(_dev(np.array(g)), _dev(sv), _dev(er), mp, coeff_out=co, tables_out=tb)
        if c.good:
            want = rc.host_coeff_g(np.array(g), rows, erased)
            assert status.cpu().tolist() == [0]
            assert np.array_equal(co.cpu().numpy()[0], rc.coeff_block(want, c.k, mp))
            assert np.array_equal(tb.cpu().numpy().view("<u4").reshape(c.k, mp, 8), rc.table_block(want, c.k, mp))
        else:
            assert status.cpu().tolist() == [1], c.id
            assert _untouched(co.cpu().numpy()) and _untouched(tb.cpu().numpy()), c.id
    assert want is not None


# ---- the launcher called directly -----------------------------------------------------------------------
def test_null_outputs_and_no_patterns():
    g = rc.codec(*C1014).G
    er = (3, 11)
    sv = rc.first_survivors(14, 10, er)
    want = rc.host_coeff(C1014, sv, er)
    status, co, tb = _solve(g, [sv], [er], coeff=False, tables=False)
    assert status == [0] and co is None and tb is None
    status, co, tb = _solve(g, [sv], [er], tables=False)
    assert status == [0] and np.array_equal(co[0], rc.coeff_block(want, 10, 2))
    status, co, tb = _solve(g, [sv], [er], coeff=False)
    assert status == [0] and np.array_equal(tb[0], rc.table_block(want, 10, 2))
    # npat == 0: a no-op that reads no pointer
    h = hip()
    h.repair_solve(0, 14, 10, 0, 0, 0, 4, 0, 0, 0, 0)
    empty = solve_patterns(_dev(g), torch.zeros((0, 10), dtype=torch.int32, device="cuda"),
                           torch.zeros((0, 4), dtype=torch.int32, device="cuda"), 4)
    assert empty.shape == (0,)
    torch.cuda.synchronize()


def test_launcher_argument_rules():
    """Refused with nothing launched: counts out of range and null required pointers."""
    h = hip()
    gd = _dev(rc.codec(*C1014).G)
    sv, er = (_dev(a) for a in rc.id_arrays([tuple(range(10))], [(10,)], 1))
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ok = (gd.data_ptr(), 14, 10, sv.data_ptr(), er.data_ptr(), 1, 1, 0, 0, st.data_ptr(), 0)
    for pos, value in [(5, -1), (2, 0), (2, 15), (1, 257), (6, 0), (6, 257), (0, 0), (3, 0), (4, 0), (9, 0)]:
        args = list(ok)
        args[pos] = value
        with pytest.raises(RuntimeError):
            h.repair_solve(*args)
    torch.cuda.synchronize()
    assert st.item() == -7
    h.repair_solve(*ok)
    assert st.item() == 0
    assert h.repair_solve_lds_bytes(256, 128, 128) <= 65536 and h.repair_solve_lds_bytes(257, 128, 4) == -1
    with pytest.raises(ValueError):
        solve_patterns(gd, sv.to(torch.int64), er, 1)
    with pytest.raises(ValueError):
        solve_patterns(gd, sv, er, 1, coeff_out=torch.zeros(9, dtype=torch.uint8, device="cuda"))


def test_invalid_lists_give_status_2_and_write_nothing():
    """The guard against out-of-range reads: ids outside [0, n), a survivor twice, an erased id twice, an
    erased id among the survivors. Status 2, no coefficient, no table word; the valid patterns of the same
    launch are solved."""
    base = tuple(range(10))
    lists = [
        (base, (10, 11)),                                  # valid
        (base[:9] + (14,), (10,)),                         # survivor id == n
        (base[:9] + (-1,), (10,)),                         # negative survivor
        (base[:9] + (1 << 20,), (10,)),                    # far out of range
        (base[:9] + (0,), (10,)),                          # survivor twice
        (base, (14,)),                                     # erased id == n
        (base, (-2,)),                                     # below the -1 padding
        (base, (3,)),                                      # erased id is a survivor
        (base, (12, 12)),                                  # erased id twice
        ((13, 12, 11, 10, 9, 8, 7, 6, 5, 4), (0, 1, 2, 3)),  # valid
    ]
    status, co, tb = _solve(rc.codec(*C1014).G, [sv for sv, _ in lists], [er for _, er in lists], 4)
    assert status == [0, 2, 2, 2, 2, 2, 2, 2, 2, 0]
    for q, (sv, er) in enumerate(lists):
        if status[q]:
            assert _untouched(co[q]) and _untouched(tb[q]), q
        else:
            want = rc.host_coeff(C1014, sv, er)
            assert np.array_equal(co[q], rc.coeff_block(want, 10, 4)) and np.array_equal(tb[q], rc.table_block(want, 10, 4))


# ---- reconstruct_batch(device_solve=True) -----------------------------------------------------------------
class _Counting:
    """The native module with ``repair_solve`` and ``repair_batched`` counted."""

    def __init__(self, real):
        self._real, self.solves, self.repairs = real, 0, 0

    def __getattr__(self, name):
        return getattr(self._real, name)

    def repair_solve(self, *a, **kw):
        self.solves += 1
        return self._real.repair_solve(*a, **kw)

    def repair_batched(self, *a, **kw):
        self.repairs += 1
        return self._real.repair_batched(*a, **kw)


@pytest.fixture
def counted(monkeypatch):
    spy = _Counting(hip())
    monkeypatch.setattr(repair_ops, "hip", lambda: spy)
    return spy


def _oracle(g, bad, erased):
    return np.stack([gf.reconstruct_oracle(g, bad[b], [i for i in erased[b] if i >= 0]) for b in range(len(bad))])


def _both_ways(code, erased, ncols, seed, form=None):
    """Damage consistent stripes, repair a copy with the default call and one with ``device_solve=True``
    in guard-filled arenas: both equal the oracle and each other, guards intact. ``form`` turns the
    per-stripe id lists into the ``erased`` argument."""
    k, n, matrix = code
    rs = ReedSolomon(k, n, matrix=matrix)
    good = rc.consistent(rs.G, len(erased), ncols, seed)
    bad = rc.damage(good, erased)
    want = _oracle(rs.G, bad, erased)
    assert np.array_equal(want, good)
    arg = erased if form is None else form(erased)
    bufs = []
    for flag in (False, True):
        buf, stripes = rc.arena(bad, "cuda")
        assert rs.reconstruct_batch(stripes, arg, device_solve=flag) is stripes
        rc.assert_arena(buf, want, f"device_solve={flag}")
        bufs.append(buf)
    assert torch.equal(*bufs)
    return rs


@pytest.mark.parametrize("nstripes,ncols", [(1, 1), (2, 4099), (3, 65539), (257, 33)])
def test_batches(nstripes, ncols, counted):
    """Batches of 1, 2, 3 and 257 stripes, every stripe with a pattern of its own (257 distinct patterns
    at (10, 14)), rows of 1 to 65,539 bytes."""
    pats = rc.all_patterns(14, 4)
    pick = [pats[int(i)] for i in np.linspace(0, 1469, nstripes)] if nstripes > 1 else [(2, 7, 10, 13)]
    assert len(set(pick)) == nstripes
    rs = _both_ways(C1014, pick, ncols, nstripes)
    assert counted.solves == 1 and counted.repairs == 2
    (plan,) = [p for key, p in rs._plans.items() if key[0] == "repbd"]
    assert plan.npat == nstripes and plan.status.tolist() == [0] * nstripes


def test_zero_to_p_erasures_in_every_form():
    """0..p erasures in one batch: ragged lists, the -1 padded array (numpy and CPU tensor, ids in any
    order, one listed twice) and one list shared by every stripe."""
    ragged = [(), (4,), (13, 0), (11, 3, 7), (12, 1, 0, 9), (), (10, 11, 12, 13)]
    _both_ways(C1014, ragged, 1025, 1, form=lambda er: [list(e) for e in er])

    def padded(er):
        a = np.full((len(er), 5), -1, dtype=np.int64)
        for b, ids in enumerate(er):
            a[b, 5 - len(ids):] = ids  # (padding first)
        a[1, 0] = 4  # listed twice
        return a

    _both_ways(C1014, ragged, 1025, 2, form=padded)
    _both_ways(C1014, ragged, 1025, 3, form=lambda er: torch.from_numpy(padded(er)).to(torch.int32))
    _both_ways(C1014, [(9, 2, 12)] * 3, 4099, 4, form=lambda er: [9, 2, 12])
    _both_ways((4, 8, "cauchy"), [(0, 1, 2, 3), (7,), (4, 5, 6, 7), (3, 4)], 17, 5)
    _both_ways((3, 19, "cauchy"), [tuple(range(16)), tuple(range(3, 19)), (1,)], 4099, 6)


def test_one_row_a_byte_off_alignment_takes_the_byte_form():
    rs = ReedSolomon(10, 14, matrix="cauchy")
    erased = [(0, 10), (5,), (13, 12, 1)]
    good = rc.consistent(rs.G, 3, 4099, 8)
    bad = rc.damage(good, erased)
    buf, stripes = rc.arena(bad, "cuda")
    odd = torch.full((4099 + 32,), rc.GUARD, dtype=torch.uint8, device="cuda")
    odd[1: 4100].copy_(stripes[1, 3])
    rows = [[stripes[b, i] for i in range(14)] for b in range(3)]
    rows[1][3] = odd[1: 4100]
    assert rows[1][3].data_ptr() % 16 == 1
    rs.reconstruct_batch(rows, erased, device_solve=True)
    (plan,) = [p for key, p in rs._plans.items() if key[0] == "repbd"]
    assert plan.bytewise
    rc.assert_arena(buf, good)
    got = odd.cpu().numpy()
    assert np.array_equal(got[1: 4100], good[1, 3]) and (got[:1] == rc.GUARD).all() and (got[4100:] == rc.GUARD).all()


def test_side_stream():
    """The solve runs on the current stream at planning, the repair on the side stream after it."""
    rs = ReedSolomon(10, 14, matrix="cauchy")
    erased = [(1, 11), (0, 2, 4, 6), (13,)]
    good = rc.consistent(rs.G, 3, 4099, 9)
    buf, stripes = rc.arena(rc.damage(good, erased), "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rs.reconstruct_batch(stripes, erased, stream=side, device_solve=True)
    side.synchronize()
    rc.assert_arena(buf, good)
    stripes[0, 1] = 7
    torch.cuda.current_stream().synchronize()
    rs.reconstruct_batch(stripes, erased, stream=side, device_solve=True)  # the cached plan
    side.synchronize()
    rc.assert_arena(buf, good)


def test_repeat_call_hits_the_cache_and_solves_nothing(counted):
    rs = ReedSolomon(10, 14, matrix="cauchy")
    erased = np.array([[3, -1], [10, 0], [-1, -1], [12, 13]])
    ids = [[i for i in row if i >= 0] for row in erased.tolist()]
    good = rc.consistent(rs.G, 4, 513, 10)
    bad = rc.damage(good, ids)
    buf, stripes = rc.arena(bad, "cuda")
    rs.reconstruct_batch(stripes, erased, device_solve=True)
    assert (counted.solves, counted.repairs) == (1, 1)
    rc.assert_arena(buf, good)
    stripes.copy_(torch.from_numpy(bad))
    rs.reconstruct_batch(stripes, erased, device_solve=True)
    assert (counted.solves, counted.repairs) == (1, 2)
    rc.assert_arena(buf, good)
    # the default call has a key of its own: a host-solved plan, and no solve launch
    stripes.copy_(torch.from_numpy(bad))
    rs.reconstruct_batch(stripes, erased)
    assert (counted.solves, counted.repairs) == (1, 3)
    assert sorted(key[0] for key in rs._plans) == ["repb", "repbd"]
    rc.assert_arena(buf, good)
    # no host solve was cached by the device-solved call
    fresh = ReedSolomon(10, 14, matrix="cauchy")
    buf2, stripes2 = rc.arena(bad, "cuda")
    fresh.reconstruct_batch(stripes2, erased, device_solve=True)
    assert not fresh._dm
    rc.assert_arena(buf2, good)


# ---- refusals: the arena is unchanged afterwards ------------------------------------------------------------
def test_refusals(counted):
    rs = ReedSolomon(10, 14, matrix="vandermonde")
    sing = rc.vandermonde_singular()
    good = rc.consistent(rs.G, 4, 1025, 12)
    bad = rc.damage(good, [(0,), sing[0], (13, 5), sing[3]])
    buf, stripes = rc.arena(bad, "cuda")
    before = buf.clone()

    def refused(exc, erased, what=stripes, match=None, codec=rs, **kw):
        with pytest.raises(exc, match=match) as ei:
            codec.reconstruct_batch(what, erased, device_solve=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(buf, before)
        return ei.value

    # a singular pattern: the first stripe that uses it is named, the repair kernel is not launched
    err = refused(UnrecoverableError, [[0], list(sing[0]), [13, 5], list(sing[3])], match="stripe 1")
    assert err.stripes == [1, 3] and str(list(sing[0])) in str(err)
    refused(UnrecoverableError, list(sing[5]), match="the pattern")
    assert counted.solves == 2 and counted.repairs == 0 and not rs._plans
    # more than p erasures: refused on the host, before any solve
    refused(UnrecoverableError, [[0], [1, 2, 3, 4, 5], [6], [7]], match="stripe 1")
    # aliasing rows: a stripe listed twice with something to write
    twice = [stripes[0], stripes[1], stripes[0], stripes[2]]
    refused(ValueError, [[0], [1], [2], [3]], what=twice, match="overlaps")
    # ids on the device
    refused(ValueError, torch.tensor([[0], [1], [2], [3]], device="cuda"), match="CPU tensor")
    refused(ValueError, [[0], [14], [2], [3]])
    assert counted.solves == 2 and counted.repairs == 0
    # the other fields
    buf16 = torch.zeros((2, 6, 64), dtype=torch.uint8, device="cuda")
    for field in ("gf16", "gf65536"):
        other = ReedSolomon(4, 6, matrix="cauchy", field=field)
        with pytest.raises(NotImplementedError, match=field):
            other.reconstruct_batch(buf16, [[0], [5]], device_solve=True)
        with pytest.raises(NotImplementedError, match=field):
            other.reconstruct(buf16[0], [0], device_solve=True)
        assert not buf16.any() and not other._plans
    # and what is repairable still is
    rs.reconstruct_batch(stripes, [[0], [], [13, 5], []], device_solve=True)
    want = np.array(bad)
    want[[0, 2]] = good[[0, 2]]
    rc.assert_arena(buf, want)


# ---- reconstruct(device_solve=True) ---------------------------------------------------------------------------
def _plan_of(rs, tag):
    (plan,) = [p for key, p in rs._plans.items() if isinstance(key[0], tuple) and key[0][0] == tag]
    return plan


@pytest.mark.parametrize("code,erased,ncols", [(C1014, (3, 9, 10, 12), 4099), (C1014, (13,), 1),
                                              ((128, 160, "cauchy"), (140,), 4099),
                                              ((128, 160, "cauchy"), tuple(range(3, 99, 3)), 4099),
                                              ((128, 160, "cauchy"), rc.WIDE[(128, 160, "cauchy")][-1], 65539)],
                         ids=["10-14-e4", "10-14-e1-c1", "128-160-e1", "128-160-e32-natives", "128-160-e32"])
def test_reconstruct(code, erased, ncols, counted):
    """One pattern through the kernel, the GEMM on the engine the default call picks."""
    k, n, matrix = code
    rs = ReedSolomon(k, n, matrix=matrix)
    good = rc.consistent(rs.G, 1, ncols, 13)
    bad = rc.damage(good, [erased])
    assert np.array_equal(gf.reconstruct_oracle(rs.G, bad[0], erased), good[0])
    bufs = []
    for flag in (False, True):
        buf, stripes = rc.arena(bad, "cuda")
        assert rs.reconstruct(stripes[0], erased, device_solve=flag) is not None
        rc.assert_arena(buf, good, f"device_solve={flag}")
        bufs.append((buf, stripes))
    assert counted.solves == 1
    assert _plan_of(rs, "repd").engine == _plan_of(rs, "rep").engine
    buf, stripes = bufs[1]
    stripes.copy_(torch.from_numpy(bad))
    rs.reconstruct(stripes[0], erased, device_solve=True)  # the cached plan: no second solve
    assert counted.solves == 1
    rc.assert_arena(buf, good)


@pytest.mark.parametrize("code,survivors,erased", rc.CHOSEN, ids=lambda v: None)
def test_reconstruct_with_chosen_survivors(code, survivors, erased):
    k, n, matrix = code
    rs = ReedSolomon(k, n, matrix=matrix)
    good = rc.consistent(rs.G, 1, 1031, 14)
    # rows that are neither survivors nor erased hold garbage and must stay as they are
    unused = [i for i in range(n) if i not in survivors and i not in erased]
    bad = rc.damage(good, [erased])
    bad[0, unused] = 0x77
    want = np.array(good)
    want[0, unused] = 0x77
    got = []
    for flag in (False, True):
        buf, stripes = rc.arena(bad, "cuda")
        rs.reconstruct(stripes[0], erased, survivors=survivors, device_solve=flag)
        rc.assert_arena(buf, want, f"device_solve={flag}")
        got.append(buf)
    assert torch.equal(*got)


def test_reconstruct_refuses_a_singular_pattern(counted):
    rs = ReedSolomon(10, 14, matrix="vandermonde")
    sing = rc.vandermonde_singular()[-1]
    good = rc.consistent(rs.G, 1, 4099, 15)
    buf, stripes = rc.arena(rc.damage(good, [sing]), "cuda")
    before = buf.clone()
    with pytest.raises(UnrecoverableError, match="singular"):
        rs.reconstruct(stripes[0], sing, device_solve=True)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and counted.solves == 1 and not rs._plans
    with pytest.raises(ValueError):
        rs.reconstruct(stripes[0], [0], survivors=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], device_solve=True)
    with pytest.raises(ValueError):
        rs.reconstruct(stripes[0], [0], survivors=[1, 1, 2, 3, 4, 5, 6, 7, 8, 9], device_solve=True)
    assert torch.equal(buf, before) and counted.solves == 1


# ---- heal_batch(device_solve=True) -------------------------------------------------------------------------------
def test_heal_batch_repairs_33_stripes_and_lists_the_singular_one(counted):
    """Reference Vandermonde (10, 14): 32 stripes with one or two bad chunks are repaired, the stripe
    whose four suspects form a singular pattern is left as it was and listed; no host solve is made."""
    rs = ReedSolomon(10, 14, matrix="vandermonde")
    sing = rc.vandermonde_singular()[0]
    good = rc.consistent(rs.G, 33, 4101, 16)
    bad = np.array(good)
    for b in range(33):
        chunks = sing if b == 17 else ((b % 14,) if b % 3 else (b % 14, (b + 5) % 14))
        for t, i in enumerate(chunks):
            bad[b, i, 100 * t + b: 100 * t + b + 9] ^= 0x21 + t
    buf, stripes = rc.arena(bad, "cuda")
    report = rs.heal_batch(stripes, device_solve=True)
    assert report.unhealed == [17] and report.dirty == [17]
    want = np.array(good)
    want[17] = bad[17]
    rc.assert_arena(buf, want)
    assert counted.solves == 2 and counted.repairs == 1 and not rs._dm
    # the same through the host solve
    buf2, stripes2 = rc.arena(bad, "cuda")
    report2 = rs.heal_batch(stripes2)
    assert report2.unhealed == [17] and torch.equal(buf2, buf)
