"""The C API's device layer on the MI355X (csrc/capi/gfrs_capi.cpp over lib/libgfrs.so): plans,
the device-built decoder, the in-place update and the host pipeline, each compared exactly with the
numpy oracle (``GF256.gemm``, ``rs.G``, ``rs.E``). The library repeats in C++ what ops/gemm.py does
in Python (descriptor, alignment and stride detection, engine choice, bit-matrix, passes of 8,
placeholder pointers), so every row here is a view of a guard-filled arena (tests/capi_cases.py)
that is compared as a whole: a wrong stride, a stale table or a copy pitch off by one shows as bytes
outside the oracle's rows or as oracle bytes that were not stored."""
import ctypes

import numpy as np
import pytest
import torch

import capi_cases as cc
from capi_cases import AUTO, EINVAL, MFMA, OK, VALU
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import hip

pytestmark = pytest.mark.gpu

ENGINE_NAME = {AUTO: "auto", VALU: "valu", MFMA: "mfma"}


@pytest.fixture(scope="module")
def lib():
    lib = cc.load()
    yield lib
    assert lib.gfrs_release() == OK


def auto_engine(k: int, m: int, aligned: bool = True) -> int:
    """gfrs.h: "Engine AUTO picks the FP4 matrix-core kernel for wide stripes (k >= 64, m >= 16)";
    rows that are not 16-byte aligned stay on the v_perm kernel's byte form."""
    return MFMA if aligned and k >= 64 and m >= 16 else VALU


# ---- 1. gfrs_plan -----------------------------------------------------------------------------------
VALU_SHAPES = [(1, 1, 1), (3, 2, 17), (10, 4, 4101), (16, 5, 4097), (20, 17, 777), (40, 9, 4101), (255, 1, 300)]
MFMA_SHAPES = [(128, 32), (128, 26), (128, 16), (128, 8), (100, 17), (40, 32), (64, 16), (1, 1)]
CHUNKS_AND_REMAINDER = 256 * 5 + 77
MFMA_LENGTHS = [CHUNKS_AND_REMAINDER, 200, 768]  # whole chunks + a v_perm remainder, remainder only, no remainder
LAYOUTS = ["uniform", "scattered", "reversed"]
COPIES = ["null", "all", "alternate", "head"]


def _plan_cases():
    cases = []
    for k, m, c in VALU_SHAPES:
        cases += [(k, m, c, VALU, lay, cp) for lay in LAYOUTS for cp in COPIES]
        cases.append((k, m, c, AUTO, "uniform", "null"))
    for k, m in MFMA_SHAPES:
        for c in MFMA_LENGTHS:
            cases += [(k, m, c, MFMA, lay, cp) for lay in LAYOUTS for cp in COPIES]
            if auto_engine(k, m) == MFMA:
                cases += [(k, m, c, AUTO, "uniform", cp) for cp in ("null", "all")]
    # k = 2: any two rows are "equally spaced", here the second below the first and further off than a row
    for m in (2, 32):
        for c in (CHUNKS_AND_REMAINDER, 200):
            cases += [(2, m, c, eng, "k2", cp) for eng in (VALU, MFMA) for cp in COPIES]
    return cases


def _case_id(case):
    k, m, c, eng, lay, cp = case
    return f"k{k}-m{m}-C{c}-{ENGINE_NAME[eng]}-{lay}-copy_{cp}"


def lay_rows(arena, layout: str, count: int, n: int, seed: int):
    if layout == "uniform":
        return arena.rows(count, n)
    if layout == "reversed":
        return arena.rows(count, n)[::-1]
    if layout == "scattered":
        return arena.scattered(count, n, seed)
    assert layout == "k2" and count == 2
    low = arena.take(n, 0, 3 * 256)
    return [arena.take(n), low]


def copy_mask(mode: str, k: int, m: int):
    """Which inputs have a copy destination; None = the copy argument itself is NULL."""
    if mode == "null":
        return None
    if mode == "all":
        return [True] * k
    if mode == "alternate":
        return [j % 2 == 1 for j in range(k)]
    assert mode == "head"
    return [j < k - m for j in range(k)]


class PlanSetup:
    """The rows of one plan in one arena, inputs stored, outputs and copies expected in the image."""

    def __init__(self, k, m, c, layout="uniform", copy="null", shifts=None, seed=0):
        shifts = shifts or {}
        self.k, self.m, self.c = k, m, c
        self.coeff, self.data, self.want = cc.gemm_case(k, m, max(c, 1), seed)
        self.arena = cc.DeviceArena(cc.arena_bytes(2 * k + m, c))
        a = self.arena

        def rows(name, count, lay, seed, moved):
            if name in shifts:  # one row of a uniform set moved off its 16-byte boundary
                return [a.take(c, shifts[name] if j == moved else 0) for j in range(count)]
            return lay_rows(a, lay, count, c, seed)

        self.ins = rows("in", k, layout, 1, k // 2)
        self.outs = rows("out", m, "uniform" if layout == "k2" else layout, 2, m - 1)
        mask = copy_mask(copy, k, m)
        self.copies = None
        if mask is not None:
            self.copies = [r if keep else None for r, keep in zip(rows("copy", k, layout, 3, 1), mask)]
        for j, r in enumerate(self.ins):
            r.put(self.data[j, :c])
        self.in_ptrs = cc.ptr_array([r.ptr for r in self.ins])
        self.out_ptrs = cc.ptr_array([r.ptr for r in self.outs])
        self.copy_ptrs = None if self.copies is None else cc.ptr_array([r.ptr if r else 0 for r in self.copies])

    def create(self, lib, engine, ncols=None, coeff=None):
        plan = ctypes.c_void_p()
        rc = lib.gfrs_plan_create(ctypes.byref(plan), 0, self.k, self.m, cc.coeff_bytes(self.coeff if coeff is None else coeff),
                                  self.in_ptrs, self.out_ptrs, self.copy_ptrs, self.c if ncols is None else ncols, engine)
        return rc, plan

    def expect(self, want=None):
        want = self.want if want is None else want
        for i, r in enumerate(self.outs):
            r.expect(want[i, :self.c])
        for j, r in enumerate(self.copies or []):
            if r is not None:  # a row with no destination leaves its buffer at the fill value
                r.expect(self.data[j, :self.c])


@pytest.mark.parametrize("case", _plan_cases(), ids=_case_id)
def test_plan_matches_oracle(lib, case):
    k, m, c, engine, layout, copy = case
    s = PlanSetup(k, m, c, layout, copy)
    torch.cuda.synchronize()
    rc, plan = s.create(lib, engine)
    assert rc == OK, cc.err(lib)
    try:
        assert lib.gfrs_plan_engine(plan) == (engine or auto_engine(k, m))
        assert lib.gfrs_plan_run(plan, None) == OK, cc.err(lib)
        s.expect()
        s.arena.check(_case_id(case))
    finally:
        lib.gfrs_plan_destroy(plan)


@pytest.mark.parametrize("k,m,want", [(63, 16, VALU), (64, 15, VALU), (64, 16, MFMA)])
def test_plan_auto_engine_choice(lib, k, m, want):
    s = PlanSetup(k, m, CHUNKS_AND_REMAINDER)
    torch.cuda.synchronize()
    rc, plan = s.create(lib, AUTO)
    assert rc == OK, cc.err(lib)
    try:
        assert lib.gfrs_plan_engine(plan) == want
        assert lib.gfrs_plan_run(plan, None) == OK, cc.err(lib)
        s.expect()
        s.arena.check(f"AUTO at k={k} m={m}")
    finally:
        lib.gfrs_plan_destroy(plan)


UNALIGNED = [{"in": 1}, {"out": 3}, {"copy": 2}]


@pytest.mark.parametrize("shifts", UNALIGNED, ids=lambda s: "+".join(f"{r}{v}" for r, v in s.items()))
def test_plan_unaligned_rows(lib, shifts):
    """One row off its 16-byte boundary at (64, 16), where aligned rows would go to the matrix
    cores: AUTO reports VALU and is exact, VALU is exact, and a forced MFMA plan is refused on the
    host with nothing written."""
    k, m, c = 64, 16, CHUNKS_AND_REMAINDER
    for engine in (AUTO, VALU):
        s = PlanSetup(k, m, c, copy="all", shifts=shifts)
        torch.cuda.synchronize()
        rc, plan = s.create(lib, engine)
        assert rc == OK, cc.err(lib)
        try:
            assert lib.gfrs_plan_engine(plan) == VALU
            assert lib.gfrs_plan_run(plan, None) == OK, cc.err(lib)
            s.expect()
            s.arena.check(f"{ENGINE_NAME[engine]} with {shifts}")
        finally:
            lib.gfrs_plan_destroy(plan)
    s = PlanSetup(k, m, c, copy="all", shifts=shifts)
    torch.cuda.synchronize()
    rc, plan = s.create(lib, MFMA)
    assert rc == EINVAL and not plan.value
    assert "aligned" in cc.err(lib)
    s.arena.check(f"refused MFMA plan with {shifts}")


@pytest.mark.parametrize("engine", [VALU, MFMA], ids=ENGINE_NAME.get)
@pytest.mark.parametrize("k,m", [(128, 26), (10, 4)])
def test_plan_set_coeff(lib, engine, k, m):
    """Run, set a second matrix, run again: the second matrix's oracle everywhere. On the matrix-core
    engine the whole chunks come from the bit-matrix and the remainder from the v_perm tables, so a
    stale one of the two shows in one region only; the regions are asserted apart."""
    c = CHUNKS_AND_REMAINDER
    whole = c // 256 * 256
    s = PlanSetup(k, m, c, copy="head")
    second = cc.noise([k, m, 99], m, k)
    want2 = gf.GF256.gemm(second, s.data).astype(np.uint8)
    # the two matrices must disagree in every output row and both regions, or the test proves nothing
    assert all((s.want[i, :whole] != want2[i, :whole]).any() and (s.want[i, whole:] != want2[i, whole:]).any()
               for i in range(m))
    torch.cuda.synchronize()
    rc, plan = s.create(lib, engine)
    assert rc == OK, cc.err(lib)
    try:
        assert lib.gfrs_plan_run(plan, None) == OK
        s.expect()
        s.arena.check("first matrix")
        assert lib.gfrs_plan_set_coeff(plan, cc.coeff_bytes(second)) == OK, cc.err(lib)
        assert lib.gfrs_plan_engine(plan) == engine
        assert lib.gfrs_plan_run(plan, None) == OK
        s.expect(want2)
        got = s.arena.snapshot()
        for i, r in enumerate(s.outs):
            assert s.arena.region_equal(got, r, 0, whole), \
                f"whole-chunk region [0, {whole}) of output {i} is not the second matrix's (stale bit-matrix or table)"
            assert s.arena.region_equal(got, r, whole, c), \
                f"remainder region [{whole}, {c}) of output {i} is not the second matrix's (stale v_perm table)"
        s.arena.check("second matrix")
        assert lib.gfrs_plan_set_coeff(plan, None) == EINVAL and lib.gfrs_plan_set_coeff(None, cc.coeff_bytes(second)) == EINVAL
    finally:
        lib.gfrs_plan_destroy(plan)


@pytest.mark.parametrize("engine,k,m", [(VALU, 10, 4), (MFMA, 128, 32)], ids=["valu", "mfma"])
def test_plan_two_runs_and_zero_columns(lib, engine, k, m):
    c = CHUNKS_AND_REMAINDER
    s = PlanSetup(k, m, c, copy="all")
    torch.cuda.synchronize()
    rc, plan = s.create(lib, engine)
    assert rc == OK, cc.err(lib)
    rc0, empty = s.create(lib, engine, ncols=0)
    assert rc0 == OK, cc.err(lib)
    try:
        assert lib.gfrs_plan_run(empty, None) == OK, cc.err(lib)
        s.arena.check("ncols == 0 writes nothing")
        assert lib.gfrs_plan_run(plan, None) == OK
        s.expect()
        s.arena.check("first run")
        assert lib.gfrs_plan_run(plan, None) == OK
        s.arena.check("second run")
    finally:
        lib.gfrs_plan_destroy(plan)
        lib.gfrs_plan_destroy(empty)


@pytest.mark.parametrize("engine,k,m", [(VALU, 10, 4), (MFMA, 128, 32)], ids=["valu", "mfma"])
def test_plan_on_a_side_stream(lib, engine, k, m):
    """The inputs are uploaded on a torch side stream and the plan runs on it with no sync between."""
    c = CHUNKS_AND_REMAINDER
    s = PlanSetup(k, m, c, copy="alternate")
    fresh = cc.noise([k, c, 5], k, c)
    pinned = torch.from_numpy(fresh).pin_memory()
    torch.cuda.synchronize()
    rc, plan = s.create(lib, engine)
    assert rc == OK, cc.err(lib)
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for j, r in enumerate(s.ins):
                s.arena.tensor(r).copy_(pinned[j], non_blocking=True)
            assert lib.gfrs_plan_run(plan, side.cuda_stream) == OK, cc.err(lib)
        side.synchronize()
        want = gf.GF256.gemm(s.coeff, fresh).astype(np.uint8)
        for j, r in enumerate(s.ins):
            r.expect(fresh[j])
        s.data = fresh
        s.expect(want)
        s.arena.check("side stream")
    finally:
        lib.gfrs_plan_destroy(plan)


# ---- 2. gfrs_decoder ---------------------------------------------------------------------------------
DEC_C = 256 * 3 + 77
DECODERS = [(4, 2, 1, AUTO), (4, 2, 2, AUTO), (10, 4, 1, AUTO), (10, 4, 2, AUTO), (10, 4, 3, AUTO), (10, 4, 4, AUTO),
            (3, 5, 3, AUTO), (128, 32, 8, AUTO), (128, 32, 16, AUTO), (128, 32, 26, AUTO), (128, 32, 32, AUTO),
            (100, 28, 17, MFMA), (10, 4, 4, MFMA)]


def pattern(k: int, p: int, e: int, seed, shift: int = 0):
    """(survivor ids in a shuffled order, erased natives): e natives lost, the other k - e natives
    survive with e parity rows chosen at random (the other p - e parity rows are lost too). ``shift``
    moves the lost natives round by that many ids: another set whenever e < k."""
    rng = np.random.default_rng(seed)
    lost = np.sort((rng.choice(k, size=e, replace=False) + shift) % k)
    natives = [j for j in range(k) if j not in set(lost.tolist())]
    parity = (k + rng.choice(p, size=e, replace=False)).tolist()
    rows = np.array(natives + parity, dtype=np.int32)
    return rng.permutation(rows).astype(np.int32), lost.tolist()


class DecoderSetup:
    def __init__(self, lib, k, p, e, engine, matrix="cauchy", ncols=DEC_C):
        self.lib, self.k, self.p, self.e, self.n, self.c = lib, k, p, e, k + p, ncols
        self.rs = ReedSolomon(k, k + p, matrix=matrix)
        self.data = cc.noise([k, p, 7], k, ncols)
        self.stripe = np.vstack([self.data, gf.GF256.gemm(self.rs.E, self.data).astype(np.uint8)])
        self.arena = cc.DeviceArena(cc.arena_bytes(self.n + k, ncols))
        self.chunks = self.arena.rows(self.n, ncols)
        self.outs = self.arena.rows(k, ncols)
        self.dec = ctypes.c_void_p()
        torch.cuda.synchronize()
        rc = lib.gfrs_decoder_create(ctypes.byref(self.dec), 0, k, p, cc.coeff_bytes(self.rs.E),
                                     cc.ptr_array([r.ptr for r in self.chunks]), cc.ptr_array([r.ptr for r in self.outs]),
                                     ncols, e, engine)
        assert rc == OK, cc.err(lib)

    def load(self, rows) -> None:
        """The survivors hold the stripe, every lost chunk row holds junk (it is never read), and the
        output rows are back at the fill value."""
        alive = set(int(r) for r in rows if 0 <= r < self.n)
        for j, r in enumerate(self.chunks):
            r.put(self.stripe[j] if j in alive else np.full(self.c, 0x3C, dtype=np.uint8))
        for r in self.outs:
            r.put(np.full(self.c, cc.GUARD, dtype=np.uint8))

    def solve(self, rows, external=False) -> int:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        assert rows.size == self.k
        if external:
            self._ext = torch.from_numpy(rows).cuda()
            torch.cuda.synchronize()
            rc = self.lib.gfrs_decoder_solve(self.dec, self._ext.data_ptr(), None)
        else:
            dst = self.lib.gfrs_decoder_rows(self.dec)
            assert dst
            torch.cuda.synchronize()
            assert self.lib.gfrs_copy(dst, rows.ctypes.data, rows.nbytes) == OK, cc.err(self.lib)
            rc = self.lib.gfrs_decoder_solve(self.dec, None, None)
        assert rc == OK, cc.err(self.lib)
        return self.lib.gfrs_decoder_status(self.dec, None)

    def run_and_check(self, what, decoded: bool) -> None:
        assert self.lib.gfrs_decoder_run(self.dec, None) == OK, cc.err(self.lib)
        if decoded:
            for j, r in enumerate(self.outs):
                r.expect(self.data[j])
        self.arena.check(what)

    def close(self):
        self.lib.gfrs_decoder_destroy(self.dec)


@pytest.fixture
def decoder(lib):
    made = []

    def make(*args, **kw):
        made.append(DecoderSetup(lib, *args, **kw))
        return made[-1]

    yield make
    for d in made:
        d.close()


@pytest.mark.parametrize("k,p,e,engine", DECODERS, ids=lambda v: str(v))
def test_decoder_rebuilds_and_copies(decoder, lib, k, p, e, engine):
    """Two patterns of the same size on one decoder, the first through gfrs_decoder_rows, the second
    as an external rows_dev: out equals the data in every row (rebuilt and copied alike), the chunk
    rows and the guards are unchanged."""
    d = decoder(k, p, e, engine)
    assert lib.gfrs_decoder_engine(d.dec) == (engine or auto_engine(k, e))
    for t, external in enumerate((False, True)):
        rows, lost = pattern(k, p, e, [k, p, e], shift=t)
        d.load(rows)
        assert d.solve(rows, external) == 0
        d.run_and_check(f"pattern {t}: natives {lost} lost, survivors {rows.tolist()}", decoded=True)


def test_decoder_patterns_differ():
    """The two patterns test_decoder_rebuilds_and_copies solves lose different natives wherever the
    shape has more than one choice."""
    for k, p, e, _ in DECODERS:
        if e < k:
            assert pattern(k, p, e, [k, p, e])[1] != pattern(k, p, e, [k, p, e], shift=1)[1], (k, p, e)


def _bad_lists(k, p, e):
    rows, _ = pattern(k, p, e, [k, p, e, 3])
    dup, past, neg = rows.copy(), rows.copy(), rows.copy()
    dup[1] = dup[0]
    past[2] = k + p
    neg[0] = -1
    fewer, _ = pattern(k, p, e - 1, [k, p, e, 4])  # a valid list that loses e - 1 natives
    return {"duplicate id": dup, "id == n": past, "negative id": neg, "another number of lost natives": fewer}


@pytest.mark.parametrize("what", ["duplicate id", "id == n", "negative id", "another number of lost natives"])
def test_decoder_invalid_list_is_status_2_and_stores_nothing(decoder, what):
    k, p, e = 10, 4, 2
    d = decoder(k, p, e, AUTO)
    good, _ = pattern(k, p, e, [k, p, e, 0])
    d.load(good)
    assert d.solve(good) == 0
    d.run_and_check("good pattern first", decoded=True)
    d.load(good)  # outputs back at the fill value
    assert d.solve(_bad_lists(k, p, e)[what]) == 2
    d.run_and_check(f"run after a refused list ({what}) stores nothing", decoded=False)
    again, _ = pattern(k, p, e, [k, p, e, 1])
    d.load(again)
    assert d.solve(again, external=True) == 0
    d.run_and_check("good pattern after the refused one", decoded=True)


def test_decoder_singular_pattern_is_status_1_and_stores_nothing(decoder):
    """The reference Vandermonde (10, 4) cannot recover chunks {4, 5, 9, 11}
    (test_singular_census_matches_survey)."""
    k, p, e = 10, 4, 3
    d = decoder(k, p, e, AUTO, matrix="vandermonde")
    singular = np.array([13, 0, 1, 2, 3, 12, 6, 7, 8, 10], dtype=np.int32)
    d.load(singular)
    assert d.solve(singular) == 1
    d.run_and_check("run after a singular pattern stores nothing", decoded=False)
    good = np.array([0, 1, 2, 3, 10, 11, 6, 7, 8, 12], dtype=np.int32)  # natives 4, 5, 9 lost, parity 13 lost
    d.load(good)
    assert d.solve(good) == 0
    d.run_and_check("good pattern after the singular one", decoded=True)


# ---- 3. gfrs_update ----------------------------------------------------------------------------------
UPD_C = 4101


class UpdateSetup:
    """d changed rows (old, new or delta) and p parity rows in one arena, for one form."""

    def __init__(self, d, p, form, shift_row=False, ncols=UPD_C):
        self.d, self.p, self.form, self.c = d, p, form, ncols
        self.coeff = cc.noise([d, p, 11], p, d)
        self.coeff[0, 0] = 1
        self.old, self.new, self.par = (cc.noise([d, p, 12 + t], n, ncols) for t, n in enumerate((d, d, p)))
        self.delta = self.old ^ self.new
        self.arena = a = cc.DeviceArena(cc.arena_bytes(2 * d + p, ncols))
        self.first = [a.take(ncols, 1 if shift_row and t == d - 1 else 0) for t in range(d)]
        self.second = a.rows(d, ncols) if form != "delta" else None
        self.parity = a.rows(p, ncols)
        for t in range(d):
            self.first[t].put(self.delta[t] if form == "delta" else self.old[t])
            if self.second:
                self.second[t].put(self.new[t])
        for i in range(p):
            self.parity[i].put(self.par[i])

    def create(self, lib):
        u = ctypes.c_void_p()
        rc = lib.gfrs_update_create(ctypes.byref(u), 0, self.d, self.p, cc.coeff_bytes(self.coeff),
                                    cc.ptr_array([r.ptr for r in self.first]),
                                    cc.ptr_array([r.ptr for r in self.second]) if self.second else None,
                                    cc.ptr_array([r.ptr for r in self.parity]), int(self.form == "store_new"))
        assert rc == OK, cc.err(lib)
        return u

    def expect(self, col0, ncols):
        moved = gf.GF256.gemm(self.coeff, self.delta[:, col0: col0 + ncols]).astype(np.uint8)
        for i, r in enumerate(self.parity):
            r.expect(self.par[i, col0: col0 + ncols] ^ moved[i], col0)
        if self.form == "store_new":
            for t, r in enumerate(self.first):
                r.expect(self.new[t, col0: col0 + ncols], col0)


@pytest.mark.parametrize("reach", ["aligned", "odd_col0", "unaligned_row"])
@pytest.mark.parametrize("p", [1, 2, 3, 5])
@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7, 8, 17])
def test_update_every_width(lib, d, p, reach):
    """Each kernel instantiation d = 2..8 and a list of 17 (passes of 8, 8 and 1), in the pair, delta
    and store_new forms; the byte form through an odd col0 and through one unaligned row."""
    col0, ncols = (5, 4000) if reach == "odd_col0" else (0, UPD_C)
    for form in ("pairs", "delta", "store_new"):
        s = UpdateSetup(d, p, form, shift_row=reach == "unaligned_row")
        torch.cuda.synchronize()
        u = s.create(lib)
        try:
            assert lib.gfrs_update_run(u, col0, ncols, None) == OK, cc.err(lib)
            s.expect(col0, ncols)
            s.arena.check(f"d={d} p={p} {form} {reach}")
        finally:
            lib.gfrs_update_destroy(u)


@pytest.mark.parametrize("which", ["parity rows", "new row against old row"])
def test_update_window_rule_at_its_boundary(lib, which):
    """Rows that are views 112 bytes apart: a window of 112 columns does not overlap, runs and is
    exact; one of 113 is refused (GFRS_EINVAL) and writes nothing."""
    gap, d, p = 112, 1, 2
    coeff = cc.noise([gap, 1], p, d)
    arena = cc.DeviceArena(cc.arena_bytes(8, 4 * gap))
    block = arena.take(2 * gap)  # two views, 112 bytes apart, inside it
    close = [arena.at(block.off, gap), arena.at(block.off + gap, gap)]
    far = [arena.take(gap + 1) for _ in range(3)]
    if which == "parity rows":
        parity, old, new, store_new = close, far[0], far[1], 0
    else:
        parity, old, new, store_new = far[:2], close[0], close[1], 1
    vals = {id(r): cc.noise([gap, 2 + t], r.n) for t, r in enumerate([*parity, old, new])}
    for r in (*parity, old, new):
        r.put(vals[id(r)])
    torch.cuda.synchronize()
    u = ctypes.c_void_p()
    assert lib.gfrs_update_create(ctypes.byref(u), 0, d, p, cc.coeff_bytes(coeff), cc.ptr_array([old.ptr]),
                                  cc.ptr_array([new.ptr]), cc.ptr_array([r.ptr for r in parity]), store_new) == OK, cc.err(lib)
    try:
        assert lib.gfrs_update_run(u, 0, gap + 1, None) == EINVAL
        assert "overlap" in cc.err(lib)
        arena.check(f"{which}: a refused window of {gap + 1} writes nothing")
        assert lib.gfrs_update_run(u, 0, gap, None) == OK, cc.err(lib)
        delta = (vals[id(old)][:gap] ^ vals[id(new)][:gap])[None, :]
        moved = gf.GF256.gemm(coeff, delta).astype(np.uint8)
        for i, r in enumerate(parity):
            r.expect(vals[id(r)][:gap] ^ moved[i])
        if store_new:
            old.expect(vals[id(new)][:gap])
        arena.check(f"{which}: a window of {gap}")
    finally:
        lib.gfrs_update_destroy(u)


# ---- 4. host GEMM ------------------------------------------------------------------------------------
HOST_INPUTS = ["one_pinned", "separate_pinned", "pageable", "plus1"]


class HostSetup:
    """k input rows in host memory and m output rows that are views of a guard-filled pinned buffer,
    64-byte aligned and an odd number of 64-byte units apart."""

    def __init__(self, k, m, c, inputs="one_pinned", seed=1):
        self.k, self.m, self.c = k, m, c
        self.coeff, self.data, self.want = cc.gemm_case(k, m, c, seed)
        self.arena = cc.HostArena(cc.arena_bytes(k + m, c, 4096), pinned=inputs != "pageable")
        a, self.keep = self.arena, []
        if inputs == "one_pinned":
            # contiguous rows: a single 2-D run whose pitch equals the slice when C does
            block = a.take(k * c)
            self.ins = [cc.Row(a, block.off + j * c, c) for j in range(k)]
            self.in_ptrs = [r.ptr for r in self.ins]
        elif inputs == "separate_pinned":
            self.keep = [torch.from_numpy(np.array(self.data[j])).pin_memory() for j in range(k)]
            self.ins, self.in_ptrs = [], [t.data_ptr() for t in self.keep]
        else:
            self.ins = a.scattered(k, c, 4) if inputs == "pageable" else a.rows(k, c, shift=1)
            self.in_ptrs = [r.ptr for r in self.ins]
        for j, r in enumerate(self.ins):
            r.put(self.data[j])
        self.outs = a.pitched(m, c, (c + 63) // 64 * 64 + cc.PAD + 64, shift=64)
        self.out_ptrs = [r.ptr for r in self.outs]

    def check(self, what):
        for i, r in enumerate(self.outs):
            r.expect(self.want[i])
        self.arena.check(what)
        for j, t in enumerate(self.keep):
            assert np.array_equal(t.numpy(), self.data[j]), f"{what}: input row {j} changed"

    def run_c(self, lib, streams, slice_bytes, devices=(0,)):
        devs = (ctypes.c_int * len(devices))(*devices)
        rc = lib.gfrs_gemm_host(devs, len(devices), self.k, self.m, cc.coeff_bytes(self.coeff), cc.ptr_array(self.in_ptrs),
                                cc.ptr_array(self.out_ptrs), self.c, streams, slice_bytes)
        assert rc == OK, cc.err(lib)

    def run_py(self, streams, slice_bytes, devices=(0,), **opts):
        res = hip().gemm_host(list(devices), self.in_ptrs, self.out_ptrs, cc.coeff_bytes(self.coeff), self.c, streams,
                              slice_bytes, **opts)
        per = res["devices"]
        assert sum(s["bytes_h2d"] for s in per) == self.k * self.c
        assert sum(s["bytes_d2h"] for s in per) == self.m * self.c
        return per


def _host_cases():
    cases = []
    for sl in (256, 4096):
        for s in (1, 2, 3, 5):  # S = 5 is more lanes than the short lengths have slices
            lengths = [1, 255, 256, 257, 4097, 2 * s * sl - 1, 2 * s * sl, 2 * s * sl + 1]
            cases += [(10, 4, c, s, sl, "one_pinned") for c in lengths]
    for k, m in ((1, 1), (17, 3), (32, 20)):
        cases += [(k, m, c, 2, 256, inp) for c in (257, 4097) for inp in HOST_INPUTS]
    cases += [(10, 4, 4097, 3, 256, inp) for inp in HOST_INPUTS[1:]]
    cases += [(10, 4, 2 * 3 * 4096 + 1, 3, 4096, inp) for inp in HOST_INPUTS[1:]]
    return cases


@pytest.mark.parametrize("k,m,c,streams,slice_bytes,inputs", _host_cases())
def test_gemm_host_matches_oracle(lib, k, m, c, streams, slice_bytes, inputs):
    s = HostSetup(k, m, c, inputs)
    s.run_c(lib, streams, slice_bytes)
    s.check(f"gfrs_gemm_host k={k} m={m} C={c} S={streams} slice={slice_bytes} {inputs}")


@pytest.mark.parametrize("opts", [{"rect": False}, {"copy_streams": 0}, {"max_blocks": 3}, {"bytewise": True}, {}],
                         ids=lambda o: "-".join(f"{a}={v}" for a, v in o.items()) or "defaults")
@pytest.mark.parametrize("inputs", ["one_pinned", "plus1"])
def test_gemm_host_options_the_c_entry_does_not_expose(opts, inputs):
    k, m, c = 10, 4, 3 * 2 * 256 + 77
    s = HostSetup(k, m, c, inputs)
    per = s.run_py(3, 256, **opts)
    assert len(per) == 1 and per[0]["slices"] == (c + 255) // 256 and per[0]["lanes"] == 3
    s.check(f"hip().gemm_host {opts} {inputs}")


def test_gemm_host_zero_columns(lib):
    s = HostSetup(10, 4, 257)
    s.c = 0
    s.run_c(lib, 2, 256)
    s.arena.check("ncols == 0 writes nothing")


@pytest.mark.parametrize("c,first_empty", [(3 * 4096 + 5, False), (5000, True)])
def test_gemm_host_two_shards_on_one_device(lib, c, first_empty):
    """devices [0, 0]: shard boundaries are multiples of 4 KiB with the remainder last, so at
    C = 5000 the first shard has no columns at all."""
    k, m = 10, 4
    s = HostSetup(k, m, c)
    s.run_c(lib, 2, 256, devices=(0, 0))
    s.check(f"gfrs_gemm_host on [0, 0], C={c}")
    s = HostSetup(k, m, c, "pageable")
    per = s.run_py(2, 256, devices=(0, 0))
    assert len(per) == 2 and (per[0]["bytes_h2d"] == 0) == first_empty
    s.check(f"hip().gemm_host on [0, 0], C={c}")
