"""The GEMM engines at the edges of their launch arithmetic (tests/geometry_cases.py; the cases are
held to their classes by tests/test_geometry_cases.py), bit-exact against the numpy oracle (GPU).

Every input, output and copy destination is a row of one guard-filled arena (tests/capi_cases.py)
with at least 256 guard bytes behind it; outputs and copy destinations start as 0x5A. After the
launch the whole arena is compared with a host image that holds the oracle's columns of the window
in the outputs, the inputs' same columns in the copy rows that have a destination, and what was
there before everywhere else: a tail rounded up to its 16-byte store, a padding block that works, a
skipped lap, a remainder at the wrong column or a window start rounded down all show, as bytes past
a row's end, bytes of the row outside the window, or window bytes still at their fill.

T. tail ladder: every tail residue behind 248 (and 249) groups, the tail lanes split over two blocks;
B. block and grid edges: 1 .. 16 * 256 + 1 lane items on one and on several output tiles;
S. capped grids (max_blocks) with a ragged last lap that holds the tail lanes;
W. windows [col0, col0 + n) on and off every engine's grid, and the kernel each falls to;
L. chunks per persistent block of the matrix-core forms, at the default slots and with one slot;
Q. the batched launches, three stripes with guard bytes between them.

One parametrised case is one engine and one family. Kernels reached only through a GFRS_TUNE key
the native code reads once (rows throughput form, the wide vec kernel, the narrowed tile, two
GF(2^16) groups per lane on short rows, forced FP4 forms, one-slot persistent grids) run in one
child process per knob setting (two settings: one per family), one child at a time.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import capi_cases as cc
import geometry_cases as gc
from gpu_rscode_amd.ops import Gemm16Plan, GemmPlan
from gpu_rscode_amd.utils.tune import with_tune

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
ENGINE_ARG = {"valu": "valu", "lut": "lut", "i8": "mfma_i8", "fp4": "mfma", "valu16": "valu16", "mfma16": "mfma"}


def _hip():
    from gpu_rscode_amd._native import hip

    h = hip()
    assert h.device_count() > 0, "HIP module loaded but sees no device"
    return h


class Arena(cc.DeviceArena):
    """A device arena whose rows are uploaded in one copy: ``put`` fills the host image only, and
    :meth:`upload` sends the image before the launch (one copy each way per case)."""

    def _store(self, off, host):
        pass

    def upload(self):
        self.buf.copy_(torch.from_numpy(self.image))


def gpu_launch(s: gc.Setup) -> None:
    """One plan over the arena's rows and one ``run`` of the case's window on the engine under test."""
    e, c, a = s.e, s.c, s.arena
    a.upload()
    view = lambda rows: [a.tensor(r) for r in rows]  # noqa: E731
    B = e.batch
    ins, outs = [view(st) for st in s.ins], [view(st) for st in s.outs]
    cps = None if s.copies is None else [[a.tensor(r) if r is not None else None for r in st] for st in s.copies]
    if B == 1:
        ins, outs, cps = ins[0], outs[0], None if cps is None else cps[0]
    if e.w == 16:
        plan = Gemm16Plan(ins, outs, s.coeff, copies=cps, engine=ENGINE_ARG[e.kind])
        assert plan.symwise == (e.shift % 16 != 0)
        if B > 1 and e.kind == "mfma16":
            assert plan.in_bstride is not None
    else:
        plan = GemmPlan(ins, outs, s.coeff.astype(np.uint8), copies=cps, engine=ENGINE_ARG[e.kind])
        assert plan.bytewise == (e.shift % 16 != 0)
        if e.kind == "fp4" and B == 1 and e.form is not None:
            assert plan.fp4_form == e.form, (plan.fp4_form, e.form)
            if s.layout == "uniform" and s.copies is None:
                assert plan.in_stride != 0
        if e.kind == "fp4" and B > 1:
            assert plan.in_bstride is not None and _hip().fp4_batched_supported(c.k, c.m, 8)
    assert plan.engine == ENGINE_ARG[e.kind] and plan.batch == B and plan.ncols == c.nrow
    kw = dict(col0=c.col0, ncols=c.n)
    if c.max_blocks:
        kw["max_blocks"] = c.max_blocks
    if e.cfg is not None and e.w == 8:
        kw.update(vec=e.cfg[0], pf=e.cfg[1], nt=True)
    plan.run(**kw)


def run_sweep(name: str, family: str) -> list:
    _hip()
    return gc.sweep(name, family, gpu_launch, Arena)


IN_PROCESS = [(n, f) for n, e in gc.ENGINES.items() if not e.tune for f in e.families]


@pytest.mark.parametrize("name,family", IN_PROCESS, ids=[f"{n}-{f}" for n, f in IN_PROCESS])
def test_geometry(name, family):
    """Every case of one engine and one family, on uniform and scattered rows with fused copies
    (and without, where the kernel has an instantiation of its own for that)."""
    failures = run_sweep(name, family)
    assert not failures, f"{len(failures)} cases failed; first: {failures[0]}"


def run_child(sweeps) -> None:
    """The child's side: its sweeps in turn, one line per failed case and a final marker."""
    total = 0
    for name, family in sweeps:
        for line in run_sweep(name, family):
            total += 1
            print("GEOMETRY-FAIL", line, flush=True)
    print("GEOMETRY-DONE", total, flush=True)


CHILDREN = gc.child_units()


def _child_id(unit):
    setting, sweeps = unit
    fams = "".join(sorted({f for _, f in sweeps}))
    return ",".join(f"{a}={v}" for a, v in setting) + (f"-{fams}" if setting in gc.SPLIT_BY_FAMILY else "")


@pytest.mark.parametrize("unit", CHILDREN, ids=_child_id)
def test_geometry_under_a_knob_read_once(unit):
    """All sweeps of one GFRS_TUNE setting in one fresh process (the native code reads the key once);
    the two settings of geometry_cases.SPLIT_BY_FAMILY have one child per family. Measured on an
    MI355X beside tests/test_gpu_engines.py (slowest case 3.89 s): fp4_free_cus 4.40 s, which holds
    family L only and so stays one child; every other child 2.4 to 3.1 s."""
    setting, sweeps = unit
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_geometry as t; "
            f"t.run_child({sweeps!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=with_tune(**dict(setting)))
    failed = [ln for ln in r.stdout.splitlines() if ln.startswith("GEOMETRY-FAIL")]
    assert r.returncode == 0 and "GEOMETRY-DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert failed == [] and r.stdout.rstrip().endswith("GEOMETRY-DONE 0"), failed[:3]


def test_fp4_router_mirror_is_the_native_router():
    """The mirror's fp4_route against the native one wherever a case list depends on it."""
    h = _hip()
    for k in (32, 100, 112, 113, 128, 129, 256):
        for m in range(1, 41):
            for copies in (False, True):
                assert gc.fp4_route(k, m, copies) == h.fp4_route(k, m, copies, 8), (k, m, copies)


@pytest.mark.parametrize("name", ["valu16_g1", "sym", "mfma", "batched_valu16", "batched_mfma"])
def test_gf65536_refuses_odd_windows_and_writes_nothing(name):
    e = gc.ENGINES[name]
    c = gc.cases(name, "W")[0]
    for col0, n in ((1, c.nrow - 1), (0, c.nrow - 1), (3, 15), (2, 17)):
        s = gc.Setup(Arena, e, gc.Case("W", c.k, c.m, c.nrow, col0, n), "uniform", e.copies[0])
        with pytest.raises(ValueError):
            gpu_launch(s)
        assert s.check() is None, f"{name}: refused window [{col0}, {col0 + n}) wrote something"
