"""The GEMM engines on inputs a random draw never produces (tests/engine_cases.py; the cases are
held to their conditions by tests/test_engine_cases.py), bit-exact against the numpy oracle (GPU).

A. Count ladder: the matrix-core engines (FP4 in its v1 / A-resident / tile-major forms and its
   batched launch, int8, GF(2^16) FP4 with its K passes) on columns whose saturated output bit counts
   0, w, 2w, ... w k and, every second lap, one less: the whole range of the integer count behind the
   parity, up to the design bound 8 k = 2048 at k = 256.
B. Structured matrices on every engine of both fields: zero, null rows and columns, selections
   (the output must be the input row byte for byte), all ones (a plain XOR), a third zeros and a
   third ones. Outputs are filled with 0xAB first, so a row the kernel does not store shows.
C. Every coefficient of the field on one input row at a time: a wrong byte names the coefficient,
   the value and the input row. Host-built and device-built operands must give identical bytes.

The reference is ``GF256.gemm`` for the GF(2^8) ladder. The GF(2^16) ladder and the structured
cases of both fields use ``engine_cases.oracle_gemm``: the same loop as ``gf.field(w).gemm`` over
the same ``mul_table`` rows, each computed once per distinct coefficient instead of once per matrix
entry (12,000 tables of 65,536 entries at (300, 40)); the CPU module pins it equal to ``F.gemm`` on
random matrices and on a whole ladder shape. The every-coefficient cases use the oracle's ``mul`` and
``matmul``. None of them touches the kernels or their table builders.
"""
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

import engine_cases as ec
from gpu_rscode_amd.gf import GF256
from gpu_rscode_amd.models import alloc_rows
from gpu_rscode_amd.ops import Gemm16Plan, GemmPlan
from gpu_rscode_amd.utils.tune import with_tune

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
COPY_FILL = 0x44


def _hip():
    from gpu_rscode_amd._native import hip

    h = hip()
    assert h.device_count() > 0, "HIP module loaded but sees no device"
    return h


def _as_bytes(sym: np.ndarray) -> np.ndarray:
    """Symbol rows as the byte rows the kernels read (GF(2^16): little-endian pairs)."""
    a = np.ascontiguousarray(sym)
    return a if a.dtype == np.uint8 else a.astype("<u2").view(np.uint8).reshape(a.shape[0], -1)


def _upload(host_u8: np.ndarray) -> torch.Tensor:
    t = alloc_rows(host_u8.shape[0], host_u8.shape[1], "cuda")
    t.copy_(torch.from_numpy(np.array(host_u8)))
    return t


def _strided(batch: int, rows: int, ncols: int, fill: int) -> torch.Tensor:
    """[batch, rows, ncols] over one allocation, row pitch a multiple of 256: stripes at fixed strides."""
    pitch = (ncols + 255) // 256 * 256
    base = torch.full((batch * rows * pitch,), fill, dtype=torch.uint8, device="cuda")
    return base.as_strided((batch, rows, ncols), (rows * pitch, pitch, 1))


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    i, c = (int(v) for v in bad[0])
    return f"{bad.shape[0]} wrong symbols, first at row {i}, column {c}: got {int(got[i, c]):#x}, want {int(want[i, c]):#x}"


def _check_out(got, want, what=""):
    assert got.shape == want.shape
    assert np.array_equal(got, want), (what, _first_diff(got, want))


def _copy_rows(k: int, ncols: int, copies: bool):
    """Destinations for the odd input rows (the even ones have none), or nothing."""
    if not copies:
        return None, None
    dst = alloc_rows(k, ncols, "cuda", fill=COPY_FILL)
    return dst, [dst[j] if j % 2 else None for j in range(k)]


def _check_copies(dst, in_bytes):
    if dst is None:
        return
    c = dst.cpu().numpy()
    for j in range(in_bytes.shape[0]):
        want = in_bytes[j] if j % 2 else np.full(in_bytes.shape[1], COPY_FILL, np.uint8)
        assert np.array_equal(c[j], want), ("copy of input row", j)


# ---- launchers: one engine each, returning the output symbols ---------------------------------------
def _gemm8(coeff, data, *, engine="valu", run_kw=None, copies=False, scattered=False, offset=0, fill=0xAB,
           form=None, seed=0):
    """One GF(2^8) launch of ``engine`` on byte rows ``data``: uniform rows of one allocation, or
    separately allocated rows in a shuffled allocation order (``scattered``), or rows ``offset``
    bytes off alignment (the byte kernel). Fused copies are checked here. ``form``: the FP4 form the
    plan must report."""
    _hip()
    k, ncols = data.shape
    m = coeff.shape[0]
    if offset:
        buf = torch.from_numpy(np.concatenate([np.zeros((k, offset), np.uint8), data], axis=1)).cuda()
        inputs = [buf[j, offset:] for j in range(k)]
        out = torch.full((m, ncols), fill, dtype=torch.uint8, device="cuda")
    else:
        dev = _upload(data)
        inputs = dev
        if scattered:
            rows = [None] * k
            for j in np.random.default_rng(seed).permutation(k):
                rows[j] = dev[j].clone()
            inputs = rows
        out = alloc_rows(m, ncols, "cuda", fill=fill)
    dst, cps = _copy_rows(k, ncols, copies)
    plan = GemmPlan(inputs, out, np.asarray(coeff, dtype=np.uint8), copies=cps, engine=engine)
    assert plan.engine == engine
    assert plan.bytewise == bool(offset)
    if form is not None:
        assert plan.fp4_form == form, (plan.fp4_form, form)
        if not scattered and not copies and k > 2:
            assert plan.in_stride != 0
    plan.run(**(run_kw or {}))
    torch.cuda.synchronize()
    _check_copies(dst, data)
    return out.cpu().numpy()


def _gemm8_batched(coeff, data, *, engine, copies=False, fill=0xAB):
    """One batched GF(2^8) launch on [B, k, C] stripes at fixed strides; outputs and copy
    destinations share one allocation per stripe so that both sit at the output stride."""
    _hip()
    B, k, ncols = data.shape
    m = coeff.shape[0]
    x = _strided(B, k, ncols, 0)
    x.copy_(torch.from_numpy(np.array(data)))
    both = _strided(B, m + k, ncols, fill)
    out, dst = both[:, :m], both[:, m:]
    cps = [[dst[b, j] if j % 2 else None for j in range(k)] for b in range(B)] if copies else None
    plan = GemmPlan(x, out, np.asarray(coeff, dtype=np.uint8), copies=cps, engine=engine)
    assert plan.batch == B and plan.engine == engine
    if engine == "mfma":  # the batched launch has one form: the A-resident kernel, grid over stripes
        assert plan.fp4_form is None and plan.in_bstride is not None and _hip().fp4_batched_supported(k, m, 8)
    plan.run()
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    for b in range(B):
        for j in range(k):
            want = data[b, j] if copies and j % 2 else np.full(ncols, fill, np.uint8)
            assert np.array_equal(d[b, j], want), ("copy", b, j)
    return out.cpu().numpy()


def _gemm16(coeff, data_u8, *, engine, copies=False, offset=0, fill=0xAB, device_sel=False):
    """One GF(2^16) launch of ``engine`` on byte rows; returns the output symbols. ``offset`` = 2:
    rows off 16-byte alignment (the symbol kernel). ``device_sel``: the matrix-core operand is built
    on the device from the rows of a shuffled device matrix picked by an index list."""
    _hip()
    k, nbytes = data_u8.shape
    m = coeff.shape[0]
    if offset:
        flat = torch.zeros(k * nbytes + offset, dtype=torch.uint8, device="cuda")
        x = flat[offset:].view(k, nbytes)
        x.copy_(torch.from_numpy(np.array(data_u8)))
        inputs = [x[j] for j in range(k)]
        out = torch.full((m, nbytes), fill, dtype=torch.uint8, device="cuda")
    else:
        inputs = _upload(data_u8)
        out = alloc_rows(m, nbytes, "cuda", fill=fill)
    dst, cps = _copy_rows(k, nbytes, copies)
    if device_sel:
        plan = Gemm16Plan(inputs, out, copies=cps, device_tables=True, engine=engine)
        perm = np.random.default_rng(m).permutation(m)
        big = np.zeros((m, coeff.shape[1]), dtype="<u2")
        big[perm] = coeff  # row perm[i] of the device matrix is coefficient row i
        plan.set_device_coeff(torch.from_numpy(big.view(np.int16)).cuda(),
                              torch.from_numpy(perm.astype(np.int32)).cuda())
    else:
        plan = Gemm16Plan(inputs, out, coeff, copies=cps, engine=engine)
    assert plan.engine == engine
    assert plan.symwise == bool(offset)
    plan.run()
    torch.cuda.synchronize()
    _check_copies(dst, data_u8)
    return out.cpu().numpy().view("<u2")


def _gemm16_batched(coeff, data_u8, *, engine, copies=False, fill=0xAB):
    _hip()
    B, k, nbytes = data_u8.shape
    m = coeff.shape[0]
    x = _strided(B, k, nbytes, 0)
    x.copy_(torch.from_numpy(np.array(data_u8)))
    both = _strided(B, m + k, nbytes, fill)
    out, dst = both[:, :m], both[:, m:]
    cps = [[dst[b, j] if j % 2 else None for j in range(k)] for b in range(B)] if copies else None
    plan = Gemm16Plan(x, out, coeff, copies=cps, engine=engine)
    assert plan.batch == B and plan.engine == engine
    if engine == "mfma":
        assert plan.in_bstride is not None
    plan.run()
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    for b in range(B):
        for j in range(k):
            want = data_u8[b, j] if copies and j % 2 else np.full(nbytes, fill, np.uint8)
            assert np.array_equal(d[b, j], want), ("copy", b, j)
    return np.ascontiguousarray(out.cpu().numpy()).view("<u2")


def _in_subprocess(call: str, **tune):
    """``test_gpu_engines.<call>`` in a fresh process whose GFRS_TUNE also holds ``tune`` (knobs
    the native code reads once per process)."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_gpu_engines as t; t.{call}; "
            "print('ENGINE-OK')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=with_tune(**tune))
    assert r.returncode == 0 and "ENGINE-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- A. count ladder --------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _ladder(w: int, k: int, m: int, first: int = 0):
    """(coeff, data, want) of one ladder shape, computed once and shared (read-only)."""
    F = ec.field(w)
    coeff, data = ec.ladder_coeff(w, m, k, first), ec.ladder_data(w, k)
    # (w = 16: the oracle's gemm with one multiply table per distinct coefficient, not 12,000)
    want = GF256.gemm(coeff, data) if w == 8 else ec.oracle_gemm(F, coeff, data)
    for a in (coeff, data, want):
        a.setflags(write=False)
    return coeff, data, want


@lru_cache(maxsize=None)
def _ladder_batch(w: int, k: int, m: int, B: int):
    """Stripe b is the ladder rotated by 37 b symbols, so the stripes differ column by column."""
    coeff, data, want = _ladder(w, k, m)
    return coeff, np.stack([np.roll(data, 37 * b, axis=1) for b in range(B)]), \
        np.stack([np.roll(want, 37 * b, axis=1) for b in range(B)])


def _check_ladder(w, k, got, want, what="", shift=0):
    """Exact comparison; a wrong symbol is reported with the count its column's saturated bit reached."""
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    if bad.size:
        i, c = (int(v) for v in bad[0])
        t, odd = ec.ladder_heights(k)
        t, odd = np.roll(t, shift), np.roll(odd, shift)
        cols = np.unique(bad[:, 1])
        lo, hi = (int(w * t[cols].min()), int(w * t[cols].max()))
        raise AssertionError(f"{what}: {bad.shape[0]} wrong symbols at counts {lo}..{hi}; first: output row {i}, "
                             f"column {c} (count {int(w * t[c] - (odd[c] and t[c] >= 1))}): got {int(got[i, c]):#x}, "
                             f"want {int(want[i, c]):#x}")


def _fp4_ladder(k, m, variant, form):
    coeff, data, want = _ladder(8, k, m)
    sc = variant == "scattered_copies"
    got = _gemm8(coeff, data, engine="mfma", scattered=sc, copies=sc, fill=0x5A, form=form, seed=k + m)
    _check_ladder(8, k, got, want, (form, k, m))


# (k, m, form with uniform rows, form with scattered rows + fused copies): fp4_route's choice
_FP4_ROUTED = [(128, 8, "v1", "v1"), (100, 17, "v1", "v1"), (256, 40, "v1", "v1"), (128, 16, "ar", "ar"),
               (128, 32, "ar", "tm"), (128, 20, "tm", "tm"), (128, 26, "tm", "tm")]


@pytest.mark.parametrize("variant", ["uniform", "scattered_copies"])
@pytest.mark.parametrize("k,m,form_plain,form_copy", _FP4_ROUTED)
def test_ladder_fp4_routed_forms(k, m, form_plain, form_copy, variant):
    """Every FP4 form on the shapes it is routed to, over the whole count range: 8 k = 1024 at
    k = 128 and, at (256, 40), the design bound 2048 itself. 16 laps of 256-column chunks and a
    ragged rest on the v_perm tables."""
    _fp4_ladder(k, m, variant, form_plain if variant == "uniform" else form_copy)


@pytest.mark.parametrize("variant", ["uniform", "scattered_copies"])
@pytest.mark.parametrize("form", ["v1", "ar", "tm"])
def test_ladder_fp4_forced_forms(form, variant, monkeypatch):
    """GFRS_TUNE=fp4=v1 / ar / tm on (128, 24), which each of them is built for."""
    monkeypatch.setenv("GFRS_TUNE", f"fp4={form}")
    _fp4_ladder(128, 24, variant, form)


@pytest.mark.parametrize("k,m,first", [(128, 32, 0)] + [(255, 1, b) for b in range(8)])
def test_ladder_int8_mfma(k, m, first):
    """The int8 MFMA engine; its one-row shape takes each saturating coefficient in turn."""
    coeff, data, want = _ladder(8, k, m, first)
    _check_ladder(8, k, _gemm8(coeff, data, engine="mfma_i8", fill=0x5A), want, (k, m, first))


@pytest.mark.parametrize("engine", ["valu", "lut"])
def test_ladder_control_engines(engine):
    """The same case on engines that count nothing (v_perm, LDS tables): a control."""
    coeff, data, want = _ladder(8, 128, 32)
    _check_ladder(8, 128, _gemm8(coeff, data, engine=engine, fill=0x5A), want, engine)


def run_ladder_fp4_batched():
    coeff, data, want = _ladder_batch(8, 128, 32, 3)
    got = _gemm8_batched(coeff, data, engine="mfma", fill=0x5A)
    for b in range(3):
        _check_ladder(8, 128, got[b], want[b], ("stripe", b), shift=37 * b)


def test_ladder_fp4_batched():
    """The batched FP4 launch (A-resident kernel, grid over stripes) on a [3, 128, ...] tensor."""
    run_ladder_fp4_batched()


@pytest.mark.parametrize("knobs", [("0", "0"), ("0", "1000000000000"), ("1000000000000", "0")])
def test_ladder_fp4_batched_remainder_kernels(knobs):
    """The same launch with every batched v_perm kernel in turn under its ragged rest (vec at its
    widest tile, narrowed tile, k-split). Subprocess: the thresholds are read once."""
    _in_subprocess("run_ladder_fp4_batched()", ksplit_lanes=knobs[0], short_lanes=knobs[1])


# GF(2^16): (300, 40) two M-tile groups per block and two K passes, so the ladder crosses the pass
# boundary; (300, 35) one group, one pass, count 4800
@pytest.mark.parametrize("k,m,copies", [(300, 40, False), (300, 35, False), (17, 20, False), (64, 16, True)])
def test_ladder16_fp4(k, m, copies):
    coeff, data, want = _ladder(16, k, m)
    got = _gemm16(coeff, _as_bytes(data), engine="mfma", copies=copies, fill=0x5A)
    _check_ladder(16, k, got, want, (k, m))


def test_ladder16_fp4_batched():
    coeff, data, want = _ladder_batch(16, 64, 16, 3)
    got = _gemm16_batched(coeff, np.stack([_as_bytes(d) for d in data]), engine="mfma", fill=0x5A)
    for b in range(3):
        _check_ladder(16, 64, got[b], want[b], ("stripe", b), shift=37 * b)


def test_ladder16_control_engine():
    coeff, data, want = _ladder(16, 300, 40)
    _check_ladder(16, 300, _gemm16(coeff, _as_bytes(data), engine="valu16", fill=0x5A), want, "valu16")


# ---- B. structured matrices -------------------------------------------------------------------------
ENGINES8, ENGINES16, BATCH = ec.ENGINES8, ec.ENGINES16, ec.BATCH  # shapes and tiles: engine_cases.py


@lru_cache(maxsize=None)
def _struct_case(w: int, engine: str, name: str):
    """(coeff, data, want) of one structured case on one engine's shape; batched engines get
    [BATCH, k, C] data. ``want`` is the oracle's, and where the case says what the output is
    without field arithmetic (zero, selection, XOR) that must agree."""
    F = ec.field(w)
    k, m, ncols, tile = ec.engines(w)[engine]
    seed = ec.engine_seed(w, engine)
    coeff = ec.structured(name, w, m, k, tile, seed)
    batched = engine.startswith("batched")
    data = ec.random_symbols(w, k * (BATCH if batched else 1), ncols, seed + 1)
    stripes = data.reshape(BATCH, k, ncols) if batched else data.reshape(1, k, ncols)
    want = []
    for x in stripes:
        ref = ec.oracle_gemm(F, coeff, x)
        direct = ec.structured_expect(name, w, m, k, seed, x)
        if direct is not None:
            assert np.array_equal(ref, direct)
        want.append(ref)
    want = np.stack(want)
    if not batched:
        stripes, want = stripes[0], want[0]
    stripes.setflags(write=False)
    want.setflags(write=False)
    return coeff, stripes, want


def run_struct8(engine: str, name: str):
    coeff, data, want = _struct_case(8, engine, name)
    if engine == "vec":
        got = _gemm8(coeff, data, engine="valu", run_kw=dict(vec=2, pf=2, nt=True), copies=True)
    elif engine == "valu_wide":
        got = _gemm8(coeff, data, engine="valu", copies=True)
    elif engine.startswith("rows"):
        pf = int(engine.rsplit("pf", 1)[1])
        got = _gemm8(coeff, data, engine="valu", run_kw=dict(vec=1, pf=pf, nt=True), copies=True)
    elif engine == "byte":
        got = _gemm8(coeff, data, engine="valu", offset=3, copies=True)
    elif engine == "lut":
        got = _gemm8(coeff, data, engine="lut", copies=True)
    elif engine == "mfma_i8":
        got = _gemm8(coeff, data, engine="mfma_i8")
    elif engine.startswith("mfma_"):
        got = _gemm8(coeff, data, engine="mfma", scattered=True, copies=True, form=engine[5:], seed=7)
    elif engine == "batched_valu":
        got = _gemm8_batched(coeff, data, engine="valu", copies=True)
    else:
        got = _gemm8_batched(coeff, data, engine="mfma", copies=True)
    _check_out(got, want, (engine, name))


@pytest.mark.parametrize("name", ec.STRUCTURED)
@pytest.mark.parametrize("engine", sorted(ENGINES8))
def test_structured_gf256(engine, name):
    """Every GF(2^8) engine on every structured matrix, fused copies wherever the engine takes them
    (destination-less rows keep their fill); outputs start as 0xAB."""
    run_struct8(engine, name)


def run_struct16(engine: str, name: str):
    key = "valu16_g2" if engine == "valu16_g2_forced_g1" else engine
    coeff, data, want = _struct_case(16, key, name)
    if engine.startswith("batched"):
        got = _gemm16_batched(coeff, np.stack([_as_bytes(d) for d in data]),
                              engine="mfma" if engine == "batched_mfma" else "valu16", copies=True)
    elif engine == "sym":
        got = _gemm16(coeff, _as_bytes(data), engine="valu16", offset=2, copies=True)
    elif engine == "mfma":
        got = _gemm16(coeff, _as_bytes(data), engine="mfma", copies=True)
    else:
        got = _gemm16(coeff, _as_bytes(data), engine="valu16", copies=True)
    _check_out(got, want, (engine, name))


def run_struct8_all(engine: str):
    for name in ec.STRUCTURED:
        run_struct8(engine, name)


@pytest.mark.parametrize("engine", sorted(e for e in ENGINES8 if e.startswith("rows")))
def test_structured_gf256_rows_throughput_form(engine):
    """Launches this small take the latency form of the rows-in-flight kernel
    (gf_gemm_rows_lat_kernel); GFRS_TUNE=rows_lat_groups=0 sends the same cases through the
    throughput form (gf_gemm_rows_kernel). One subprocess per kernel instance, the five cases in
    turn (a failure names engine and case): the threshold is read once."""
    _in_subprocess(f"run_struct8_all({engine!r})", rows_lat_groups=0)


@pytest.mark.parametrize("name", ec.STRUCTURED)
@pytest.mark.parametrize("engine", sorted(ENGINES16))
def test_structured_gf65536(engine, name):
    """Every GF(2^16) engine on every structured matrix: the v_perm vector kernel with one and two
    16-byte groups per lane, the symbol kernel on rows 2 bytes off alignment, the FP4 matrix cores,
    and both batched forms."""
    run_struct16(engine, name)


@pytest.mark.parametrize("name", ec.STRUCTURED)
def test_structured_gf65536_long_rows_one_group_per_lane(name):
    """The long-row shape with GFRS_TUNE=gf16_vec_g=1: the vector kernel's one-group form at the
    4-row tile. Subprocess: the knob is read once."""
    _in_subprocess(f"run_struct16('valu16_g2_forced_g1', {name!r})", gf16_vec_g=1)


# ---- C. every coefficient, one input row at a time --------------------------------------------------
def _check_every(w: int, got: np.ndarray, rows=None):
    """``got`` against the whole expected output; a wrong impulse column is reported as the
    (coefficient, value, input row) it belongs to."""
    want = ec.every_expect(w)
    coeff = ec.every_coeff(w)[0]
    if rows is not None:
        want, coeff = want[rows], coeff[rows]
    n, per = ec.every_dims(w)
    bad = np.argwhere(got != want)
    if bad.size:
        i, c = (int(v) for v in bad[0])
        where = (f"coefficient {int(coeff[i, c // per]):#x} on input row {c // per}, impulse {c % per}"
                 if c < n * per else f"random column {c - n * per}")
        raise AssertionError(f"{bad.shape[0]} wrong symbols; first: output row {i}, {where}: "
                             f"got {int(got[i, c]):#x}, want {int(want[i, c]):#x}")


@pytest.mark.parametrize("engine", ["vec", "byte", "lut", "mfma_i8", "mfma"])
def test_every_gf256_coefficient(engine):
    """coeff = arange(256) as 16 x 16 on impulse columns: the output spells out the 256 x 256 product
    table through each engine's own tables (v_perm records, LDS nibble tables, bit-matrices)."""
    coeff, data, _ = ec.every_coeff(8)
    if engine == "vec":
        got = _gemm8(coeff, data, engine="valu", run_kw=dict(vec=1, pf=2, nt=True))
    elif engine == "byte":
        got = _gemm8(coeff, data, engine="valu", offset=3)
    elif engine == "mfma":
        got = _gemm8(coeff, data, engine="mfma", form="v1")
    else:
        got = _gemm8(coeff, data, engine=engine)
    _check_every(8, got)


def run_every8_rows(block: int):
    coeff, data, _ = ec.every_coeff(8)
    rows = slice(4 * block, 4 * block + 4)
    got = _gemm8(coeff[rows], data, engine="valu", run_kw=dict(vec=1, pf=0, nt=True))
    _check_every(8, got, rows)


@pytest.mark.parametrize("block", range(4))
def test_every_gf256_coefficient_rows_in_flight(block):
    """The rows-in-flight kernel (k = 16, 4-row tiles; its latency form at this size): one launch
    per block of four matrix rows."""
    run_every8_rows(block)


def run_every8_rows_all():
    for block in range(4):
        run_every8_rows(block)


def test_every_gf256_coefficient_rows_throughput_form():
    """The same four launches on the kernel's throughput form (GFRS_TUNE=rows_lat_groups=0, read
    once: a subprocess)."""
    _in_subprocess("run_every8_rows_all()", rows_lat_groups=0)


def test_every_gf256_coefficient_device_built_operands():
    """The v_perm records and the FP4 bit-matrix built on the device (perm_tables, fp4_bitmat_sel
    with a row index list into a shuffled device matrix): the same bytes as the host-built plan."""
    h = _hip()
    coeff, data, _ = ec.every_coeff(8)
    host_built = _gemm8(coeff, data, engine="mfma", form="v1")
    k, ncols = data.shape
    m = coeff.shape[0]
    dev = _upload(data)
    out = alloc_rows(m, ncols, "cuda", fill=0xAB)
    plan = GemmPlan(dev, out, device_tables=True, engine="mfma")
    assert plan.engine == "mfma" and plan.fp4_form == "v1"
    c8 = np.asarray(coeff, dtype=np.uint8)
    perm = np.random.default_rng(8).permutation(m)
    big = np.zeros_like(c8)
    big[perm] = c8
    cdev = torch.from_numpy(c8).cuda()
    h.perm_tables(cdev.data_ptr(), m, k, plan.desc.data_ptr(), plan.m_pad, torch.cuda.current_stream().cuda_stream)
    plan.set_device_coeff(torch.from_numpy(big).cuda(), torch.from_numpy(perm.astype(np.int32)).cuda())
    plan.run()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _check_every(8, got)
    assert np.array_equal(got, host_built)
    # the device-built records themselves, against the host builder's
    from gpu_rscode_amd.ops.gemm import perm_tables_from_coeff
    tabs = plan.table_view().cpu().numpy()[:, :m, :].view(np.uint32)
    assert np.array_equal(tabs, np.transpose(perm_tables_from_coeff(c8), (1, 0, 2)))


@pytest.mark.parametrize("engine", ["valu16", "sym", "mfma", "mfma_device"])
def test_every_gf65536_coefficient(engine):
    """coeff = arange(65536) as 256 x 256 on the 16 basis symbols of every input row: the output
    determines every coefficient's whole 16 x 16 map, through the byte-map quadruples (valu16, the
    symbol kernel) and the bit-matrices (mfma; mfma_device: built on the device through a row index
    list into a shuffled device matrix, as the device-built decode plans do)."""
    coeff, data, _ = ec.every_coeff(16)
    if engine == "sym":
        got = _gemm16(coeff, _as_bytes(data), engine="valu16", offset=2)
    elif engine == "mfma_device":
        got = _gemm16(coeff, _as_bytes(data), engine="mfma", device_sel=True)
        assert np.array_equal(got, _gemm16(coeff, _as_bytes(data), engine="mfma"))  # host-built: identical bytes
    else:
        got = _gemm16(coeff, _as_bytes(data), engine=engine)
    _check_every(16, got)
