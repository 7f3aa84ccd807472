"""The route of the device repair solve, on the CPU: ``gf.repair_coeff_oracle`` (the systematic solve
and the parity product, the plain numpy form of csrc/kernels/gf_repair_solve.hip) against the host
path's ``G[erased] . inv(G[survivors])``, exactly; and ``device_solve=True`` on CPU tensors, which
takes the CPU path. tests/test_gpu_repair_solve.py runs the kernel on the same cases."""
import itertools

import numpy as np
import pytest
import torch

import repair_solve_cases as rc
import solver_cases as sc
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd.models.rs import UnrecoverableError


def _agree(code, survivors, erased):
    want = rc.host_coeff(code, survivors, erased)
    assert want is not None, (code, erased)
    got = gf.repair_coeff_oracle(rc.codec(*code).G, survivors, erased)
    assert got.dtype == np.uint8 and got.shape == (len(erased), code[0])
    assert np.array_equal(got, want), (code, survivors, erased)


@pytest.mark.parametrize("code", [(10, 14, "cauchy"), (4, 8, "cauchy")], ids=lambda c: f"{c[0]}-{c[1]}")
def test_oracle_equals_the_inverse_for_every_pattern(code):
    """Every pattern of 1..p erasures with its default survivors: 1,470 at (10, 14), 162 at (4, 8)."""
    k, n, _ = code
    pats = rc.all_patterns(n, n - k)
    assert len(pats) == {14: 1470, 8: 162}[n]
    for er in pats:
        _agree(code, rc.first_survivors(n, k, er), er)


def test_oracle_equals_the_inverse_at_3_19():
    """(3, 19), p = 16. A pattern's row for erased id x depends on the survivors and on x alone (the
    solve X is a function of the survivors; row x is a row of X or the base row of x plus its product
    with X), and a pattern of e erasures has the survivors and rows of the 16-erasure pattern with the
    same three survivors. So the 969 patterns of 16 erasures hold every (survivors, row) pair that any
    of the 524,287 patterns of 1..16 erasures has; they are all checked, and a seeded 1,500 of the
    others (a few from every e) are checked whole, among them every pattern of 1 and of 2 erasures:
    all half million through numpy take minutes."""
    code, k, n = (3, 19, "cauchy"), 3, 19
    full = list(itertools.combinations(range(n), 16))
    assert len(full) == 969
    for er in full:
        _agree(code, rc.first_survivors(n, k, er), er)
    small = rc.all_patterns(n, 2)
    assert len(small) == 19 + 171
    for er in small + rc.sample_patterns(n, 16, 1500 - len(small), 319, 3, 15):
        _agree(code, rc.first_survivors(n, k, er), er)


@pytest.mark.parametrize("code", list(rc.WIDE), ids=lambda c: f"{c[0]}-{c[1]}")
def test_oracle_equals_the_inverse_on_wide_codes(code):
    k, n, _ = code
    assert {len(er) for er in rc.WIDE[code]} >= {1, n - k}
    for er in rc.WIDE[code]:
        _agree(code, rc.first_survivors(n, k, er), er)


@pytest.mark.parametrize("code,survivors,erased", rc.CHOSEN, ids=lambda v: None)
def test_oracle_with_chosen_survivors(code, survivors, erased):
    """Survivor lists in any order that skip natives which are there, erased ids in any order."""
    k = code[0]
    assert any(i not in survivors and i not in erased for i in range(k)) or sorted(survivors) != list(survivors)
    _agree(code, survivors, erased)


def test_oracle_refuses_bad_lists():
    g = rc.codec(4, 8).G
    for sv, er in [((0, 1, 2), (3,)), ((0, 1, 2, 2), (3,)), ((0, 1, 2, 8), (3,)), ((0, 1, 2, -1), (3,)),
                   ((0, 1, 2, 3), (3,)), ((0, 1, 2, 3), (8,)), ((0, 1, 2, 3), (-1,))]:
        with pytest.raises(ValueError) as ei:
            gf.repair_coeff_oracle(g, sv, er)
        assert not isinstance(ei.value, gf.SingularMatrixError)
    assert gf.repair_coeff_oracle(g, (0, 1, 2, 3), ()).shape == (0, 4)


def test_vandermonde_singular_exactly_where_the_host_is():
    """Reference Vandermonde (10, 14), all 1,470 patterns: the oracle raises for exactly the patterns
    for which ``decode_matrix`` does (12, all of 4 erasures) and equals the inverse elsewhere."""
    code = (10, 14, "vandermonde")
    host = rc.vandermonde_singular()
    assert len(host) == 12 and all(len(er) == 4 for er in host)
    g = rc.codec(*code).G
    raised = []
    for er in rc.all_patterns(14, 4):
        sv = rc.first_survivors(14, 10, er)
        try:
            got = gf.repair_coeff_oracle(g, sv, er)
        except gf.SingularMatrixError:
            raised.append(er)
            continue
        assert np.array_equal(got, rc.host_coeff(code, sv, er)), er
    assert raised == host


@pytest.mark.parametrize("case", rc.PIVOT_GOOD, ids=str)
def test_oracle_on_the_pivoting_systems(case):
    """The planted systems of tests/solver_cases.py as ``rs.G`` / ``rs.E``: the natives' rows equal the
    host solve (``decode_matrix``), and with every parity row that is no survivor erased as well the
    whole block equals ``G[erased] . inv(G[survivors])``."""
    rs = rc.pivot_codec(case)
    g, rows, erased = sc.system(case)
    assert np.array_equal(rs.G, g) and np.array_equal(rs.E, g[case.k:])
    dm = rs.decode_matrix(rows)
    assert np.array_equal(dm[list(erased)], sc.oracle_rows(case))
    assert np.array_equal(gf.repair_coeff_oracle(rs.G, rows, erased), dm[list(erased)])
    lost_parity = [i for i in range(case.k, case.n) if i not in rows][:3]
    both = lost_parity[:1] + list(erased)[::-1] + lost_parity[1:]
    assert np.array_equal(gf.repair_coeff_oracle(rs.G, rows, both), gf.GF256.matmul(rs.G[both], dm))


@pytest.mark.parametrize("case", rc.PIVOT_SINGULAR, ids=str)
def test_oracle_on_the_singular_pivoting_systems(case):
    rs = rc.pivot_codec(case)
    _, rows, erased = sc.system(case)
    with pytest.raises(UnrecoverableError):
        rs.decode_matrix(rows)
    with pytest.raises(gf.SingularMatrixError):
        gf.repair_coeff_oracle(rs.G, rows, erased)


def test_repair_bench_fresh_runs_on_the_cpu():
    """``scripts/repair_bench.py --fresh --device cpu``: one small shape end to end, one JSON line."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "repair_bench.py"), "--fresh", "--device", "cpu",
                          "--code", "10:14", "--cols", "257", "--stripes", "5", "--erasures", "3", "--rounds", "1",
                          "--reps", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    (line,) = out.stdout.strip().splitlines()
    res = json.loads(line)
    assert res["fresh"] and res["shape"]["distinct_patterns"] == 5 and res["device"].startswith("cpu")
    for mode in ("host_solve", "device_solve"):
        assert res[mode]["batch_first_call_host_clock"]["median_us"] > 0


# ---- the keyword on CPU tensors --------------------------------------------------------------------------
def _cpu_batch(rs, nstripes, ncols, erased, seed):
    good = rc.consistent(rs.G, nstripes, ncols, seed)
    return good, torch.from_numpy(rc.damage(good, erased))


@pytest.mark.parametrize("field", ["gf256", "gf16"])
def test_cpu_tensors_ignore_the_flag(field):
    """``device_solve=True`` on CPU tensors is the default call: same bytes, any field, no GPU."""
    if field == "gf16":
        rs = ReedSolomon(4, 6, matrix="cauchy", field="gf16")
        erased = [[0], [5, 1], [], [2, 3]]
        stripes = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(4, 6, 37), dtype=np.uint8))
        for b in range(4):
            rs.encode(stripes[b, :4], stripes[b, 4:])
        good = stripes.numpy().copy()
        bad = torch.from_numpy(rc.damage(good, erased))
    else:
        rs = ReedSolomon(10, 14, matrix="cauchy")
        erased = [[0], [13, 2], [], [3, 4, 11, 12], [9, 8, 7, 6]]
        good, bad = _cpu_batch(rs, 5, 4099, erased, 7)
    a, b = bad.clone(), bad.clone()
    assert rs.reconstruct_batch(a, erased) is a
    assert rs.reconstruct_batch(b, erased, device_solve=True) is b
    assert torch.equal(a, b) and np.array_equal(b.numpy(), good)
    one, two = bad[1].clone(), bad[1].clone()
    rs.reconstruct(one, erased[1])
    rs.reconstruct(two, erased[1], device_solve=True)
    assert torch.equal(one, two) and np.array_equal(two.numpy(), good[1])


def test_cpu_singular_and_heal_with_the_flag():
    """A singular pattern on CPU tensors raises as it does without the flag, nothing written; heal_batch
    with the flag lists the singular stripe in ``unhealed``."""
    rs = ReedSolomon(10, 14, matrix="vandermonde")
    sing = rc.vandermonde_singular()[0]
    good = rc.consistent(rs.G, 3, 257, 11)
    bad = torch.from_numpy(rc.damage(good, [(1,), sing, (13,)]))
    before = bad.clone()
    with pytest.raises(UnrecoverableError, match="stripe 1"):
        rs.reconstruct_batch(bad, [[1], list(sing), [13]], device_solve=True)
    assert torch.equal(bad, before)
    with pytest.raises(UnrecoverableError):
        rs.reconstruct(bad[1], sing, device_solve=True)
    assert torch.equal(bad, before)
    dirty = np.array(good)
    dirty[0, 3, 5:9] ^= 0x41
    for t, i in enumerate(sing):
        dirty[1, i, 20 * t: 20 * t + 7] ^= 0x10 + t
    stripes = torch.from_numpy(dirty)
    rep = rs.heal_batch(stripes, device_solve=True)
    assert rep.unhealed == [1] and rep.dirty == [1]
    after = stripes.numpy()
    assert np.array_equal(after[[0, 2]], good[[0, 2]]) and np.array_equal(after[1], dirty[1])
