"""Batched partial-stripe writes on CPU tensors: ``ReedSolomon.update_batch`` / ``update_delta_batch`` /
``write_batch`` against the numpy oracle (``gf.update_oracle``, stripe by stripe), exactly. The case
functions take the device, so tests/test_gpu_update_batch.py runs the same cases through the batched
gfx950 kernel (``csrc/kernels/gf_update.hip``), where each case is also compared with a loop of single
``update`` / ``write`` calls on copies of the same buffers."""
import time
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_update as cases
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd._native import cpu
from gpu_rscode_amd.ops import BatchUpdatePlan
from gpu_rscode_amd.ops.rows import batch_part
from gpu_rscode_amd.ops.update import batch_ids, check_overlap_batch, update_batch_layout

# p = 1 | SUB = 2 | the flagship | p = 5, a padded sub-tile | p = 17, m_pad = 32 | wide
NARROW = [(3, 4, "vandermonde"), (4, 6, "cauchy"), (10, 14, "vandermonde"), (5, 10, "cauchy"), (19, 36, "cauchy")]
WIDE = (128, 160, "cauchy")
# one stripe | two | odd | more than a workgroup's worth of grid.y rows and no multiple of anything
BATCHES = [1, 2, 3, 257]
# tail only | no group, 15 tail lanes | one group and a tail byte | a workgroup edge and a tail
SHAPES = [1, 15, 17, 4101]
RUNS = [(c, b, s) for c in NARROW for b in BATCHES for s in SHAPES] + [(c, 2, 65536 + 3) for c in NARROW] \
    + [(WIDE, 3, s) for s in (17, 4101)]


def run_id(r):
    return f"{cases.code_id(r[0])}-B{r[1]}-C{r[2]}"


@lru_cache(maxsize=None)
def host_batch(code, nstripes: int, ncols: int) -> np.ndarray:
    """B consistent stripes ``[B, n, C]`` (one oracle GEMM over all columns); shared, never modified."""
    k, n, _ = code
    rng = np.random.default_rng(11 * n + 1000 * nstripes + ncols)
    data = rng.integers(0, 256, size=(nstripes, k, ncols), dtype=np.uint8)
    flat = data.transpose(1, 0, 2).reshape(k, nstripes * ncols)
    par = gf.GF256.gemm(cases.codec(code).E, flat).reshape(n - k, nstripes, ncols).transpose(1, 0, 2)
    out = np.ascontiguousarray(np.concatenate([data, par], axis=1))
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def host_new_batch(code, nstripes: int, ncols: int) -> np.ndarray:
    """New contents for every native of every stripe, ``[B, k, C]``."""
    k, n, _ = code
    out = np.random.default_rng(13 * n + 1000 * nstripes + ncols + 1).integers(0, 256, size=(nstripes, k, ncols),
                                                                               dtype=np.uint8)
    out.setflags(write=False)
    return out


def pick(rows: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """``rows[b, ids[b, t]]`` as ``[B, d, C]``."""
    return np.take_along_axis(rows, np.asarray(ids, dtype=np.int64)[:, :, None], axis=1)


def expected_batch(code, host: np.ndarray, ids: np.ndarray, old: np.ndarray, new: np.ndarray) -> np.ndarray:
    """``gf.update_oracle`` stripe by stripe: ``[B, p, C]``."""
    k, e = code[0], cases.codec(code).E
    return np.stack([gf.update_oracle(e, host[b, k:], list(ids[b]), old[b], new[b]) for b in range(host.shape[0])])


def spread_ids(k: int, nstripes: int, d: int, seed: int = 0) -> np.ndarray:
    """d distinct ids per stripe, unsorted, another permutation in each stripe; stripe b's first id is
    ``b % k``, so ids 0 and k - 1 both occur once B >= k."""
    rng = np.random.default_rng(100 * k + d + seed)
    out = np.empty((nstripes, d), dtype=np.int64)
    for b in range(nstripes):
        rest = [j for j in rng.permutation(k) if j != b % k]
        out[b] = [b % k] + rest[: d - 1]
    return out


def to_batch(host: np.ndarray, device: str, shift: int = 0):
    """``[B, r, C]`` host rows in alloc_rows storage with garbage in the pitch padding: the 2-D
    ``[B * r, C]`` tensor (for the padding check) and its ``[B, r, C]`` view."""
    nstripes, r, ncols = host.shape
    flat = cases.to_device(host.reshape(nstripes * r, ncols), device, shift)
    pitch = flat.stride(0)
    return flat, flat.as_strided((nstripes, r, ncols), (r * pitch, pitch, 1), flat.storage_offset())


def assert_batch(t: torch.Tensor, want: np.ndarray, what=""):
    got = t.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def singles(device) -> bool:
    """On the GPU every case is also compared with a loop of single calls (another kernel path)."""
    return device != "cpu"


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_forms(device, code, nstripes, ncols, ids=None, shift=0):
    """All three forms over the whole rows: the oracle's parity stripe by stripe; old, new, delta and
    the pitch padding unchanged; the natives hold new after a write."""
    rs, k = cases.codec(code), code[0]
    host, fresh = host_batch(code, nstripes, ncols), host_new_batch(code, nstripes, ncols)
    ids = spread_ids(k, nstripes, min(2, k)) if ids is None else np.asarray(ids)
    old, new = pick(host, ids), pick(fresh, ids)
    want = expected_batch(code, host, ids, old, new)
    pf, par = to_batch(host[:, k:], device, shift)
    of, old_t = to_batch(old, device, shift)
    nf, new_t = to_batch(new, device, shift)
    assert rs.update_batch(par, ids, old_t, new_t) is par
    assert_batch(par, want, "update_batch")
    assert_batch(old_t, old, "old")
    assert_batch(new_t, new, "new")
    p2f, par2 = to_batch(host[:, k:], device, shift)
    df, delta = to_batch(old ^ new, device, shift)
    assert rs.update_delta_batch(par2, ids, delta) is par2
    assert_batch(par2, want, "update_delta_batch")
    assert_batch(delta, old ^ new, "delta")
    sf, stripes = to_batch(host, device, shift)
    assert rs.write_batch(stripes, ids, new_t) is stripes
    full = np.array(host)
    np.put_along_axis(full, ids[:, :, None], new, axis=1)
    full[:, k:] = want
    assert_batch(stripes, full, "write_batch")
    assert_batch(new_t, new, "new after write")
    cases.assert_padding(pf, of, nf, p2f, df, sf)
    if singles(device):
        p3f, par3 = to_batch(host[:, k:], device, shift)
        s3f, stripes3 = to_batch(host, device, shift)
        for b in range(nstripes):
            rs.update(par3[b], [int(j) for j in ids[b]], old_t[b], new_t[b])
            rs.write(stripes3[b], [int(j) for j in ids[b]], new_t[b])
        assert torch.equal(par3, par) and torch.equal(stripes3, stripes), "batch differs from a loop of single calls"


def case_shared_list(device, code=(10, 14, "vandermonde"), nstripes=4, ncols=4101):
    """A shared list gives what the same list repeated B times gives."""
    rs, k = cases.codec(code), code[0]
    host, fresh = host_batch(code, nstripes, ncols), host_new_batch(code, nstripes, ncols)
    shared = [k - 1, 0, 4]
    ids = np.tile(np.array(shared), (nstripes, 1))
    old, new = pick(host, ids), pick(fresh, ids)
    want = expected_batch(code, host, ids, old, new)
    (_, old_t), (_, new_t) = to_batch(old, device), to_batch(new, device)
    for form in (shared, tuple(shared), ids.tolist(), ids):
        _, par = to_batch(host[:, k:], device)
        rs.update_batch(par, form, old_t, new_t)
        assert_batch(par, want, type(form).__name__)


def case_stripe_identity(device, nstripes, which, code=(10, 14, "vandermonde"), ncols=4101):
    """Only stripe ``which`` has a nonzero delta: every other stripe's parity is byte for byte what it
    was, the changed one equals the oracle."""
    rs, k = cases.codec(code), code[0]
    host, fresh = host_batch(code, nstripes, ncols), host_new_batch(code, nstripes, ncols)
    ids = spread_ids(k, nstripes, 2, seed=which)
    delta = np.zeros((nstripes, 2, ncols), dtype=np.uint8)
    delta[which] = pick(host, ids)[which] ^ pick(fresh, ids)[which]
    want = np.array(host[:, k:])
    want[which] = gf.update_oracle(rs.E, host[which, k:], list(ids[which]), pick(host, ids)[which],
                                   pick(fresh, ids)[which])
    assert not np.array_equal(want[which], host[which, k:])
    pf, par = to_batch(host[:, k:], device)
    df, delta_t = to_batch(delta, device)
    rs.update_delta_batch(par, ids, delta_t)
    assert_batch(par, want, f"stripe {which} of {nstripes}")
    cases.assert_padding(pf, df)


def case_write_forms(device, code, nstripes=3, ncols=4101, col0=0, nc=None):
    """write_batch in the one-tensor form and the natives + parity= form: the stripes' syndrome
    (existing code, independent of the update) is all zero, the natives equal new inside the window
    and their old contents outside it."""
    rs, k = cases.codec(code), code[0]
    host, fresh = host_batch(code, nstripes, ncols), host_new_batch(code, nstripes, ncols)
    nc = ncols - col0 if nc is None else nc
    w = slice(col0, col0 + nc)
    ids = spread_ids(k, nstripes, min(3, k), seed=5)
    new = pick(fresh, ids)
    want_nat = np.array(host[:, :k])
    inside = np.array(want_nat)
    np.put_along_axis(inside, ids[:, :, None], new, axis=1)
    want_nat[:, :, w] = inside[:, :, w]
    nf, new_t = to_batch(new, device)
    sf, stripes = to_batch(host, device)
    assert rs.write_batch(stripes, ids, new_t, col0=col0, ncols=nc) is stripes
    assert_batch(stripes[:, :k], want_nat, "natives, one tensor")
    assert not rs.syndrome_mask_batch(stripes, block_bytes=4096).cpu().numpy().any()
    df, data = to_batch(host[:, :k], device)
    pf, par = to_batch(host[:, k:], device)
    assert rs.write_batch(data, ids, new_t, parity=par, col0=col0, ncols=nc) is data
    assert_batch(data, want_nat, "natives, parity=")
    assert not rs.syndrome_mask_batch(data, par, block_bytes=4096).cpu().numpy().any()
    assert torch.equal(par, stripes[:, k:])
    assert_batch(new_t, new, "new")
    cases.assert_padding(nf, sf, df, pf)


def case_window(device, code, col0, ncols, nstripes=3):
    """A window of 4117-byte stripes: inside it the oracle's bytes, outside it byte-identical to before,
    parity and (under write) natives alike. A col0 that is no multiple of 16 takes the byte form."""
    rs, k, c = cases.codec(code), code[0], cases.WINDOW_C
    host, fresh = host_batch(code, nstripes, c), host_new_batch(code, nstripes, c)
    w = slice(col0, col0 + ncols)
    for d in (1, min(k, 9)):
        ids = spread_ids(k, nstripes, d, seed=col0)
        old, new = pick(host, ids), pick(fresh, ids)
        want = np.array(host)
        want[:, k:, w] = expected_batch(code, host, ids, old, new)[:, :, w]
        (pf, par), (of, old_t), (nf, new_t) = (to_batch(a, device) for a in (host[:, k:], old, new))
        rs.update_batch(par, ids, old_t, new_t, col0=col0, ncols=ncols)
        assert_batch(par, want[:, k:], "update_batch")
        assert_batch(old_t, old, "old")
        (p2f, par2), (df, delta) = to_batch(host[:, k:], device), to_batch(old ^ new, device)
        rs.update_delta_batch(par2, ids, delta, col0, ncols)
        assert_batch(par2, want[:, k:], "update_delta_batch")
        sf, stripes = to_batch(host, device)
        inside = np.array(want)
        np.put_along_axis(inside, ids[:, :, None], new, axis=1)
        want[:, :k, w] = inside[:, :k, w]
        rs.write_batch(stripes, ids, new_t, col0=col0, ncols=ncols)
        assert_batch(stripes, want, "write_batch")
        assert_batch(new_t, new, "new")
        cases.assert_padding(pf, of, nf, p2f, df, sf)


def case_one_unaligned_row(device, code=(10, 14, "vandermonde"), nstripes=3, ncols=4101):
    """One row of one stripe one byte off alignment (the lists-of-rows form): the whole batch takes the
    byte form (``plan.bytewise``) and stays exact."""
    rs, k = cases.codec(code), code[0]
    host, fresh = host_batch(code, nstripes, ncols), host_new_batch(code, nstripes, ncols)
    ids = spread_ids(k, nstripes, 2, seed=9)
    old, new = pick(host, ids), pick(fresh, ids)
    want = expected_batch(code, host, ids, old, new)
    for odd in ("parity", "old", "new"):
        (pf, par), (of, old_t), (nf, new_t) = (to_batch(a, device) for a in (host[:, k:], old, new))
        rows = {"parity": [[par[b, i] for i in range(par.shape[1])] for b in range(nstripes)],
                "old": [[old_t[b, t] for t in range(2)] for b in range(nstripes)],
                "new": [[new_t[b, t] for t in range(2)] for b in range(nstripes)]}
        src = {"parity": host[1, k + 1], "old": old[1, 1], "new": new[1, 1]}[odd]
        off = cases.to_device(src[None], device, shift=1)
        assert off[0].data_ptr() % 16 == 1
        rows[odd][1][1] = off[0]
        if device != "cpu":
            plan = BatchUpdatePlan(rows["parity"], rows["old"], rows["new"], changed=ids, coeff=rs.E)
            aligned = BatchUpdatePlan(par, old_t, new_t, changed=ids, coeff=rs.E)
            assert plan.bytewise and not aligned.bytewise
        rs.update_batch(rows["parity"], ids, rows["old"], rows["new"])
        got = np.stack([cases.to_host(r) for r in rows["parity"]])
        assert np.array_equal(got, want), odd
        assert np.array_equal(cases.to_host(rows["old"][1]), old[1]) and np.array_equal(cases.to_host(rows["new"][1]),
                                                                                       new[1])
        cases.assert_padding(pf, of, nf, off)


def case_input_forms(device, code=(4, 6, "cauchy"), nstripes=3, ncols=4101):
    """Contiguous tensors, strided views (a slice of a larger tensor in the batch and row dimensions),
    a list of tensors and a list of lists of rows, each with ids as a list, a numpy array and a CPU
    tensor: one result."""
    rs, k, n = cases.codec(code), code[0], code[1]
    host, fresh = host_batch(code, nstripes, ncols), host_new_batch(code, nstripes, ncols)
    ids = spread_ids(k, nstripes, 2, seed=3)
    old, new = pick(host, ids), pick(fresh, ids)
    want = expected_batch(code, host, ids, old, new)
    full = np.array(host)
    np.put_along_axis(full, ids[:, :, None], new, axis=1)
    full[:, k:] = want

    def contiguous(a):
        return torch.from_numpy(np.array(a)).to(device)

    def strided(a):
        big = torch.full((a.shape[0] + 2, a.shape[1] + 3, a.shape[2] + 64), cases.GARBAGE, dtype=torch.uint8,
                         device=device)
        view = big[1: 1 + a.shape[0], 2: 2 + a.shape[1], 32: 32 + a.shape[2]]
        view.copy_(torch.from_numpy(np.array(a)))
        assert not view.is_contiguous()
        return view

    def tensors(a):
        return [contiguous(s) for s in a]

    def lists(a):
        return [[contiguous(r) for r in s] for s in a]

    def host_of(x):
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.stack([cases.to_host(s) for s in x])

    id_forms = (ids.tolist(), ids, ids.astype(np.int32), torch.from_numpy(ids), torch.from_numpy(ids.astype(np.int32)))
    for i, make in enumerate((contiguous, strided, tensors, lists)):
        for id_form in id_forms[i % 2:: 2] if i else id_forms:
            par, old_t, new_t = make(host[:, k:]), make(old), make(new)
            assert rs.update_batch(par, id_form, old_t, new_t) is par
            assert np.array_equal(host_of(par), want), (make.__name__, type(id_form).__name__)
            par2 = make(host[:, k:])
            rs.update_delta_batch(par2, id_form, make(old ^ new))
            assert np.array_equal(host_of(par2), want), (make.__name__, "delta")
            stripes = make(host)
            assert rs.write_batch(stripes, id_form, new_t) is stripes
            assert np.array_equal(host_of(stripes), full), (make.__name__, "write")
            data, par3 = make(host[:, :k]), make(host[:, k:])
            rs.write_batch(data, id_form, new_t, parity=par3)
            assert np.array_equal(host_of(data), full[:, :k]) and np.array_equal(host_of(par3), want)
            assert np.array_equal(host_of(old_t), old) and np.array_equal(host_of(new_t), new)
    # mixed forms in one call
    par, new_t = strided(host[:, k:]), tensors(new)
    rs.update_batch(par, ids, lists(old), new_t)
    assert np.array_equal(host_of(par), want)


def case_refusals(device):
    """Each raises ValueError with every buffer unchanged."""
    code, nstripes, c = (4, 6, "cauchy"), 3, 4101
    rs, k = cases.codec(code), 4
    host, fresh = host_batch(code, nstripes, c), host_new_batch(code, nstripes, c)
    sf, stripes = to_batch(host, device)
    nf, new_t = to_batch(fresh, device)
    par, nat = stripes[:, k:], stripes[:, :k]
    ids = np.array([[1], [3], [0]])
    old1, new1 = nat[:, 1:2], new_t[:, 1:2]  # one row per stripe, of some native: what they hold is not the point

    def refused(fn, *a, exc=ValueError, **kw):
        with pytest.raises(exc):
            fn(*a, **kw)
        assert_batch(stripes, host, "stripes after a refusal")
        assert_batch(new_t, fresh, "new after a refusal")

    for fn, first in ((rs.update_batch, (par,)), (rs.update_delta_batch, (par,)), (rs.write_batch, (stripes,))):
        pair = fn == rs.update_batch

        def rows(d=1, nb=nstripes):
            return (nat[:nb, :d], new_t[:nb, :d]) if pair else (new_t[:nb, :d],)
        refused(fn, *first, [[1, 1]] * 3, *rows(2))                # a duplicate id in one stripe's row
        refused(fn, *first, [[0, 1], [2, 2], [1, 3]], *rows(2))
        refused(fn, *first, [[1], [k], [0]], *rows())              # an id of k
        refused(fn, *first, [[1], [0], [-1]], *rows())             # an id of -1
        refused(fn, *first, ids[:2], *rows())                      # ids of shape [B - 1, d]
        refused(fn, *first, [[1], [2, 3], [0]], *rows())           # a ragged ids list
        refused(fn, *first, [[1, 2], [2, 3], [0]], *rows(2))
        refused(fn, *first, [], *rows())                           # no ids at all
        refused(fn, *first, np.zeros((3, 0), dtype=np.int64), *rows())
        refused(fn, *first, [[0, 1, 2, 3, 0]] * 3, *rows(4))       # more than k
        refused(fn, *first, np.array([[1.0], [2.0], [0.0]]), *rows())  # not integers
        refused(fn, *first, np.zeros((3, 1, 1), dtype=np.int64), *rows())
        refused(fn, *first, ids, *rows(2))                         # wrong row counts
        refused(fn, *first, ids, *rows(1, 2))                      # wrong stripe counts
        refused(fn, *first, ids, *(r[:, :, :c - 1] for r in rows()))  # unequal lengths
        refused(fn, *first, ids, *rows()[:-1], rows()[-1].to(torch.int8))  # int8 rows
        refused(fn, *first, ids, *rows(), col0=c - 1, ncols=2)     # a window past the rows
        refused(fn, *first, ids, *rows(), col0=-1)
        refused(fn, *first, ids, *rows(), col0=c + 1)
        refused(fn, *first, ids, *rows(), ncols=-1)
        if device != "cpu":
            refused(fn, *first, ids.tolist(), *rows()[:-1], rows()[-1].cpu())  # mixed devices
            refused(fn, *first, torch.from_numpy(ids).to(device), *rows())    # CUDA ids
    refused(rs.update_batch, par[:, :1], ids, old1, new1)          # parity row count
    refused(rs.update_batch, par.to(torch.int8), ids, old1, new1)
    refused(rs.write_batch, stripes[:, :5], ids, new1)             # not n rows
    refused(rs.write_batch, nat, ids, new1, parity=par[:, :1])
    refused(rs.write_batch, nat[:2], ids[:2], new1[:2], parity=par)
    # aliasing, over the whole batch
    twice = [par[0], par[1], par[0]]
    refused(rs.update_batch, twice, ids, old1, new1)               # one stripe's parity listed twice
    refused(rs.update_delta_batch, twice, ids, new1)
    # one parity row shared by two stripes
    refused(rs.update_batch, [[par[0, 0], par[0, 1]], [par[1, 0], par[0, 1]], par[2]], ids, old1, new1)
    refused(rs.update_batch, [[par[0, 0], par[0, 1]], [par[1, 0], par[0, 1][5:c]], par[2]], ids,
            old1[:, :, : c - 5], new1[:, :, : c - 5])
    refused(rs.update_batch, par, ids, old1, par[:, :1])           # a parity row as a new row
    refused(rs.update_delta_batch, par, ids, [[par[1, 0]], [par[2, 0]], [par[0, 0]]])  # ... of another stripe
    refused(rs.update_batch, par, ids, old1, old1)                 # new overlapping old
    refused(rs.update_batch, par, ids, old1, [[nat[1, 1]], [nat[2, 1]], [nat[0, 1]]])  # ... another stripe's old
    refused(rs.write_batch, stripes, ids, pick_t(nat, ids))        # new inside the stripes
    refused(rs.write_batch, stripes, ids, par[:, :1])
    refused(rs.write_batch, nat, ids, par[:, :1], parity=par)
    refused(rs.write_batch, [stripes[0], stripes[1], stripes[0]], ids, new1)  # one stripe written twice
    cases.assert_padding(sf, nf)


def pick_t(t: torch.Tensor, ids) -> list:
    return [[t[b, int(j)] for j in row] for b, row in enumerate(np.asarray(ids))]


def case_no_parity_and_empty(device):
    """p == 0: update_batch is a no-op, write_batch only copies (inside the window). B == 0 returns."""
    rs = ReedSolomon(3, 3)
    rng = np.random.default_rng(3)
    data, new = rng.integers(0, 256, (2, 3, 100), dtype=np.uint8), rng.integers(0, 256, (2, 1, 100), dtype=np.uint8)
    (sf, stripes), (nf, new_t) = to_batch(data, device), to_batch(new, device)
    empty = stripes[:, 3:]
    ids = [[1], [2]]
    assert rs.update_batch(empty, ids, stripes[:, 1:2], new_t) is empty
    rs.update_delta_batch(empty, ids, new_t)
    assert_batch(stripes, data)
    rs.write_batch(stripes, ids, new_t, col0=10, ncols=50)
    data[0, 1, 10:60], data[1, 2, 10:60] = new[0, 0, 10:60], new[1, 0, 10:60]
    assert_batch(stripes, data)
    cases.assert_padding(sf, nf)
    rs = cases.codec((4, 6, "cauchy"))
    none = torch.zeros((0, 6, 64), dtype=torch.uint8, device=device)
    assert rs.update_batch(none[:, 4:], [1], none[:, :1], none[:, :1]) is not None
    rs.update_delta_batch(none[:, 4:], np.zeros((0, 1), dtype=np.int64), none[:, :1])
    assert rs.write_batch(none, [2, 0], none[:, :2]) is none
    rs.update_batch([], [1], [], [])


def case_other_field(device, field, code=(4, 6, "cauchy"), nstripes=3, ncols=4102):
    """gf16 / gf65536: the updated parity equals the codec's own encode_batch of the new natives."""
    k, n, matrix = code
    rs = ReedSolomon(k, n, matrix=matrix, field=field)
    rng = np.random.default_rng(n + ncols)
    data = rng.integers(0, 256, size=(nstripes, k, ncols), dtype=np.uint8)
    fresh = rng.integers(0, 256, size=(nstripes, k, ncols), dtype=np.uint8)
    parity = rs.encode_batch(torch.from_numpy(data).to(device)).cpu().numpy()
    for d in (1, 2, k):
        ids = spread_ids(k, nstripes, d, seed=d)
        after = np.array(data)
        np.put_along_axis(after, ids[:, :, None], pick(fresh, ids), axis=1)
        want = rs.encode_batch(torch.from_numpy(after).to(device)).cpu().numpy()
        for c0, nc in ((0, ncols), (18, 4000)):
            w = slice(c0, c0 + nc)
            expect = np.array(parity)
            expect[:, :, w] = want[:, :, w]
            (pf, par), (of, old_t), (nf, new_t) = (to_batch(a, device)
                                                   for a in (parity, pick(data, ids), pick(fresh, ids)))
            rs.update_batch(par, ids, old_t, new_t, c0, nc)
            assert_batch(par, expect, (field, d, "update_batch"))
            p2f, par2 = to_batch(parity, device)
            rs.update_delta_batch(par2, ids, to_batch(pick(data, ids) ^ pick(fresh, ids), device)[1], c0, nc)
            assert_batch(par2, expect, (field, d, "update_delta_batch"))
            sf, stripes = to_batch(np.concatenate([data, parity], axis=1), device)
            rs.write_batch(stripes, ids, new_t, col0=c0, ncols=nc)
            full = np.concatenate([data, expect], axis=1)
            inside = np.concatenate([after, expect], axis=1)
            full[:, :k, w] = inside[:, :k, w]
            assert_batch(stripes, full, (field, d, "write_batch"))
            cases.assert_padding(pf, of, nf, p2f, sf)


# ---- CPU tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,nstripes,ncols", RUNS, ids=map(run_id, RUNS))
def test_codes_batches_and_row_lengths(code, nstripes, ncols):
    case_forms("cpu", code, nstripes, ncols)


IDS_RUNS = [((10, 14, "vandermonde"), 11, d) for d in (1, 2, 3, 8, 9, 10)] + \
    [((4, 6, "cauchy"), 5, d) for d in (1, 2, 3, 4)] + [((19, 36, "cauchy"), 20, d) for d in (1, 9, 19)] + \
    [(WIDE, 3, d) for d in (8, 17)]


@pytest.mark.parametrize("code,nstripes,d", IDS_RUNS, ids=[f"{cases.code_id(c)}-B{b}-d{d}" for c, b, d in IDS_RUNS])
def test_per_stripe_ids(code, nstripes, d):
    """Stripe b changes native b % k first (ids 0 and k - 1 both occur); d = 2, 3 unsorted with another
    permutation in each stripe; d = 8 the cap, d = 9 two passes, d = k."""
    ids = spread_ids(code[0], nstripes, d)
    if nstripes >= code[0]:
        assert {0, code[0] - 1} <= set(ids[:, 0].tolist())
    case_forms("cpu", code, nstripes, 4101 if code != WIDE else 273, ids)


def test_shared_list_equals_the_list_repeated():
    case_shared_list("cpu")


@pytest.mark.parametrize("nstripes,which", [(3, 0), (3, 1), (3, 2), (257, 0), (257, 128), (257, 256)])
def test_stripe_identity(nstripes, which):
    case_stripe_identity("cpu", nstripes, which)


@pytest.mark.parametrize("col0,nc", [(0, None), (16, 4000), (5, 100)])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (5, 10, "cauchy")], ids=cases.code_id)
def test_write_batch_forms(code, col0, nc):
    case_write_forms("cpu", code, col0=col0, nc=nc)


@pytest.mark.parametrize("col0,ncols", cases.WINDOWS)
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=cases.code_id)
def test_windows(code, col0, ncols):
    case_window("cpu", code, col0, ncols)


def test_one_unaligned_row():
    case_one_unaligned_row("cpu")


def test_input_forms():
    case_input_forms("cpu")


def test_refusals():
    case_refusals("cpu")


def test_no_parity_rows_and_empty_batch():
    case_no_parity_and_empty("cpu")


def test_gf16_field():
    case_other_field("cpu", "gf16")


def test_gf65536_field():
    case_other_field("cpu", "gf65536")
    rs = ReedSolomon(4, 6, field="gf65536")
    rows = torch.zeros((2, 7, 64), dtype=torch.uint8)
    for c0, nc in ((1, 10), (2, 9)):
        with pytest.raises(ValueError, match="even"):
            rs.update_batch(rows[:, 4:6], [0], rows[:, :1], rows[:, 6:], c0, nc)


def test_layout_mirror_and_plan_is_gpu_only():
    for args in ((4, 1, 2, 1), (10, 3, 4, 7), (128, 8, 32, 257), (19, 8, 32, 65537)):
        assert dict(cpu().update_batch_layout(*args)) == update_batch_layout(*args)
    rows = torch.zeros((2, 3, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        BatchUpdatePlan(rows[:, :1], rows[:, 1:2], rows[:, 2:3], changed=[0], coeff=np.array([[1, 2]], dtype=np.uint8))


def test_a_batch_of_65537_stripes_validates_without_a_loop_over_stripes():
    """Ids and aliasing of a tensor-form batch of 65,537 stripes: numpy on the pointer arrays, well under
    a second (a Python loop over the stripes' rows takes several)."""
    nstripes = 65537
    t = torch.zeros((nstripes, 8, 32), dtype=torch.uint8)
    ids = np.arange(nstripes)[:, None] % 4
    t0 = time.perf_counter()
    par, old, new = (batch_part(x, "rows") for x in (t[:, 4:6, :17], t[:, 6:7, :17], t[:, 7:8, :17]))
    assert batch_ids(ids, nstripes, 4).shape == (nstripes, 1)
    check_overlap_batch(par.ptrs(), old.ptrs(), new.ptrs(), 17, True)
    took = time.perf_counter() - t0
    assert took < 1.0, took
    with pytest.raises(ValueError, match="overlap"):
        check_overlap_batch(par.ptrs(), old.ptrs(), batch_part(t[:, 5:6, :17], "rows").ptrs(), 17)
    same = torch.cat([t[:65536], t[4:5]])  # (a copy: no aliasing) ...
    check_overlap_batch(batch_part(same[:, 4:6], "rows").ptrs(), batch_part(same[:, 6:7], "rows").ptrs(), None, 32)
    ptrs = par.ptrs().copy()
    ptrs[65536] = ptrs[4]  # ... the same stripe listed twice
    with pytest.raises(ValueError, match="overlap"):
        check_overlap_batch(ptrs, old.ptrs(), new.ptrs(), 17)
