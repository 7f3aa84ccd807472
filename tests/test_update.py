"""Partial-stripe writes on CPU tensors: ``ReedSolomon.update`` / ``update_delta`` / ``write`` against
the numpy oracle (``gf.update_oracle``), exactly, and against the encoding of the new natives. The
case functions take the device, so tests/test_gpu_update.py runs the same cases through the gfx950
kernel (``csrc/kernels/gf_update.hip``)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from gpu_rscode_amd import ReedSolomon, alloc_rows, flat_rows, gf
from gpu_rscode_amd.ops import UpdatePlan

# (k, n, matrix): the common narrow codes | p = 1 | p = 5, a padded sub-tile | p = 16 | p = 17, one past a
# multiple of 4 and of 16 | p = 32 | p = 56
NARROW = [(4, 6, "cauchy"), (10, 14, "vandermonde"), (3, 4, "vandermonde"), (5, 10, "cauchy"),
          (20, 36, "vandermonde"), (19, 36, "cauchy")]
WIDE = [(128, 160, "cauchy"), (200, 256, "cauchy")]
CODES = NARROW + WIDE
# tail only | one 16-byte group, with and without a tail byte | one workgroup span, with and without
# a tail | past 65536; the wide codes keep the two smallest that hold a group, a tail and a workgroup edge
SHAPES = [1, 15, 16, 17, 4096, 4101, 65536 + 3]
WIDE_SHAPES = [17, 4101]
GARBAGE = 0xA5
WINDOW_C = 4117  # the shortest row that holds every window below, with a ragged tail
WINDOWS = [(16, 4096), (4096, 5), (0, WINDOW_C), (WINDOW_C - 1, 1), (5, 100), (17, 4101 - 17)]


def code_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}"


def changed_lists(k: int) -> list[tuple]:
    """[0] and [k-1] | [k-1, 0], unsorted | 3 ids (the pair loop has a remainder) | 8 ids, the cap | 9
    ids, two passes | all k; each where k allows, without repeats."""
    rng = np.random.default_rng(k)
    out = [(0,), (k - 1,), (k - 1, 0)]
    for d in (3, 8, 9):
        if d <= k:
            out.append(tuple(int(j) for j in rng.permutation(k)[:d]))
    out.append(tuple(range(k)))
    seen, uniq = set(), []
    for c in out:
        if c not in seen and len(set(c)) == len(c):
            seen.add(c)
            uniq.append(c)
    return uniq


FULL = [(c, s, ch) for c in CODES for s in (SHAPES if c in NARROW else WIDE_SHAPES) for ch in changed_lists(c[0])]
# write, windows and the rest: every code at the shapes with a group, a tail and a workgroup edge
SHORT = [(c, s, ch) for c in CODES for s in WIDE_SHAPES for ch in changed_lists(c[0])]


def run_id(r):
    c, s, ch = r
    return f"{code_id(c)}-{s}-d{len(ch)}-{ch[0]}"


@lru_cache(maxsize=None)
def codec(code) -> ReedSolomon:
    k, n, matrix = code
    return ReedSolomon(k, n, matrix=matrix)


@lru_cache(maxsize=None)
def host_stripe(code, ncols: int) -> np.ndarray:
    """A consistent [n, C] stripe, encoded by the numpy oracle; shared by every test, never modified."""
    k, n, _ = code
    rng = np.random.default_rng(7000 * n + ncols)
    data = rng.integers(0, 256, size=(k, ncols), dtype=np.uint8)
    out = np.vstack([data, gf.GF256.gemm(codec(code).E, data)])
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def host_new(code, ncols: int) -> np.ndarray:
    """New contents for every native, [k, C]; a test takes rows ``changed``."""
    k, n, _ = code
    out = np.random.default_rng(9000 * n + ncols + 1).integers(0, 256, size=(k, ncols), dtype=np.uint8)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def expected_parity(code, ncols: int, changed: tuple) -> np.ndarray:
    """``gf.update_oracle`` on the host stripe, cross-checked once against the encoding of the new
    natives: the updated parity is the parity of the stripe that holds them."""
    k = code[0]
    host, new = host_stripe(code, ncols), host_new(code, ncols)
    ch = list(changed)
    want = gf.update_oracle(codec(code).E, host[k:], ch, host[ch], new[ch])
    data = np.array(host[:k])
    data[ch] = new[ch]
    assert np.array_equal(want, gf.GF256.gemm(codec(code).E, data))
    want.setflags(write=False)
    return want


def to_device(host: np.ndarray, device: str, shift: int = 0) -> torch.Tensor:
    """The rows in alloc_rows storage whose pitch padding holds garbage; ``shift`` starts every row
    that many bytes past its 16-byte aligned start (one spare row keeps the last row's padding inside
    the storage)."""
    rows = host.shape[0]
    t = alloc_rows(rows + 1, host.shape[1] + shift, device, fill=GARBAGE)[:rows, shift:]
    assert all(t[i].data_ptr() % 16 == shift for i in range(rows))
    t.copy_(torch.from_numpy(np.array(host)))
    return t


def to_host(t) -> np.ndarray:
    rows = [t[i] for i in range(t.shape[0])] if isinstance(t, torch.Tensor) else t
    return np.stack([r.cpu().numpy() for r in rows])


def assert_padding(*tensors):
    """Every byte between the rows' C columns (the pitch padding, and the bytes before a shifted
    row's start) still holds the fill."""
    for t in tensors:
        flat = flat_rows(t).cpu().numpy().reshape(t.shape[0], t.stride(0))
        assert (flat[:, t.shape[1]:] == GARBAGE).all(), "pitch padding written"


def assert_rows(t, want: np.ndarray, what=""):
    got = to_host(t)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


# ---- cases (device-generic) -----------------------------------------------------------------------
def case_update(device, code, ncols, changed, shift=0, shift_new=None):
    """update and update_delta over the whole row: both give the oracle's parity; old, new, delta and
    the pitch padding are unchanged."""
    rs, k, ch = codec(code), code[0], list(changed)
    host, new = host_stripe(code, ncols), host_new(code, ncols)
    want = expected_parity(code, ncols, changed)
    par = to_device(host[k:], device, shift)
    old_t = to_device(host[ch], device, shift)
    new_t = to_device(new[ch], device, shift if shift_new is None else shift_new)
    assert rs.update(par, ch, old_t, new_t) is par
    assert_rows(par, want, "update")
    assert_rows(old_t, host[ch], "old")
    assert_rows(new_t, new[ch], "new")
    par2 = to_device(host[k:], device, shift)
    delta = to_device(host[ch] ^ new[ch], device, shift if shift_new is None else shift_new)
    assert rs.update_delta(par2, ch, [delta[t] for t in range(len(ch))]) is par2
    assert_rows(par2, want, "update_delta")
    assert_rows(delta, host[ch] ^ new[ch], "delta")
    assert_padding(par, old_t, new_t, par2, delta)


def case_write(device, code, ncols, changed, shift=0, shift_new=None):
    """write: the natives equal new, the parity equals the oracle, nothing else moved, and on gf256 the
    stripe's syndrome (existing code, independent of the update) is zero."""
    rs, k, ch = codec(code), code[0], list(changed)
    host, new = host_stripe(code, ncols), host_new(code, ncols)
    want = np.array(host)
    want[ch] = new[ch]
    want[k:] = expected_parity(code, ncols, changed)
    stripe = to_device(host, device, shift)
    new_t = to_device(new[ch], device, shift if shift_new is None else shift_new)
    assert rs.write(stripe, ch, new_t) is stripe
    assert_rows(stripe, want, "write")
    assert_rows(new_t, new[ch], "new")
    assert_padding(stripe, new_t)
    assert not rs.syndrome_mask(stripe, 4096).cpu().numpy().any()


def case_window(device, code, col0, ncols, changed):
    """A window of a 4117-byte stripe: inside it the oracle's bytes, outside it byte-identical to before,
    parity and (under write) natives alike."""
    rs, k, ch, c = codec(code), code[0], list(changed), WINDOW_C
    host, new = host_stripe(code, c), host_new(code, c)
    w = slice(col0, col0 + ncols)
    want = np.array(host)
    want[k:, w] = expected_parity(code, c, changed)[:, w]
    par, old_t, new_t = to_device(host[k:], device), to_device(host[ch], device), to_device(new[ch], device)
    rs.update(par, ch, old_t, new_t, col0=col0, ncols=ncols)
    assert_rows(par, want[k:], "update")
    assert_rows(old_t, host[ch], "old")
    par2, delta = to_device(host[k:], device), to_device(host[ch] ^ new[ch], device)
    rs.update_delta(par2, ch, delta, col0, ncols)
    assert_rows(par2, want[k:], "update_delta")
    stripe = to_device(host, device)
    want[ch, w] = new[ch][:, w]
    rs.write(stripe, ch, new_t, col0=col0, ncols=ncols)
    assert_rows(stripe, want, "write")
    assert_rows(new_t, new[ch], "new")
    assert_padding(par, old_t, new_t, par2, delta, stripe)


def case_default_window(device):
    """ncols defaults to the shortest row minus col0."""
    code, ch = (4, 6, "cauchy"), [2]
    rs, c = codec(code), 4101
    host, new = host_stripe(code, c), host_new(code, c)
    par, old_t = to_device(host[4:], device), to_device(host[ch], device)
    new_t = to_device(new[ch][:, :4000], device)  # the shortest row
    rs.update(par, ch, old_t, new_t, col0=33)
    want = np.array(host[4:])
    want[:, 33:4000] = expected_parity(code, c, (2,))[:, 33:4000]
    assert_rows(par, want)


def case_noop_and_composition(device, code, ncols):
    """old == new leaves the parity bit-identical; two successive updates equal the one combined."""
    rs, k = codec(code), code[0]
    host, new = host_stripe(code, ncols), host_new(code, ncols)
    par, old_t, same = to_device(host[k:], device), to_device(host[[1]], device), to_device(host[[1]], device)
    rs.update(par, [1], old_t, same)
    assert_rows(par, host[k:], "old == new")
    a, b = [0], [k - 1, 1]
    rs.update(par, a, to_device(host[a], device), to_device(new[a], device))
    rs.update(par, b, to_device(host[b], device), to_device(new[b], device))
    assert_rows(par, expected_parity(code, ncols, tuple(a + b)), "two updates")
    one = to_device(host[k:], device)
    rs.update(one, a + b, to_device(host[a + b], device), to_device(new[a + b], device))
    assert_rows(one, to_host(par), "combined")
    assert_padding(par, one)


def case_other_field(device, field, code=(4, 6, "cauchy"), ncols=4102):
    """gf16 / gf65536: the updated parity equals the codec's own CPU encode of the new natives."""
    k, n, matrix = code
    rs = ReedSolomon(k, n, matrix=matrix, field=field)
    rng = np.random.default_rng(n + ncols)
    data = rng.integers(0, 256, size=(k, ncols), dtype=np.uint8)
    new = rng.integers(0, 256, size=(k, ncols), dtype=np.uint8)
    parity = to_host(rs.encode(torch.from_numpy(data)))
    for ch in ([0], [k - 1, 0], list(range(k))):
        after = np.array(data)
        after[ch] = new[ch]
        want = to_host(rs.encode(torch.from_numpy(after)))
        for c0, nc in ((0, ncols), (18, 4000)):
            w = slice(c0, c0 + nc)
            expect = np.array(parity)
            expect[:, w] = want[:, w]
            par, old_t, new_t = to_device(parity, device), to_device(data[ch], device), to_device(new[ch], device)
            rs.update(par, ch, old_t, new_t, c0, nc)
            assert_rows(par, expect, (field, ch, "update"))
            par2 = to_device(parity, device)
            rs.update_delta(par2, ch, to_device(data[ch] ^ new[ch], device), c0, nc)
            assert_rows(par2, expect, (field, ch, "update_delta"))
            stripe = to_device(np.vstack([data, parity]), device)
            rs.write(stripe, ch, new_t, c0, nc)
            full = np.vstack([data, expect])
            full[ch, w] = new[ch][:, w]
            assert_rows(stripe, full, (field, ch, "write"))
            assert_padding(par, par2, stripe, old_t, new_t)


def case_refusals(device):
    """Each raises ValueError with every buffer unchanged."""
    code, c = (4, 6, "cauchy"), 4101
    rs, k = codec(code), 4
    host, new = host_stripe(code, c), host_new(code, c)
    stripe, new_t = to_device(host, device), to_device(new, device)
    par, nat = stripe[k:], stripe[:k]

    def refused(fn, *a, **kw):
        with pytest.raises(ValueError):
            fn(*a, **kw)
        assert_rows(stripe, host, "stripe after a refusal")
        assert_rows(new_t, new, "new after a refusal")

    for fn, first in ((rs.update, (par,)), (rs.update_delta, (par,)), (rs.write, (stripe,))):
        pair = fn == rs.update

        def rows(ids):  # the argument rows that go with `changed`
            ids = [j % k for j in ids]
            return ((nat[ids], new_t[ids]) if pair else (new_t[ids],))
        refused(fn, *first, [1, 1], *rows([1, 1]))           # duplicates
        refused(fn, *first, [k], *rows([0]))                 # an id equal to k
        refused(fn, *first, [-1], *rows([0]))
        refused(fn, *first, [], *rows([0])[:0], *([new_t[:0]] * (2 if pair else 1)))  # an empty changed
        refused(fn, *first, [1], *rows([1, 2]))              # row-count mismatch
        refused(fn, *first, [0, 1, 2, 3, 0], *rows([0, 1, 2, 3, 0]))  # more than k
        refused(fn, *first, [1], *rows([1]), c - 1, 2)       # a window past the rows
        refused(fn, *first, [1], *rows([1]), col0=-1)
        refused(fn, *first, [1], *rows([1]), col0=c + 1)
    refused(rs.update, par[:1], [1], nat[[1]], new_t[[1]])   # parity row count
    refused(rs.write, stripe[:5], [1], new_t[[1]])           # not n rows
    refused(rs.update, par, [1], nat[[1]], [par[0]])         # a parity row overlapping a new row
    refused(rs.update, par, [1], nat[[1]], [par[1][5:]])
    refused(rs.update_delta, par, [1], [par[1]])
    refused(rs.write, stripe, [1], [par[0]])
    refused(rs.update, [par[0], par[0]], [1], nat[[1]], new_t[[1]])   # two parity rows sharing memory
    refused(rs.update, [par[0], par[0][100:]], [1], nat[[1]], new_t[[1]])
    refused(rs.update, par, [1], [nat[1]], [nat[1]])       # new aliasing old
    refused(rs.write, stripe, [1], [nat[1]])
    refused(rs.write, stripe, [1, 2], [nat[2], nat[1]])
    refused(rs.update, par, [1], nat[[1]], new_t[[1]].to(torch.int8))  # dtype
    if device != "cpu":
        refused(rs.update, par, [1], nat[[1]], new_t[[1]].cpu())       # devices
        with pytest.raises(ValueError):
            UpdatePlan(par, nat[[1]], [par[0]], rs.E[:, [1]])
        with pytest.raises(ValueError):
            UpdatePlan(par, new_t[[1]], None, rs.E[:, [1]], store_new=True)
        assert_rows(stripe, host)
    assert_padding(stripe, new_t)


def case_no_parity(device):
    """p == 0: update is a no-op, write only copies (inside the window)."""
    rs = ReedSolomon(3, 3)
    rng = np.random.default_rng(3)
    data, new = rng.integers(0, 256, (3, 100), dtype=np.uint8), rng.integers(0, 256, (1, 100), dtype=np.uint8)
    stripe, new_t = to_device(data, device), to_device(new, device)
    empty = stripe[3:]
    assert rs.update(empty, [1], stripe[[1]], new_t) is empty
    rs.update_delta(empty, [1], new_t)
    assert_rows(stripe, data)
    rs.write(stripe, [1], new_t, col0=10, ncols=50)
    data[1, 10:60] = new[0, 10:60]
    assert_rows(stripe, data)
    assert_padding(stripe, new_t)


# ---- CPU tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,ncols,changed", FULL, ids=map(run_id, FULL))
def test_update_and_update_delta(code, ncols, changed):
    case_update("cpu", code, ncols, changed)


@pytest.mark.parametrize("code,ncols,changed", SHORT, ids=map(run_id, SHORT))
def test_write(code, ncols, changed):
    case_write("cpu", code, ncols, changed)


@pytest.mark.parametrize("col0,ncols", WINDOWS)
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=code_id)
def test_windows(code, col0, ncols):
    for changed in ((1,), tuple(range(code[0] - 1, -1, -1))[:9]):
        case_window("cpu", code, col0, ncols, changed)


def test_default_window():
    case_default_window("cpu")


@pytest.mark.parametrize("ncols", [15, 4101, 65536 + 3])
@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (19, 36, "cauchy")], ids=code_id)
def test_unaligned_rows(code, ncols):
    k = code[0]
    for changed in ((k - 1,), tuple(range(min(k, 9)))):
        case_update("cpu", code, ncols, changed, shift=1)
        case_write("cpu", code, ncols, changed, shift=1)
        case_update("cpu", code, ncols, changed, shift=0, shift_new=1)  # parity aligned, new not
        case_write("cpu", code, ncols, changed, shift=0, shift_new=1)


@pytest.mark.parametrize("code", [(4, 6, "cauchy"), (10, 14, "vandermonde"), (5, 10, "cauchy")], ids=code_id)
def test_same_contents_and_two_updates_in_a_row(code):
    case_noop_and_composition("cpu", code, 4101)


def test_gf16_field():
    case_other_field("cpu", "gf16")


def test_gf65536_field():
    case_other_field("cpu", "gf65536")
    rs = ReedSolomon(4, 6, field="gf65536")
    rows = torch.zeros((7, 64), dtype=torch.uint8)
    for c0, nc in ((1, 10), (2, 9)):
        with pytest.raises(ValueError, match="even"):
            rs.update(rows[4:6], [0], rows[:1], rows[6:], c0, nc)


def test_refusals():
    case_refusals("cpu")


def test_no_parity_rows():
    case_no_parity("cpu")


def test_update_oracle_is_the_delta_identity():
    code = (10, 14, "vandermonde")
    for changed in changed_lists(10):
        expected_parity(code, 257, changed)  # asserts oracle == encode of the new natives
    host = host_stripe(code, 257)
    assert np.array_equal(gf.update_oracle(codec(code).E, host[10:], [3], host[[3]], host[[3]]), host[10:])


def test_update_plan_is_exported_and_gpu_only():
    rows = torch.zeros((3, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        UpdatePlan(rows[:1], rows[1:2], rows[2:3], np.array([[1]], dtype=np.uint8))
