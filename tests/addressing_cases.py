"""Shared pieces of tests/test_gpu_addressing.py: where in memory the bytes are.

A plan stores raw row pointers, so the k "rows" of a case are overlapping views of ONE device buffer
a little over 4 GiB long, and the outputs and fused-copy destinations of a windowed run
``plan.run(col0=c0, ncols=n)`` are overlapping views of one buffer each: row i starts ``W`` bytes
after row i - 1, only ``[c0, c0 + n)`` of each is written, and ``W >= n + 256`` keeps those windows
apart. Three buffers serve every case of every engine.

The expected bytes of a window come from the numpy oracle on the window's input columns; whole rows
longer than 2^32 bytes are compared on the device with a torch-only table reference
(:func:`torch_gemm_chunks`), which a CPU test pins to the oracle.
"""
from __future__ import annotations

import numpy as np
import torch

from gpu_rscode_amd import gf
from gpu_rscode_amd.gf import GF256

P31, P32 = 1 << 31, 1 << 32
L8 = P32 + 256 * 9 + 77  # row length of the windowed cases, GF(2^8)
L16 = L8 - 1             # ... GF(2^16): whole symbols
WHOLE8 = P32 + 16 * 1000 + 11  # row length of the whole-row cases
WHOLE16 = WHOLE8 - 1
S_UNI = 4112             # uniform input stride (16 x 257)
W = 2816                 # output / copy row stride: a multiple of 256, >= the longest window + 256
K_MAX, M_MAX = 300, 40
IN_BYTES = L8 + K_MAX * S_UNI + 16
OUT_BYTES = L8 + M_MAX * W
CPY_BYTES = L8 + K_MAX * W
FILL_OUT, FILL_CPY = 0x5A, 0x44
SEED = 0x5EED0ADD
CHUNK = 32 << 20         # bytes per step of the torch reference (its int64 indices: 8 x that)
GIB16 = 16 << 30

# ragged lengths: a v_perm / partial-chunk remainder after the whole 256- or 1024-byte chunks
WIN_A = (P31 - 256 * 3 - 2, 256 * 8 + 78)  # across 2^31 (start 2 mod 4, 14 mod 16)
WIN_B = (P32 - 256 * 5, 256 * 9 + 76)      # across 2^32
WIN_D_BEFORE, WIN_D_LEN = 256 * 4 + 48, 256 * 8 + 78  # around a 2^32 multiple of the absolute address
assert W % 256 == 0 and W >= max(WIN_A[1], WIN_B[1], WIN_D_LEN) + 256


def win_c(length: int) -> tuple[int, int]:
    """The window wholly above 2^32: from 2^32 + 528 to the end of the row."""
    return P32 + 528, length - (P32 + 528)


def crossing_window(row: torch.Tensor) -> tuple[int, int]:
    """A window of ``row`` whose absolute addresses cross a multiple of 2^32 (at column
    ``(-data_ptr) % 2^32``, WIN_D_BEFORE bytes into the window)."""
    x = (-int(row.data_ptr())) % P32
    for cross in (x, x + P32):
        c0 = cross - WIN_D_BEFORE
        if cross > 0 and c0 >= 0 and c0 + WIN_D_LEN <= row.numel():
            assert (row.data_ptr() + c0) >> 32 != (row.data_ptr() + c0 + WIN_D_LEN - 1) >> 32
            return c0, WIN_D_LEN
    raise AssertionError(f"row at {row.data_ptr():#x} has no 2^32 crossing a window fits around")


# ---- references -------------------------------------------------------------------------------------
class _MemoGF(gf.GF):
    """``gf.GF`` whose per-coefficient table is kept: ``gemm`` is the oracle's own code, and a wide
    GF(2^16) code drawn from a pool of coefficients (:func:`coeff16`) costs one table per pool entry
    instead of one per matrix entry (k = 300, m = 40: 13 s of tables otherwise)."""

    def __init__(self, w: int):
        super().__init__(w)
        self._tables: dict[int, np.ndarray] = {}

    def mul_table(self, c: int) -> np.ndarray:
        t = self._tables.get(c)
        if t is None:
            t = self._tables[c] = super().mul_table(c)
        return t


F16 = _MemoGF(16)


def oracle(field: int, coeff: np.ndarray, rows_u8: np.ndarray) -> np.ndarray:
    """Expected output bytes (m, n) of the (k, n) input bytes."""
    rows_u8 = np.ascontiguousarray(rows_u8)
    if field == 8:
        return GF256.gemm(coeff, rows_u8)
    return np.ascontiguousarray(F16.gemm(coeff, rows_u8.view("<u2")).astype("<u2")).view(np.uint8)


def coeff8(m: int, k: int, seed: int) -> np.ndarray:
    c = np.random.default_rng(seed).integers(0, 256, size=(m, k), dtype=np.uint8)
    c[0, : min(k, 2)] = [0, 1][: min(k, 2)]
    return c


def coeff16(m: int, k: int, seed: int) -> np.ndarray:
    """(m, k) GF(2^16) coefficients from a pool of 128 values (0 and 1 among them)."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([[0, 1], rng.integers(2, 65536, size=126)])
    c = pool[rng.integers(0, pool.size, size=(m, k))]
    c[0, : min(k, 2)] = [0, 1][: min(k, 2)]
    return c


def mul_tables(field: int, coeff: np.ndarray, device) -> dict[int, torch.Tensor]:
    """c -> the table x -> c * x on ``device``: GF(2^8) rows of the 256 x 256 product table taken
    from ``GF256`` (uint8), GF(2^16) one 65,536-entry table per coefficient from ``gf.field(16)``
    (the uint16 values held in int16)."""
    f = GF256 if field == 8 else gf.field(16)
    out = {}
    for c in sorted({int(v) for v in np.asarray(coeff).reshape(-1)}):
        t = np.ascontiguousarray(f.mul_table(c))
        out[c] = torch.from_numpy(t if field == 8 else t.view(np.int16)).to(device)
    return out


def torch_gemm_chunks(field: int, coeff: np.ndarray, rows: list[torch.Tensor], chunk: int = CHUNK):
    """Torch-only GF-GEMM of k byte rows, ``chunk`` bytes at a time: yields ``(start, end, ref)``
    with ``ref`` the (m, end - start) uint8 output bytes. Every product is one table lookup indexed
    with ``x.long()`` (GF(2^16): the little-endian symbols), XORed over j."""
    coeff = np.asarray(coeff)
    m, k = coeff.shape
    n = min(r.numel() for r in rows)
    assert field in (8, 16) and len(rows) == k and (field == 8 or (n % 2 == 0 and chunk % 2 == 0))
    tabs = mul_tables(field, coeff, rows[0].device)
    dt = torch.uint8 if field == 8 else torch.int16
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        acc = torch.zeros((m, (e - s) * 8 // field), dtype=dt, device=rows[0].device)
        for j in range(k):
            x = rows[j][s:e]
            idx = x.long() if field == 8 else x.view(torch.int16).long() & 0xFFFF
            for i in range(m):
                acc[i] ^= tabs[int(coeff[i, j])][idx]
            del idx
        yield s, e, acc.view(torch.uint8)


def whole_row_mismatches(field: int, coeff, rows, outs, chunk: int = CHUNK) -> tuple[int, int]:
    """(mismatching bytes, first chunk start with one or -1) of ``outs`` against the torch reference
    over the whole rows; one host sync, at the end."""
    bad, starts = [], []
    for s, e, ref in torch_gemm_chunks(field, coeff, rows, chunk):
        got = torch.stack([o[s:e] for o in outs])
        bad.append((got != ref).sum())
        starts.append(s)
    counts = torch.stack(bad).cpu().numpy()
    nz = np.nonzero(counts)[0]
    return int(counts.sum()), (starts[int(nz[0])] if nz.size else -1)


def first_other(buf: torch.Tensor, value: int) -> int:
    """Offset of the first byte of ``buf`` that is not ``value`` (-1: none). One compare over 64-bit
    words, the scratch an eighth of the buffer."""
    n8 = buf.numel() // 8 * 8
    pat = int.from_bytes(bytes([value]) * 8, "little", signed=True)
    if buf.data_ptr() % 8 == 0:
        dirty = bool(((buf[:n8].view(torch.int64) != pat).any() | (buf[n8:] != value).any()).item())
        if not dirty:
            return -1
    step = 256 << 20
    for s in range(0, buf.numel(), step):
        nz = torch.nonzero(buf[s : s + step] != value)
        if nz.numel():
            return s + int(nz[0].item())
    return -1


# ---- the three buffers ------------------------------------------------------------------------------
class Buffers:
    """The input, output and copy buffers of the module (about 4.3 GiB each), made on first use and
    given back on :meth:`release` (before a subprocess makes its own)."""

    NEED = IN_BYTES + OUT_BYTES + CPY_BYTES + (3 << 29)  # + the scratch of the checks

    def __init__(self):
        self.big = self.out = self.cpy = None

    def acquire(self) -> str | None:
        """None when the buffers are there; otherwise why not (too little free device memory)."""
        if self.big is not None:
            return None
        from gpu_rscode_amd.ops import fill_random_

        assert self.NEED <= GIB16
        free, _ = torch.cuda.mem_get_info()
        if free < self.NEED:
            return f"needs {self.NEED >> 20} MiB of device memory, {free >> 20} MiB are free"
        self.big = torch.empty(IN_BYTES, dtype=torch.uint8, device="cuda")
        fill_random_(self.big, SEED)
        self.out = torch.empty(OUT_BYTES, dtype=torch.uint8, device="cuda")
        self.cpy = torch.empty(CPY_BYTES, dtype=torch.uint8, device="cuda")
        return None

    def release(self) -> None:
        self.big = self.out = self.cpy = None
        torch.cuda.empty_cache()

    def fill(self) -> None:
        self.out.fill_(FILL_OUT)
        self.cpy.fill_(FILL_CPY)

    def assert_untouched(self, what) -> None:
        """Both buffers hold nothing but their fill value (the written windows put back first)."""
        for name, buf, v in (("output", self.out, FILL_OUT), ("copy", self.cpy, FILL_CPY)):
            at = first_other(buf, v)
            assert at < 0, f"{what}: {name} buffer written outside its windows, first at byte {at} ({at:#x})"


def in_offsets(k: int, layout: str, base: int = 0) -> list[int]:
    """Start of input row j in the big buffer: ``base + j * S_UNI`` ("uniform"), or rows dealt to
    shuffled 4112-byte slots with an irregular 16-byte-aligned shift each ("scattered")."""
    if layout == "uniform":
        return [base + j * S_UNI for j in range(k)]
    assert layout == "scattered" and 3 <= k <= K_MAX
    rng = np.random.default_rng(k)
    slots, shift = rng.permutation(K_MAX)[:k], rng.integers(0, 64, size=k)
    return [base + int(s) * S_UNI + 16 * int(t) for s, t in zip(slots, shift)]


def window_case(bufs: Buffers, make_plan, *, k: int, m: int, field: int = 8, layout: str = "uniform",
                in_base: int = 0, copy_rows=(), run=None, shift: int = 0, check_plan=None, seed: int = 0,
                only=None):
    """One engine configuration over every window: (a) across 2^31, (b) across 2^32, (c) above 2^32,
    and (d) around a 2^32 multiple of the absolute address of an input row, of an output row and
    (with copies) of a copy row. ``make_plan(inputs, outputs, coeff, copies)`` builds the plan,
    ``run(plan, c0, n)`` launches it (default ``plan.run(col0=c0, ncols=n)``); ``shift`` moves every
    window start up by that many bytes (the same end); ``only`` names the windows to run (default all). Outputs and copies are bit-exact against the
    oracle inside the window, and the whole output and copy buffers keep their fill outside it."""
    length = L8 if field == 8 else L16
    offs = in_offsets(k, layout, in_base)
    assert max(offs) + length <= IN_BYTES and m <= M_MAX and k <= K_MAX
    ins = [bufs.big[o : o + length] for o in offs]
    outs = [bufs.out[i * W : i * W + length] for i in range(m)]
    copies = [bufs.cpy[j * W : j * W + length] if j in copy_rows else None for j in range(k)] if copy_rows else None
    coeff = (coeff8 if field == 8 else coeff16)(m, k, 1000 * k + m + seed)
    plan = make_plan(ins, outs, coeff, copies)
    assert plan.ncols == length
    if check_plan is not None:
        check_plan(plan)
    wins = [("a", WIN_A), ("b", WIN_B), ("c", win_c(length)), ("d-in", crossing_window(ins[k // 2])),
            ("d-out", crossing_window(outs[m // 2]))]
    if copy_rows:
        wins.append(("d-copy", crossing_window(copies[sorted(copy_rows)[len(copy_rows) // 2]])))
    bufs.fill()
    for name, (c0, n) in wins:
        if only is not None and name not in only:
            continue
        c0, n = c0 + shift, n - shift
        assert 0 <= c0 and c0 + n <= length and n <= W - 256
        if run is None:
            plan.run(col0=c0, ncols=n)
        else:
            run(plan, c0, n)
        torch.cuda.synchronize()
        host_in = torch.stack([r[c0 : c0 + n] for r in ins]).cpu().numpy()
        got = torch.stack([o[c0 : c0 + n] for o in outs]).cpu().numpy()
        want = oracle(field, coeff, host_in)
        assert np.array_equal(got, want), (name, c0, n, np.argwhere(got != want)[:4].tolist())
        for o in outs:
            o[c0 : c0 + n] = FILL_OUT
        if copies is not None:
            for j in sorted(copy_rows):
                assert np.array_equal(copies[j][c0 : c0 + n].cpu().numpy(), host_in[j]), (name, "copy", j)
                copies[j][c0 : c0 + n] = FILL_CPY
        bufs.assert_untouched((name, c0, n))
    return plan


def rows_kernel_windows(bufs: Buffers) -> None:
    """The rows-in-flight kernel (k = 10, 4-row tiles) over every window; which of its two forms
    runs is GFRS_TUNE=rows_lat_groups' choice (small launches: the latency form by default)."""
    from gpu_rscode_amd.ops import GemmPlan

    window_case(bufs, lambda i, o, c, cp: GemmPlan(i, o, c), k=10, m=4)


def rows_throughput_main() -> None:
    """Subprocess body of the throughput-form case (the threshold is read once per process)."""
    bufs = Buffers()
    why = bufs.acquire()
    if why:
        print("ADDR-SKIP " + why)
        return
    rows_kernel_windows(bufs)
    print(f"ADDR-OK peak={torch.cuda.max_memory_allocated()}")
