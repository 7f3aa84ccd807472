"""Shared pieces of tests/test_stream_cases.py, tests/test_gpu_streams.py and tests/test_gpu_graphs.py:
one table entry per asynchronous entry point (everything that takes ``stream=``), and the harnesses
that run an entry behind a gate on a side stream and inside a captured graph.

An entry builds small inputs in a guard-filled arena (``capi_cases.DeviceArena`` / ``HostArena``),
knows how to make the call, which bytes the call writes and what they must be (numpy oracles of
``gf`` and ``engine_cases.oracle_gemm``; never the kernels), whether the call is documented to make
no host sync and whether it can be captured into a graph. The arena's host image is the oracle of
every byte: inputs, outputs, untouched rows and guards alike. Tensors a call returns (masks, status
words, matrices) are its "extras" and have oracles of their own.

Seeds: an entry derives all its data from one integer. ``STALE`` fills the arena before a gated call,
``REAL`` is what the gate copies in; replays of a graph use ``REPLAYS`` with one eager call (``EAGER``)
between the second and the third. Entries with a data-dependent outcome (a dirty stripe, a singular
pattern) make the even seeds the odd ones out, so a replay sequence goes clean, dirty, clean.

Nothing here touches a GPU unless a test passes ``device="cuda"``.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

import capi_cases as cc
import engine_cases as ec
import repair_solve_cases as rsc
from gpu_rscode_amd import ReedSolomon, gf
from gpu_rscode_amd.ops.matrix import encoding_matrix

F8 = gf.GF256
C = 4099                 # a few KiB with a ragged tail
C16 = 4098               # GF(2^16) rows hold whole symbols
CM = 3 * 256 + 77        # matrix-core rows
CM16 = 2 * CM
B = ec.BATCH             # stripes of the batched forms
BLOCK = 4096             # bytes per mask word: C spans two
STALE, REAL, WARM, EAGER = 3, 6, 9, 15
REPLAYS = (11, 12, 13)   # 12 is the odd one out (a flipped byte, a singular pattern)
GATE_MS, GATE_MIN_MS = 100.0, 50.0
ERASED4 = (3, 4, 7, 9)


def noise(seed, *shape) -> np.ndarray:
    return cc.noise([int(seed), len(shape)] + [int(s) for s in shape], *shape)


# ---- the arena: capi_cases' rows, as tensors -------------------------------------------------------------
class Arena:
    """A ``capi_cases`` arena on either device with its rows as torch views."""

    def __init__(self, device: str, nbytes: int):
        self.device = device
        if device == "cuda":
            self.a = cc.DeviceArena(nbytes)
            self.buf = self.a.buf
        else:
            self.a = cc.HostArena(nbytes, pinned=False)
            self.buf = torch.from_numpy(self.a.buf)
        self.image = self.a.image

    def upload(self, image: np.ndarray | None = None) -> None:
        self.buf.copy_(torch.from_numpy(np.array(self.image if image is None else image)).to(self.buf.device))

    def row(self, n: int, shift: int = 0):
        return self.a.take(n, shift)

    def tensor(self, row) -> torch.Tensor:
        return self.buf[row.off: row.off + row.n]


class Block:
    """``shape = (..., C)`` rows at one pitch (256-byte multiples, ``shift`` bytes off alignment) and
    their strided tensor view; ``put`` writes the host image only."""

    def __init__(self, arena: Arena, shape, shift: int = 0):
        self.shape = tuple(int(s) for s in shape)
        c = self.shape[-1]
        count = int(np.prod(self.shape[:-1]))
        pitch = (c + cc.PAD + 255) // 256 * 256
        self.rows = arena.a.pitched(count, c, pitch, shift)
        strides, s = [1], pitch
        for d in reversed(self.shape[1:-1]):
            strides.insert(0, s)
            s *= d
        strides.insert(0, s)
        self.t = arena.buf.as_strided(self.shape, strides[-len(self.shape):], self.rows[0].off)

    def put(self, host) -> None:
        host = np.asarray(host, dtype=np.uint8).reshape(len(self.rows), self.shape[-1])
        for r, x in zip(self.rows, host):
            r.expect(x)

    def fill(self, value: int) -> None:
        self.put(np.full(self.shape, value, dtype=np.uint8))

    def list(self):
        return [self.t[i] for i in range(self.shape[0])]


def block_bytes(*shapes) -> int:
    return sum(cc.arena_bytes(int(np.prod(s[:-1])), s[-1]) for s in shapes) + 4096


# ---- oracles ---------------------------------------------------------------------------------------------
def gemm8(coeff, data) -> np.ndarray:
    return F8.gemm(np.asarray(coeff, dtype=np.uint8), np.asarray(data, dtype=np.uint8)).astype(np.uint8)


def gemm16(coeff, data_u8) -> np.ndarray:
    """GF(2^16) GEMM on byte rows of little-endian symbols."""
    sym = np.ascontiguousarray(data_u8).view("<u2")
    out = ec.oracle_gemm(ec.field(16), coeff, sym)
    return np.ascontiguousarray(out.astype("<u2")).view(np.uint8).reshape(out.shape[0], -1)


def gemm(rs: ReedSolomon, coeff, data) -> np.ndarray:
    return gemm16(coeff, data) if rs.wide else gemm8(coeff, data)


def decode_rows(rs: ReedSolomon, rows, erased) -> np.ndarray:
    """Rows ``erased`` of inv(G[rows]) from the numpy field (not the C++ solve the codec uses)."""
    g = np.asarray(rs.G)[list(rows)]
    inv = ec.field(16).invert(g) if rs.wide else F8.invert(g)
    return np.asarray(inv)[list(erased)]


def consistent(rs: ReedSolomon, nstripes: int, ncols: int, seed: int) -> np.ndarray:
    """``[B, n, C]`` consistent stripes of the codec."""
    data = noise(seed, nstripes, rs.k, ncols)
    if rs.p == 0:
        return data
    flat = data.transpose(1, 0, 2).reshape(rs.k, -1)
    par = gemm(rs, rs.E, flat).reshape(rs.p, nstripes, ncols).transpose(1, 0, 2)
    return np.concatenate([data, par], axis=1)


def mask_oracle(h: np.ndarray, stripe: np.ndarray, block: int = BLOCK) -> np.ndarray:
    """int32 ``[ceil(C / block)]``: bit ``i % 32`` where row i of ``H . stripe`` is nonzero in the block."""
    p, ncols = h.shape[0], stripe.shape[1]
    nmask = -(-ncols // block)
    out = np.zeros(nmask, dtype=np.uint32)
    if p and ncols:
        s = gemm8(h, stripe)
        for i in range(p):
            for b in range(nmask):
                if s[i, b * block: (b + 1) * block].any():
                    out[b] |= np.uint32(1 << (i % 32))
    return out.view(np.int32)


_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def fill_random_oracle(nbytes: int, seed: int) -> np.ndarray:
    """The generator's definition: 16-byte group g holds splitmix64(seed ^ 2g) and splitmix64(seed ^
    (2g | 1)), little-endian; the tail bytes come from splitmix64(seed ^ 2 n16 ^ 0xABCD)."""
    n16, tail = divmod(nbytes, 16)
    words = []
    for g in range(n16):
        words += [_splitmix64(seed ^ (g << 1)), _splitmix64(seed ^ ((g << 1) | 1))]
    out = np.array(words, dtype="<u8").view(np.uint8)
    a = _splitmix64(seed ^ (n16 << 1) ^ 0xABCD)
    return np.concatenate([out, np.array([(a >> (8 * (t & 7))) & 0xFF for t in range(tail)], dtype=np.uint8)])


# ---- what an entry builds --------------------------------------------------------------------------------
@dataclass
class Built:
    """One entry's buffers on one device. ``fill(seed)`` writes the state before the call into the
    arena's image, ``expect(seed)`` moves the image to the state after it and returns ``(extras,
    host)``: the oracles of the tensors the call returns and of the host values it reports.
    ``call(stream)`` makes the call and returns the same pair. ``scramble``: resets device state the call
    must rebuild. ``poison``: bytes of a result that the call zero-fills with torch, not with a kernel:
    ``gated`` first fills a block of that size with 0xFF on the side stream and frees it."""
    arena: Arena
    fill: Callable
    expect: Callable
    call: Callable
    engine: Callable | None = None
    scramble: Callable | None = None
    poison: int = 0


@dataclass(frozen=True)
class Entry:
    name: str
    api: tuple               # qualified names of the entry points the call goes through
    build: Callable          # device -> Built
    nosync: bool             # documented to make no host sync on a cached call
    capture: bool            # graph-capturable on a cached call
    why: str = ""            # why it syncs / is not captured
    cpu: bool = True         # has a CPU form
    engine: str | None = None  # what ``plan.engine`` (and the FP4 form) must be on the GPU
    spellings: tuple = ("arg", "current")
    left_out: tuple = ()     # harnesses the entry is kept out of: "capture", "first"; ``why`` says why


ENTRIES: dict[str, Entry] = {}
SYNCS = "syncs once by design: the counts come back to the host"


def entry(name, api, nosync=True, capture=True, **kw):
    def deco(build):
        assert name not in ENTRIES, name
        ENTRIES[name] = Entry(name, tuple(api), build, nosync, capture, **kw)
        return build
    return deco


def _engines(rs: ReedSolomon):
    return lambda: sorted({p.engine for p in rs._plans.values() if hasattr(p, "engine")})


def _rs(k, n, fld="gf256", matrix="cauchy") -> ReedSolomon:
    return ReedSolomon(k, n, matrix=matrix, field=fld)


# ---- encode ----------------------------------------------------------------------------------------------
def _encode(name, form, k, n, ncols, fld="gf256", engine=None):
    @entry(name, ("ReedSolomon.encode", "GemmPlan.run" if fld == "gf256" else "Gemm16Plan.run"), engine=engine)
    def build(dev):
        rs = _rs(k, n, fld)
        a = Arena(dev, block_bytes((k, ncols), (n - k, ncols)))
        data, par = Block(a, (k, ncols)), Block(a, (n - k, ncols))

        def fill(seed):
            data.put(noise(seed, k, ncols))
            par.fill(0xAB)

        def expect(seed):
            par.put(gemm(rs, rs.E, noise(seed, k, ncols)))
            return [], {}

        def call(s):
            rs.encode(data.t if form == "2d" else data.list(), par.t, stream=s)
            return [], {}
        return Built(a, fill, expect, call, engine=_engines(rs))


_encode("encode_2d", "2d", 10, 14, C, engine="valu")
_encode("encode_rows", "rows", 10, 14, C, engine="valu")
_encode("encode_2d_mfma", "2d", 32, 40, CM, engine="mfma")
_encode("encode_rows_mfma", "rows", 32, 40, CM, engine="mfma")
_encode("encode_2d_gf65536", "2d", 10, 14, C16, "gf65536", engine="valu16")
_encode("encode_rows_gf65536", "rows", 10, 14, C16, "gf65536", engine="valu16")
_encode("encode_2d_gf65536_mfma", "2d", 20, 32, CM16, "gf65536", engine="mfma")


def _encode_batch(name, k, n, ncols, fld="gf256", engine=None):
    @entry(name, ("ReedSolomon.encode_batch", "GemmPlan.run" if fld == "gf256" else "Gemm16Plan.run"), engine=engine)
    def build(dev):
        rs = _rs(k, n, fld)
        a = Arena(dev, block_bytes((B, k, ncols), (B, n - k, ncols)))
        data, par = Block(a, (B, k, ncols)), Block(a, (B, n - k, ncols))

        def fill(seed):
            data.put(noise(seed, B, k, ncols))
            par.fill(0xAB)

        def expect(seed):
            par.put(consistent(rs, B, ncols, seed)[:, k:])
            return [], {}

        def call(s):
            rs.encode_batch(data.t, par.t, stream=s)
            return [], {}
        return Built(a, fill, expect, call, engine=_engines(rs))


_encode_batch("encode_batch", 10, 14, C, engine="valu")
_encode_batch("encode_batch_mfma", 128, 160, 3 * 256 + 50, engine="mfma")
_encode_batch("encode_batch_gf65536", 10, 14, C16, "gf65536", engine="valu16")
_encode_batch("encode_batch_gf65536_mfma", 20, 32, CM16, "gf65536", engine="mfma")


# ---- decode ----------------------------------------------------------------------------------------------
def _survivors(k, n, erased):
    return [i for i in range(n) if i not in erased][:k]


def _decode(name, k, n, ncols, erased, fld="gf256", device_invert=False, engine=None, capture=True):
    api = ["ReedSolomon.decode"]
    if erased:
        api.append("GemmPlan.run" if fld == "gf256" else "Gemm16Plan.run")
    if device_invert:
        api.append("decode_system_into_plan" if fld == "gf256" else "decode_system16_into_plan")

    @entry(name, api, engine=engine, capture=capture)
    def build(dev):
        rs = _rs(k, n, fld)
        rows = _survivors(k, n, erased) if erased else list(range(k))[::-1]
        a = Arena(dev, block_bytes((n, ncols), (k, ncols)))
        stripe, out = Block(a, (n, ncols)), Block(a, (k, ncols))

        def fill(seed):
            stripe.put(consistent(rs, 1, ncols, seed)[0])
            out.fill(0xCD)

        def expect(seed):
            full = consistent(rs, 1, ncols, seed)[0]
            want = full[:k].copy()
            if erased:  # the rebuilt rows from the numpy inverse, not from the stripe that was encoded
                want[list(erased)] = gemm(rs, decode_rows(rs, rows, erased), full[rows])
            out.put(want)
            return ([np.zeros(1, np.int32)] if device_invert and dev == "cuda" else []), {}

        def call(s):
            rs.decode([stripe.t[r] for r in rows], rows, out.t, stream=s, device_invert=device_invert)
            return ([rs.last_status.view(1)] if device_invert and dev == "cuda" else []), {}
        return Built(a, fill, expect, call, engine=_engines(rs))


_decode("decode_cached", 10, 14, C, ERASED4, engine="valu")
_decode("decode_pure_copy", 10, 14, C, ())
_decode("decode_device_invert", 10, 14, C, ERASED4, device_invert=True, engine="valu")
_decode("decode_device_invert_gf65536", 10, 14, C16, ERASED4, "gf65536", device_invert=True, engine="valu16")
_decode("decode_cached_gf65536", 10, 14, C16, ERASED4, "gf65536", engine="valu16")


def _decode_batch(name, k, n, ncols, erased, fld="gf256", engine=None):
    api = ["ReedSolomon.decode_batch"] + (["GemmPlan.run" if fld == "gf256" else "Gemm16Plan.run"] if erased else [])

    @entry(name, api, engine=engine)
    def build(dev):
        rs = _rs(k, n, fld)
        rows = _survivors(k, n, erased) if erased else list(range(k))[::-1]
        a = Arena(dev, block_bytes((B, k, ncols), (B, k, ncols)))
        surv, out = Block(a, (B, k, ncols)), Block(a, (B, k, ncols))

        def fill(seed):
            surv.put(consistent(rs, B, ncols, seed)[:, rows])
            out.fill(0xCD)

        def expect(seed):
            full = consistent(rs, B, ncols, seed)
            want = full[:, :k].copy()
            if erased:
                dm = decode_rows(rs, rows, erased)
                for b in range(B):
                    want[b, list(erased)] = gemm(rs, dm, full[b, rows])
            out.put(want)
            return [], {}

        def call(s):
            rs.decode_batch(surv.t, rows, out.t, stream=s)
            return [], {}
        return Built(a, fill, expect, call, engine=_engines(rs))


_decode_batch("decode_batch", 10, 14, C, ERASED4, engine="valu")
_decode_batch("decode_batch_no_native_erased", 10, 14, C, ())
_decode_batch("decode_batch_mfma", 128, 160, 3 * 256 + 50, tuple(range(5, 128, 8)), engine="mfma")
_decode_batch("decode_batch_gf65536", 10, 14, C16, ERASED4, "gf65536", engine="valu16")


# ---- reconstruct -----------------------------------------------------------------------------------------
def _reconstruct(name, device_solve):
    api = ["ReedSolomon.reconstruct", "GemmPlan.run"] + (["solve_patterns"] if device_solve else [])

    @entry(name, api, engine="valu")
    def build(dev):
        rs, erased = _rs(10, 14), [2, 9, 12]
        a = Arena(dev, block_bytes((14, C)))
        stripe = Block(a, (14, C))

        def fill(seed):
            stripe.put(rsc.damage(consistent(rs, 1, C, seed), [erased])[0])

        def expect(seed):
            stripe.put(consistent(rs, 1, C, seed)[0])
            return [], {}

        def call(s):
            rs.reconstruct(stripe.t, erased, stream=s, device_solve=device_solve)
            return [], {}
        return Built(a, fill, expect, call, engine=_engines(rs))


_reconstruct("reconstruct", False)
_reconstruct("reconstruct_device_solve", True)
BATCH_ERASED = [[1, 12], [0, 3, 5, 13], []]


def _reconstruct_batch(name, device_solve):
    api = ["ReedSolomon.reconstruct_batch", "BatchRepairPlan.run"] + (["solve_patterns"] if device_solve else [])

    @entry(name, api)
    def build(dev):
        rs = _rs(10, 14)
        a = Arena(dev, block_bytes((B, 14, C)))
        stripes = Block(a, (B, 14, C))

        def fill(seed):
            stripes.put(rsc.damage(consistent(rs, B, C, seed), BATCH_ERASED))

        def expect(seed):
            stripes.put(consistent(rs, B, C, seed))
            return [], {}

        def call(s):
            rs.reconstruct_batch(stripes.t, BATCH_ERASED, stream=s, device_solve=device_solve)
            return [], {}
        return Built(a, fill, expect, call)


_reconstruct_batch("reconstruct_batch", False)
_reconstruct_batch("reconstruct_batch_device_solve", True)


# ---- scrub: syndrome_mask (asynchronous) and the calls that report to the host -----------------------------
def _dirty(seed) -> bool:
    return seed % 2 == 0


def _syndrome(name, k, n, ncols, batched):
    api = ["ReedSolomon.syndrome_mask_batch" if batched else "ReedSolomon.syndrome_mask"]
    if n > k and ncols:
        api.append("ScrubBase.syndrome_mask")

    kw = {}
    if batched and n > k and ncols > 0:
        kw = dict(left_out=("capture", "first"),
                  why="not covered under capture: a replayed graph returned non-zero mask bytes on clean stripes")

    @entry(name, api, **kw)
    def build(dev):
        rs = _rs(k, n)
        nb = B if batched else 1
        a = Arena(dev, block_bytes((nb, n, ncols)))
        stripes = Block(a, (nb, n, ncols))
        nmask = -(-ncols // BLOCK)

        def host(seed):
            s = consistent(rs, nb, ncols, seed)
            if _dirty(seed) and ncols:
                s[nb - 1, 2, ncols - 2] ^= 0x40
            return s

        def fill(seed):
            stripes.put(host(seed))

        def expect(seed):
            s = host(seed)
            m = np.stack([mask_oracle(rs.H, s[b]) for b in range(nb)]).reshape(nb, nmask)
            return [m if batched else m[0]], {}

        def call(s):
            if batched:
                return [rs.syndrome_mask_batch(stripes.t, block_bytes=BLOCK, stream=s)], {}
            return [rs.syndrome_mask(stripes.t[0], block_bytes=BLOCK, stream=s)], {}
        # (no kernel writes the p = 0 masks: they are zero-filled by torch, and must not merely be zero already.
        # With zero columns nmask == 0: the mask has no element, and the case checks its shape and the arena only)
        return Built(a, fill, expect, call, poison=0 if n > k else 4 * nb * nmask)


_syndrome("syndrome_mask", 10, 14, C, False)
_syndrome("syndrome_mask_batch", 10, 14, C, True)
_syndrome("syndrome_mask_p0", 4, 4, C, False)
_syndrome("syndrome_mask_batch_p0", 4, 4, C, True)
_syndrome("syndrome_mask_batch_zero_columns", 10, 14, 0, True)


def _plant(rs, nb, ncols, seed, chunks):
    """Consistent stripes and the same with one wrong byte in each of ``chunks`` of the last stripe, at
    columns of their own (both mask blocks)."""
    good = consistent(rs, nb, ncols, seed)
    bad = good.copy()
    for t, j in enumerate(chunks):
        bad[nb - 1, j, (seed * 37 + t * 2053) % ncols] ^= 0x11 * (t + 1)
    return good, bad


def _report(name, method, batched, chunks, heals, api, erased=(), spellings=("arg", "current")):
    @entry(name, api, nosync=False, capture=False, why=SYNCS, spellings=spellings)
    def build(dev):
        rs = _rs(10, 14)
        nb = B if batched else 1
        a = Arena(dev, block_bytes((nb, 14, C)))
        stripes = Block(a, (nb, 14, C))

        def fill(seed):
            bad = _plant(rs, nb, C, seed, chunks)[1]
            stripes.put(rsc.damage(bad, [list(erased)] * nb))

        def expect(seed):
            good, bad = _plant(rs, nb, C, seed, chunks)
            if heals:
                stripes.put(good)
            cols = np.zeros(nb, dtype=np.int64)
            cols[nb - 1] = len(chunks)
            want = {"bad_columns": cols.tolist() if batched else int(cols[0])}
            if method.startswith("heal"):  # the second scrub's report
                want = {"bad_columns": [0] * nb if batched else 0}
            return [], want

        def call(s):
            kw = {} if method.startswith("heal") else {"stream": s, "block_bytes": BLOCK}
            args = (list(erased),) if erased else ()
            rep = getattr(rs, method)(stripes.t if batched else stripes.t[0], *args, **kw)
            return [], {"bad_columns": np.asarray(rep.bad_columns).tolist() if batched else int(rep.bad_columns)}
        return Built(a, fill, expect, call)


_report("scrub", "scrub", False, (5,), False, ("ReedSolomon.scrub", "ScrubBase.scrub", "ScrubBase.syndrome_mask"))
_report("scrub_batch", "scrub_batch", True, (5,), False,
        ("ReedSolomon.scrub_batch", "ScrubBase.scrub", "ScrubBase.syndrome_mask"))
# (heal and heal_batch take no stream: they run on the current one)
_report("heal", "heal", False, (5,), True, ("ReedSolomon.heal",), spellings=("current",))
_report("heal_batch", "heal_batch", True, (5,), True, ("ReedSolomon.heal_batch",), spellings=("current",))
_report("correct", "correct", False, (0, 6, 13), True, ("ReedSolomon.correct", "_Correct.correct"))
_report("correct_batch", "correct_batch", True, (0, 6, 13), True, ("ReedSolomon.correct_batch", "_Correct.correct"))
_report("reconstruct_checked", "reconstruct_checked", False, (5,), True,
        ("ReedSolomon.reconstruct_checked", "_CheckedRepair.run"), erased=(1, 11))
_report("reconstruct_checked_batch", "reconstruct_checked_batch", True, (5,), True,
        ("ReedSolomon.reconstruct_checked_batch", "_CheckedRepair.run"), erased=(1, 11))


# ---- partial-stripe writes -------------------------------------------------------------------------------
CHANGED = [7, 2]
CHANGED_B = np.array([[7, 2], [0, 9], [4, 1]], dtype=np.int64)
WINDOW = (1001, 2050)  # col0 off 16-byte alignment: the byte form of the window


def _windowed(old, new, win):
    if win is None:
        return new
    out = old.copy()
    out[..., win[0]: win[0] + win[1]] = new[..., win[0]: win[0] + win[1]]
    return out


def _update(name, form, k, n, win=None, shift=0):
    method = {"pair": "update", "delta": "update_delta", "write": "write"}[form]
    api = ["ReedSolomon." + method] + (["_Update.run"] if n > k else [])

    @entry(name, api)
    def build(dev):
        rs = _rs(k, n)
        p, d = n - k, len(CHANGED)
        ch = [c % k for c in CHANGED]
        a = Arena(dev, block_bytes((n, C), (d, C), (d, C)))
        stripe, first, new = Block(a, (n, C), shift), Block(a, (d, C), shift), Block(a, (d, C), shift)
        kw = {} if win is None else {"col0": win[0], "ncols": win[1]}

        def parts(seed):
            full = consistent(rs, 1, C, seed)[0]
            fresh = noise(seed + 1000, d, C)
            data2 = full[:k].copy()
            data2[ch] = _windowed(full[ch], fresh, win)
            after = np.concatenate([data2, _windowed(full[k:], gemm(rs, rs.E, data2), win)]) if p else data2
            return full, fresh, after

        def fill(seed):
            full, fresh, _ = parts(seed)
            stripe.put(full)
            first.put(full[ch] ^ fresh if form == "delta" else full[ch])
            new.put(fresh)

        def expect(seed):
            full, _, after = parts(seed)
            stripe.put(after if form == "write" else np.concatenate([full[:k], after[k:]]))
            return [], {}

        def call(s):
            par = stripe.t[k:]
            if form == "pair":
                rs.update(par, ch, first.t, new.t, stream=s, **kw)
            elif form == "delta":
                rs.update_delta(par, ch, first.t, stream=s, **kw)
            else:
                rs.write(stripe.t, ch, new.t, stream=s, **kw)
            return [], {}
        return Built(a, fill, expect, call)


for _f, _m in (("pair", "update"), ("delta", "update_delta"), ("write", "write")):
    _update(_m, _f, 10, 14)
    _update(_m + "_window", _f, 10, 14, WINDOW)
    _update(_m + "_byte_form", _f, 10, 14, None, 1)
_update("update_p0", "pair", 4, 4)
_update("write_p0", "write", 4, 4)
_update("write_p0_window", "write", 4, 4, WINDOW)


def _update_batch(name, form, win=None, shift=0):
    method = {"pair": "update_batch", "delta": "update_delta_batch", "write": "write_batch"}[form]

    @entry(name, ("ReedSolomon." + method, "_Update.run"))
    def build(dev):
        rs, k, n, d = _rs(10, 14), 10, 14, CHANGED_B.shape[1]
        a = Arena(dev, block_bytes((B, n, C), (B, d, C), (B, d, C)))
        stripes, first, new = Block(a, (B, n, C), shift), Block(a, (B, d, C), shift), Block(a, (B, d, C), shift)
        kw = {} if win is None else {"col0": win[0], "ncols": win[1]}
        pick = (np.arange(B)[:, None], CHANGED_B)

        def parts(seed):
            full = consistent(rs, B, C, seed)
            fresh = noise(seed + 1000, B, d, C)
            after = full.copy()
            after[pick] = _windowed(full[pick], fresh, win)
            for b in range(B):
                after[b, k:] = _windowed(full[b, k:], gemm(rs, rs.E, after[b, :k]), win)
            return full, fresh, after

        def fill(seed):
            full, fresh, _ = parts(seed)
            stripes.put(full)
            first.put(full[pick] ^ fresh if form == "delta" else full[pick])
            new.put(fresh)

        def expect(seed):
            full, _, after = parts(seed)
            stripes.put(after if form == "write" else np.concatenate([full[:, :k], after[:, k:]], axis=1))
            return [], {}

        def call(s):
            par = stripes.t[:, k:]
            if form == "pair":
                rs.update_batch(par, CHANGED_B, first.t, new.t, stream=s, **kw)
            elif form == "delta":
                rs.update_delta_batch(par, CHANGED_B, first.t, stream=s, **kw)
            else:
                rs.write_batch(stripes.t, CHANGED_B, new.t, stream=s, **kw)
            return [], {}
        return Built(a, fill, expect, call)


for _f, _m in (("pair", "update_batch"), ("delta", "update_delta_batch"), ("write", "write_batch")):
    _update_batch(_m, _f)
    _update_batch(_m + "_window", _f, WINDOW)
    _update_batch(_m + "_byte_form", _f, None, 1)


# ---- the GEMM engines a plan can pick, through the plan classes --------------------------------------------
def _gemm_plan8(name, engine, k, m, ncols, plan_engine, run_kw=None, shift=0, copies=True, scattered=False, form=None):
    @entry(name, ("GemmPlan.run",), cpu=False, engine=plan_engine + ("/" + form if form else ""))
    def build(dev):
        from gpu_rscode_amd.ops import GemmPlan

        coeff = noise(engine_seed(name), m, k)
        a = Arena(dev, block_bytes((k, ncols), (m, ncols), (k, ncols)) + 4 * 256 * k)
        ins = a.a.scattered(k, ncols, 7) if scattered else Block(a, (k, ncols), shift).rows
        out, dst = Block(a, (m, ncols), shift), Block(a, (k, ncols), shift)
        cps = [dst.t[j] if j % 2 else None for j in range(k)] if copies else None
        plan = GemmPlan([a.tensor(r) for r in ins], out.list(), coeff, copies=cps, engine=plan_engine)
        assert plan.bytewise == bool(shift)

        def fill(seed):
            for r, x in zip(ins, noise(seed, k, ncols)):
                r.expect(x)
            out.fill(0xAB)
            dst.fill(0x44)

        def expect(seed):
            data = noise(seed, k, ncols)
            out.put(gemm8(coeff, data))
            if copies:
                for j in range(1, k, 2):
                    dst.rows[j].expect(data[j])
            return [], {}

        def call(s):
            plan.run(s, **(run_kw or {}))
            return [], {}
        return Built(a, fill, expect, call, engine=lambda: [plan.engine + ("/" + plan.fp4_form if form else "")])


def engine_seed(name: str) -> int:
    return sum(name.encode()) + 1


for _e, (_k, _m, _, _) in sorted(ec.ENGINES8.items()):
    if _e == "vec":
        _gemm_plan8("gemm8_vec", _e, _k, _m, C, "valu", dict(vec=2, pf=2, nt=True))
    elif _e == "valu_wide":
        _gemm_plan8("gemm8_valu_wide", _e, _k, _m, C, "valu")
    elif _e.startswith("rows"):
        _gemm_plan8("gemm8_" + _e.replace("-", "m"), _e, _k, _m, C, "valu",
                    dict(vec=1, pf=int(_e.rsplit("pf", 1)[1]), nt=True))
    elif _e == "byte":
        _gemm_plan8("gemm8_byte", _e, _k, _m, C, "valu", shift=1)
    elif _e == "lut":
        _gemm_plan8("gemm8_lut", _e, _k, _m, C, "lut")
    elif _e == "mfma_i8":
        _gemm_plan8("gemm8_mfma_i8", _e, _k, _m, CM, "mfma_i8", copies=False)
    elif _e.startswith("mfma_"):
        _gemm_plan8("gemm8_" + _e, _e, _k, _m, CM, "mfma", scattered=True, form=_e[5:])
    # (the batched forms run through encode_batch / decode_batch above, v_perm and matrix cores)


def _gemm_plan16(name, k, m, ncols, plan_engine, shift=0):
    @entry(name, ("Gemm16Plan.run",), cpu=False, engine=plan_engine)
    def build(dev):
        from gpu_rscode_amd.ops import Gemm16Plan

        coeff = ec.random_symbols(16, m, k, engine_seed(name)).astype(np.int64)
        a = Arena(dev, block_bytes((k, ncols), (m, ncols), (k, ncols)))
        x, out, dst = Block(a, (k, ncols), shift), Block(a, (m, ncols), shift), Block(a, (k, ncols), shift)
        cps = [dst.t[j] if j % 2 else None for j in range(k)]
        plan = Gemm16Plan(x.list(), out.list(), coeff, copies=cps, engine=plan_engine)
        assert plan.symwise == bool(shift)

        def fill(seed):
            x.put(noise(seed, k, ncols))
            out.fill(0xAB)
            dst.fill(0x44)

        def expect(seed):
            data = noise(seed, k, ncols)
            out.put(gemm16(coeff, data))
            for j in range(1, k, 2):
                dst.rows[j].expect(data[j])
            return [], {}

        def call(s):
            plan.run(s)
            return [], {}
        return Built(a, fill, expect, call, engine=lambda: [plan.engine])


_gemm_plan16("gemm16_valu16", *ec.ENGINES16["valu16_g1"][:2], C16, "valu16")
_gemm_plan16("gemm16_sym", *ec.ENGINES16["sym"][:2], C16, "valu16", shift=2)
_gemm_plan16("gemm16_mfma", *ec.ENGINES16["mfma"][:2], CM16, "mfma")


def _device_coeff(name, wide):
    cls = "Gemm16Plan" if wide else "GemmPlan"

    @entry(name, (cls + ".set_device_coeff", cls + ".run"), cpu=False, engine="mfma")
    def build(dev):
        from gpu_rscode_amd.ops import Gemm16Plan, GemmPlan

        k, m = ec.ENGINES16["mfma"][:2] if wide else ec.ENGINES8["mfma_v1"][:2]
        ncols, w = (CM16, 2) if wide else (CM, 1)
        a = Arena(dev, block_bytes((k, ncols), (m, ncols), (m, k * w)))
        x, out, cf = Block(a, (k, ncols)), Block(a, (m, ncols)), Block(a, (m, k * w))
        if wide:
            coeff0 = ec.random_symbols(16, m, k, engine_seed(name))
            plan = Gemm16Plan(x.t, out.t, coeff0.astype(np.int64), engine="mfma")
            cf_t = cf.t.view(torch.int16)
        else:
            coeff0 = noise(engine_seed(name), m, k)
            plan = GemmPlan(x.t, out.t, coeff0, engine="mfma")
            cf_t = cf.t
        coeff_bytes = np.ascontiguousarray(coeff0.astype("<u2")).view(np.uint8).reshape(m, -1) if wide else coeff0

        def fill(seed):
            # the coefficients are an input of the call, read on its stream: stale ones differ. The
            # plan's v_perm tables (the kernels' column remainder) hold the real ones throughout.
            x.put(noise(seed, k, ncols))
            out.fill(0xAB)
            cf.put(noise(seed, m, k * w) if seed == STALE else coeff_bytes)

        def expect(seed):
            data = noise(seed, k, ncols)
            out.put(gemm16(coeff0, data) if wide else gemm8(coeff0, data))
            return [], {}

        def call(s):
            plan.set_device_coeff(cf_t, stream=s)
            plan.run(s)
            return [], {}
        return Built(a, fill, expect, call, engine=lambda: [plan.engine], scramble=lambda: plan.bitmat.zero_())


_device_coeff("set_device_coeff_run", False)
_device_coeff("set_device_coeff_run_gf65536", True)


@entry("set_coeff_run", ("GemmPlan.set_coeff", "GemmPlan.run"), nosync=False, capture=False, cpu=False,
       why="uploads host-built tables: a blocking copy from pageable memory", engine="valu")
def _set_coeff(dev):
    from gpu_rscode_amd.ops import GemmPlan

    k, m = 10, 4
    coeff = noise(77, m, k)
    a = Arena(dev, block_bytes((k, C), (m, C)))
    x, out = Block(a, (k, C)), Block(a, (m, C))
    plan = GemmPlan(x.t, out.t, noise(78, m, k), engine="valu")

    def fill(seed):
        x.put(noise(seed, k, C))
        out.fill(0xAB)

    def expect(seed):
        out.put(gemm8(coeff, noise(seed, k, C)))
        return [], {}

    def call(s):
        plan.set_coeff(coeff, stream=s)
        plan.run(s)
        return [], {}
    return Built(a, fill, expect, call, engine=lambda: [plan.engine])


@entry("gf_gemm", ("gf_gemm", "GemmPlan.run"), nosync=False, capture=False, cpu=False,
       why="builds its plan on every call: a blocking descriptor upload")
def _gf_gemm(dev):
    from gpu_rscode_amd.ops import gf_gemm

    k, m = 10, 4
    coeff = noise(79, m, k)
    a = Arena(dev, block_bytes((k, C), (m, C)))
    x, out = Block(a, (k, C)), Block(a, (m, C))

    def fill(seed):
        x.put(noise(seed, k, C))
        out.fill(0xAB)

    def expect(seed):
        out.put(gemm8(coeff, noise(seed, k, C)))
        return [], {}

    def call(s):
        gf_gemm(coeff, x.t, out.t, stream=s)
        return [], {}
    return Built(a, fill, expect, call)


# ---- device solves ---------------------------------------------------------------------------------------
def _matrices(seed, nb, n):
    """``nb`` random n x n matrices, the last one singular (two equal rows)."""
    m = noise(seed, nb, n, n)
    m[nb - 1, n - 1] = m[nb - 1, 0]
    return m


@entry("gf_invert", ("gf_invert",), cpu=False)
def _gf_invert(dev):
    from gpu_rscode_amd.ops import gf_invert

    nb, n = 4, 16
    a = Arena(dev, block_bytes((nb, n, n)))
    mats = Block(a, (nb, n, n))  # (pitched rows: the call's contiguous copy is part of what is ordered)
    t = mats.t

    def fill(seed):
        mats.put(_matrices(seed, nb, n))

    def expect(seed):
        inv, status = np.zeros((nb, n, n), np.uint8), np.zeros(nb, np.int32)
        for b, m in enumerate(_matrices(seed, nb, n)):
            try:
                inv[b] = F8.invert(m)
            except gf.SingularMatrixError:
                status[b] = 1
        assert status[nb - 1] == 1
        return [inv, status], {}

    def call(s):
        out, status = gf_invert(t, check=False, stream=s)
        return [out, status], {}
    return Built(a, fill, expect, call)


@entry("invert_into_plan_run", ("invert_into_plan", "GemmPlan.run"), cpu=False, engine="valu")
def _invert_into_plan(dev):
    from gpu_rscode_amd.ops import GemmPlan, invert_into_plan

    k, sel = 10, [3, 4, 7, 9]
    a = Arena(dev, block_bytes((k, C), (len(sel), C)) + cc.arena_bytes(3, 256))
    x, out = Block(a, (k, C)), Block(a, (len(sel), C))
    mat, ids, st = a.row(k * k), a.row(4 * len(sel)), a.row(4)
    plan = GemmPlan(x.t, out.t, device_tables=True, engine="valu")
    ids_t, st_t = a.tensor(ids).view(torch.int32), a.tensor(st).view(torch.int32)
    rs = _rs(10, 14)

    def system(seed):  # survivors' rows of a Cauchy generator: always invertible
        rows = _survivors(10, 14, [(seed + i) % 10 for i in (0, 3, 5, 8)])
        return np.asarray(rs.G)[rows]

    def fill(seed):
        x.put(noise(seed, k, C))
        out.fill(0xAB)
        mat.expect(system(seed).reshape(-1))
        ids.expect(np.array(sel, dtype="<i4").view(np.uint8))
        st.expect(np.full(4, 0xEE, np.uint8))

    def expect(seed):
        out.put(gemm8(F8.invert(system(seed))[sel], noise(seed, k, C)))
        st.expect(np.zeros(4, np.uint8))
        return [], {}

    def call(s):
        invert_into_plan(a.tensor(mat).view(k, k), plan, ids_t, status=st_t, stream=s)
        plan.run(s)
        return [], {}
    return Built(a, fill, expect, call, engine=lambda: [plan.engine])


def singular4() -> tuple:
    """A four-erasure pattern of the reference Vandermonde (10, 14) whose default survivors are singular
    (all such patterns lose three natives and one parity chunk)."""
    return next(er for er in rsc.vandermonde_singular() if len(er) == 4)


def _pattern_decoder(name, matrix, fld, ncols, engine):
    wide = fld == "gf65536"
    solve = "decode_system16_into_plan" if wide else "decode_system_into_plan"

    @entry(name, ("PatternDecoder.solve", "PatternDecoder.run", solve, ("Gemm16Plan" if wide else "GemmPlan") + ".run"),
           cpu=False, engine=engine)
    def build(dev):
        from gpu_rscode_amd.ops import PatternDecoder

        k, n = 10, 14
        rs = _rs(k, n, fld, matrix)
        good = [ERASED4, (0, 1, 5, 8), (2, 6, 7, 9)]
        if matrix == "vandermonde":  # three natives and a parity chunk, as its singular patterns
            good = [er for er in [(3, 4, 7, 13), (0, 5, 8, 11), (2, 6, 9, 12), (1, 4, 8, 13)]
                    if rsc.host_coeff((k, n, matrix), rsc.first_survivors(n, k, er), er) is not None]
            assert len(good) >= 2 and sum(i < k for i in singular4()) == 3
        e = sum(i < k for i in good[0])
        a = Arena(dev, block_bytes((n, ncols), (k, ncols)) + cc.arena_bytes(1, 256))
        stripe, out = Block(a, (n, ncols)), Block(a, (k, ncols))
        pat = a.row(4 * k)
        g = np.ascontiguousarray(rs.G, dtype="<u2").view(np.int16) if wide else np.ascontiguousarray(rs.G)
        dec = PatternDecoder(torch.from_numpy(g).to(dev), stripe.list(), out.list(), e)
        pat_t = a.tensor(pat).view(torch.int32)

        def erased(seed):
            if matrix == "vandermonde" and seed == REPLAYS[1]:
                return singular4(), True
            return good[seed % len(good)], False

        def fill(seed):
            stripe.put(consistent(rs, 1, ncols, seed)[0])
            out.fill(0xCD)
            pat.expect(np.array(_survivors(k, n, erased(seed)[0]), dtype="<i4").view(np.uint8))

        def expect(seed):
            er, singular = erased(seed)
            if singular:  # status 1, nothing stored
                return [np.ones(1, np.int32)], {}
            full = consistent(rs, 1, ncols, seed)[0]
            rows = _survivors(k, n, er)
            want = full[:k].copy()
            lost = [i for i in er if i < k]
            want[lost] = gemm(rs, decode_rows(rs, rows, lost), full[rows])
            out.put(want)
            return [np.zeros(1, np.int32)], {}

        def call(s):
            dec.solve(s, rows=pat_t)
            dec.run(s)
            return [dec.status], {}
        return Built(a, fill, expect, call, engine=lambda: [dec.engine])


_pattern_decoder("pattern_decoder", "cauchy", "gf256", C, "valu")
_pattern_decoder("pattern_decoder_vandermonde_singular", "vandermonde", "gf256", C, "valu")
_pattern_decoder("pattern_decoder_gf65536", "cauchy", "gf65536", C16, "valu16")


@entry("solve_patterns", ("solve_patterns",), cpu=False)
def _solve_patterns(dev):
    from gpu_rscode_amd.ops.gemm import pad_m
    from gpu_rscode_amd.ops.repair import solve_patterns

    code = (10, 14, "cauchy")
    k, n = code[:2]
    pats = [[(1, 12), (0, 3, 5, 13)], [(2, 9), (4, 6, 10, 11)], [(13,), (0, 1, 2, 3)]]
    m_pad = pad_m(4)
    npat = 2
    a = Arena(dev, cc.arena_bytes(3, npat * m_pad * k))
    sv_r, er_r, co_r = a.row(4 * npat * k), a.row(4 * npat * m_pad), a.row(npat * m_pad * k)
    g_dev = torch.from_numpy(np.ascontiguousarray(rsc.codec(*code).G)).to(dev)
    sv_t = a.tensor(sv_r).view(torch.int32).view(npat, k)
    er_t = a.tensor(er_r).view(torch.int32).view(npat, m_pad)

    def ids(seed):
        ers = pats[seed % len(pats)]
        return [rsc.first_survivors(n, k, er) for er in ers], ers

    def fill(seed):
        sv, er = rsc.id_arrays(*ids(seed), m_pad)
        sv_r.expect(sv.astype("<i4").view(np.uint8).reshape(-1))
        er_r.expect(er.astype("<i4").view(np.uint8).reshape(-1))
        co_r.expect(np.full(npat * m_pad * k, 0xEE, np.uint8))

    def expect(seed):
        svs, ers = ids(seed)
        co_r.expect(np.concatenate([rsc.coeff_block(rsc.host_coeff(code, s, e), k, m_pad).reshape(-1)
                                    for s, e in zip(svs, ers)]))
        return [np.zeros(npat, np.int32)], {}

    def call(s):
        return [solve_patterns(g_dev, sv_t, er_t, m_pad, coeff_out=a.tensor(co_r), stream=s)], {}
    return Built(a, fill, expect, call)


# ---- generators ------------------------------------------------------------------------------------------
@entry("fill_random_", ("fill_random_",), cpu=False)
def _fill_random(dev):
    from gpu_rscode_amd.ops import fill_random_

    a = Arena(dev, cc.arena_bytes(1, C))
    row = a.row(C)

    def fill(seed):
        row.expect(np.full(C, 0xAB, np.uint8))

    def expect(seed):
        row.expect(fill_random_oracle(C, 12345))
        return [], {}

    def call(s):
        fill_random_(a.tensor(row), 12345, stream=s)
        return [], {}
    return Built(a, fill, expect, call)


def _gen_matrix(kind):
    @entry("gen_matrix_device_" + kind, ("gen_matrix_device",), cpu=False)
    def build(dev):
        from gpu_rscode_amd.ops import gen_matrix_device

        k, p = 10, 4
        a = Arena(dev, 4096)

        def call(s):
            return [gen_matrix_device(kind, k, p, device=dev, stream=s)], {}
        return Built(a, lambda seed: None, lambda seed: ([encoding_matrix(kind, k, p)], {}), call)


_gen_matrix("vandermonde")
_gen_matrix("cauchy")


# ---- completeness: every entry point that takes a stream ---------------------------------------------------
def stream_api() -> set:
    """Qualified names of every public callable with a ``stream`` parameter: the methods of
    ``ReedSolomon`` and of the classes ``gpu_rscode_amd.ops`` exports (named after the class that
    defines them), the functions it exports, and ``ops.repair.solve_patterns``."""
    import inspect

    from gpu_rscode_amd import ops
    from gpu_rscode_amd.ops.repair import solve_patterns

    def takes_stream(fn) -> bool:
        try:
            return "stream" in inspect.signature(fn).parameters
        except (TypeError, ValueError):
            return False

    found = set()
    things = [ReedSolomon, solve_patterns] + [getattr(ops, name) for name in ops.__all__]
    for obj in things:
        if inspect.isclass(obj):
            for name, fn in inspect.getmembers(obj, inspect.isfunction):
                if not name.startswith("_") and takes_stream(fn):
                    found.add(fn.__qualname__)
        elif callable(obj) and takes_stream(obj):
            found.add(obj.__qualname__)
    return found


def covered_api() -> set:
    return {name for e in ENTRIES.values() for name in e.api}


def doc_rows() -> list[tuple]:
    """(entry, entry points, no host sync, capturable) as docs/API.md lists them."""
    return [(e.name, ", ".join(e.api), "yes" if e.nosync else "no",
             "yes" if e.capture and "capture" not in e.left_out else "no") for e in ENTRIES.values()]


def doc_table() -> str:
    lines = ["| Case | Entry points | No host sync | Graph-capturable |", "|---|---|---|---|"]
    lines += [f"| `{n}` | {', '.join('`' + x + '`' for x in api.split(', '))} | {s} | {c} |" for n, api, s, c in doc_rows()]
    return "\n".join(lines)


# ---- comparing ---------------------------------------------------------------------------------------------
def compare(what: str, got_arena: np.ndarray, want_arena: np.ndarray, extras, want_extras, host, want_host) -> None:
    if not np.array_equal(got_arena, want_arena):
        bad = np.flatnonzero(got_arena != want_arena)
        starts = bad[np.concatenate([[True], np.diff(bad) > 1])]
        runs = "; ".join(f"+{o} (got {got_arena[o]:#04x}, want {want_arena[o]:#04x})" for o in starts[:6].tolist())
        raise AssertionError(f"{what}: {bad.size} bytes of the arena differ from the oracle and the guard, in "
                             f"{starts.size} runs starting at {runs}")
    assert len(extras) == len(want_extras), (what, len(extras), len(want_extras))
    for i, (g, w) in enumerate(zip(extras, want_extras)):
        g = np.asarray(g)
        assert g.shape == np.asarray(w).shape, (what, "result", i, g.shape, np.asarray(w).shape)
        assert np.array_equal(g.astype(np.int64), np.asarray(w).astype(np.int64)), (what, "result", i, g, w)
    assert host == want_host, (what, host, want_host)


def run_plain(e: Entry, device: str, seed: int = REAL) -> None:
    """The entry's call on the current stream, everything compared with the oracle."""
    b = e.build(device)
    b.fill(seed)
    b.arena.upload()
    extras, host = b.call(None)
    want_extras, want_host = b.expect(seed)
    if device == "cuda":
        torch.cuda.synchronize()
    compare(e.name, b.arena.buf.cpu().numpy(), b.arena.image, [x.cpu().numpy() for x in extras], want_extras, host,
            want_host)


# ---- the gate (GPU) ----------------------------------------------------------------------------------------
_state: dict = {}


def streams():
    """The two streams beside the default one that a process uses: (side, other)."""
    if "streams" not in _state:
        _state["streams"] = (torch.cuda.Stream(), torch.cuda.Stream())
    return _state["streams"]


def gate_cycles() -> int:
    """``torch.cuda._sleep`` cycles for a gate of GATE_MS, from one timed call per process."""
    if "cycles" not in _state:
        probe = 20_000_000
        torch.cuda._sleep(1000)  # (load the kernel)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        torch.cuda._sleep(probe)
        t1.record()
        t1.synchronize()
        ms = max(t0.elapsed_time(t1), 1e-3)
        _state["cycles_per_ms"] = probe / ms
        _state["cycles"] = int(probe / ms * GATE_MS * 1.2)
        print(f"torch.cuda._sleep: {probe} cycles took {ms:.2f} ms: {probe / ms:.0f} cycles per ms")
    return _state["cycles"]


def check_engine(e: Entry, b: Built) -> None:
    if e.engine is not None and b.engine is not None:
        got = b.engine()
        assert got == [e.engine], (e.name, "engine", got, e.engine)


def gated(e: Entry, spelling: str, first: bool = False, fault: str | None = None) -> None:
    """The entry's call behind a gate on the side stream: a long sleep, then the copies that replace
    the stale arena with the real inputs. The call is made while the gate is pending, a snapshot of the
    arena and of the results is enqueued behind it on the side stream, and everything is compared
    with the oracle of the real inputs. ``first``: no call before the gate (the plan's first call; it
    builds a plan, whose descriptor upload blocks the host, so "no host sync" is asserted for cached
    calls only).
    ``fault``: a planted fault the harness must catch ("stream": the call goes to another stream,
    "sync": the side stream is synchronised before the call returns)."""
    side, other = streams()
    cycles = gate_cycles()
    b = e.build("cuda")
    a = b.arena
    b.fill(STALE)
    stale = a.image.copy()
    b.fill(REAL)
    staging = torch.from_numpy(a.image.copy()).cuda()
    want_extras, want_host = b.expect(REAL)
    a.upload(stale)
    if not first:
        b.call(None)
        a.upload(stale)
    if b.scramble is not None:
        b.scramble()
    if b.poison:
        # The side stream's allocator block of the result's size holds 0xFF before the call, so a mask
        # that reads zero on the side stream was zero-filled, not left as found. The fill is complete
        # before the block is freed. (This cannot show a zero-fill issued on the default stream when
        # ``stream=side`` is passed: that block comes from the default stream's pool and is filled at once.)
        with torch.cuda.stream(side):
            block = torch.full((b.poison,), 0xFF, dtype=torch.uint8, device="cuda")
        side.synchronize()
        del block
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enqueued = time.perf_counter()
    with torch.cuda.stream(side):
        t0.record()
        torch.cuda._sleep(cycles)
        a.buf.copy_(staging, non_blocking=True)
        t1.record()

    def call(s):
        if fault == "stream":
            return b.call(other)
        out = b.call(s)
        if fault == "sync":
            side.synchronize()
        return out
    if spelling == "arg":
        extras, host = call(side)
    else:
        with torch.cuda.stream(side):
            extras, host = call(None)
    # an event recorded right after the call returns, and the gate's own end: a call that had
    # synchronised with the side stream would have waited for the gate, and both would be complete
    returned = torch.cuda.Event()
    returned.record(side)
    pending = not returned.query() and not t1.query()
    with torch.cuda.stream(side):
        snap = a.buf.clone()
        extras = [x.clone() for x in extras]
    side.synchronize()
    wall = (time.perf_counter() - enqueued) * 1e3
    took = t0.elapsed_time(t1)
    torch.cuda.synchronize()
    # (see the module docstring of tests/test_gpu_streams.py: a short gate has been seen once)
    assert took >= GATE_MIN_MS, (f"the gate lasted {took:.1f} ms by its events, under {GATE_MIN_MS} ms ({cycles} cycles; "
                                 f"{wall:.1f} ms passed on the host from enqueuing it to the end of the side stream)")
    what = f"{e.name} ({spelling}{', first call' if first else ''})"
    compare(what, snap.cpu().numpy(), a.image, [x.cpu().numpy() for x in extras], want_extras, host, want_host)
    if e.nosync and not first:
        assert pending, f"{what}: the call waited for the gate ({took:.0f} ms): it made a host sync"
    check_engine(e, b)


# ---- graph capture (GPU) -----------------------------------------------------------------------------------
def captured(e: Entry, spelling: str, fault: bool = False, fresh_plan: bool = False) -> None:
    """A warm-up call, the call captured once on the side stream, three replays on fresh data of a
    seed each (compared with the oracle, whole arena included) and one eager call on the same buffers
    between the second and the third. ``fault``: the planted fault (the call runs before the capture,
    the graph holds a fill of a scratch tensor only). ``fresh_plan``: no warm-up call, for entries that
    build their plan beforehand: the plan's wait for its ready event then falls inside the capture."""
    side, _ = streams()
    b = e.build("cuda")
    a = b.arena

    def load(seed):
        b.fill(seed)
        before = a.image.copy()
        want = b.expect(seed)
        a.upload(before)
        if b.scramble is not None:
            b.scramble()
        return want

    def check(what, extras, host, want):
        torch.cuda.synchronize()
        compare(f"{e.name} ({spelling}, {what})", a.buf.cpu().numpy(), a.image, [x.cpu().numpy() for x in extras],
                want[0], host, want[1])

    if not fresh_plan:
        want = load(WARM)
        check("warm-up", *b.call(None), want)
    load(STALE)
    scratch = torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    if fault:
        extras, host = b.call(None)
        torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        if fault:
            scratch.fill_(1)
        else:
            extras, host = b.call(side if spelling == "arg" else None)
    for i, seed in enumerate(REPLAYS):
        want = load(seed)
        g.replay()
        check(f"replay {i}", extras, host, want)
        if i == 1:
            want = load(EAGER)
            check("eager call between replays", *b.call(None), want)
    check_engine(e, b)
