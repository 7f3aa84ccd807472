"""Helpers of the C API tests (tests/test_gpu_capi_plans.py, tests/test_capi.py): ctypes prototypes
of the ``gfrs_*`` functions they call, and guard-filled arenas in device, pinned and pageable host
memory. Every row a test hands to the library is a view of ONE buffer filled with ``GUARD``, with
at least ``PAD`` guard bytes after it, and the whole buffer is compared with a host image, so a
byte stored anywhere but where the oracle has one shows, as does an oracle byte that was not stored."""
import ctypes
import functools
import os

import numpy as np

from gpu_rscode_amd import _build, gf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lib", "libgfrs.so")

OK, EINVAL = 0, -1
AUTO, VALU, MFMA = 0, 1, 2
GUARD = 0xA5
PAD = 256  # guard bytes after every row, at least
HEAD = 4096  # guard bytes before the first row

_vpp = ctypes.POINTER(ctypes.c_void_p)
_i64, _int, _vp, _u8p = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p


@functools.lru_cache(maxsize=None)
def load() -> ctypes.CDLL:
    """lib/libgfrs.so with the prototypes of gfrs.h (built first when the tree's copy is stale)."""
    if _build.have_sources() and _build.stale(_build.Path(LIB)):
        _build.build("capi")
    lib = ctypes.CDLL(LIB)
    protos = {
        "gfrs_last_error": (ctypes.c_char_p, []),
        "gfrs_sync": (_int, [_int]),
        "gfrs_copy": (_int, [_vp, _vp, ctypes.c_size_t]),
        "gfrs_release": (_int, []),
        "gfrs_plan_create": (_int, [_vpp, _int, _int, _int, _u8p, _vpp, _vpp, _vpp, _i64, _int]),
        "gfrs_plan_set_coeff": (_int, [_vp, _u8p]),
        "gfrs_plan_run": (_int, [_vp, _vp]),
        "gfrs_plan_engine": (_int, [_vp]),
        "gfrs_plan_destroy": (None, [_vp]),
        "gfrs_plan16_create": (_int, [_vpp, _int, _int, _int, _vp, _vpp, _vpp, _vpp, _i64, _int]),
        "gfrs_plan16_destroy": (None, [_vp]),
        "gfrs_update_create": (_int, [_vpp, _int, _int, _int, _u8p, _vpp, _vpp, _vpp, _int]),
        "gfrs_update_run": (_int, [_vp, _i64, _i64, _vp]),
        "gfrs_update_destroy": (None, [_vp]),
        "gfrs_decoder_create": (_int, [_vpp, _int, _int, _int, _u8p, _vpp, _vpp, _i64, _int, _int]),
        "gfrs_decoder_rows": (_vp, [_vp]),
        "gfrs_decoder_solve": (_int, [_vp, _vp, _vp]),
        "gfrs_decoder_run": (_int, [_vp, _vp]),
        "gfrs_decoder_status": (_int, [_vp, _vp]),
        "gfrs_decoder_engine": (_int, [_vp]),
        "gfrs_decoder_destroy": (None, [_vp]),
        "gfrs_gemm_host": (_int, [ctypes.POINTER(_int), _int, _int, _int, _u8p, _vpp, _vpp, _i64, _int, _i64]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def err(lib) -> str:
    return (lib.gfrs_last_error() or b"").decode()


def ptr_array(addrs):
    """A C array of row addresses (0 = NULL)."""
    return (ctypes.c_void_p * max(1, len(addrs)))(*[int(a) or None for a in addrs])


def coeff_bytes(c: np.ndarray) -> bytes:
    return np.ascontiguousarray(c, dtype=np.uint8).tobytes()


def noise(seed, *shape) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def gemm_case(k: int, m: int, ncols: int, seed: int = 0):
    """(coeff [m, k], data [k, ncols], oracle [m, ncols]) of one shape: random bytes, with a zero and
    a one among the coefficients; computed once per shape and shared (read-only)."""
    rng = np.random.default_rng([k, m, ncols, seed])
    coeff = rng.integers(0, 256, size=(m, k), dtype=np.uint8)
    coeff[0, 0] = 0
    coeff[m - 1, k - 1] = 1
    data = rng.integers(0, 256, size=(k, ncols), dtype=np.uint8)
    want = gf.GF256.gemm(coeff, data).astype(np.uint8)
    for a in (coeff, data, want):
        a.setflags(write=False)
    return coeff, data, want


class Row:
    """``n`` bytes at ``off`` of an arena; ``ptr`` is what the library is given."""

    def __init__(self, arena, off: int, n: int):
        self.arena, self.off, self.n = arena, off, n
        self.ptr = arena.base + off

    def put(self, host) -> None:
        """Stores ``host`` in the row and in the image."""
        self.arena._store(self.off, np.ascontiguousarray(host, dtype=np.uint8))
        self.expect(host)

    def expect(self, host, col0: int = 0) -> None:
        """The image alone: what the row must hold after the call under test."""
        host = np.asarray(host, dtype=np.uint8)
        assert col0 + host.size <= self.n
        self.arena.image[self.off + col0: self.off + col0 + host.size] = host


class _ArenaBase:
    def __init__(self, nbytes: int):
        self.size = HEAD + nbytes + HEAD
        self.image = np.full(self.size, GUARD, dtype=np.uint8)
        self.cursor = HEAD

    def take(self, n: int, shift: int = 0, gap: int = 0) -> Row:
        """The next row of ``n`` bytes: ``shift`` bytes past a 256-byte boundary, at least
        ``PAD + gap`` guard bytes after it."""
        off = (self.cursor + 255) // 256 * 256 + shift
        self.cursor = off + n + PAD + gap
        assert self.cursor <= self.size - HEAD, "arena too small for its rows"
        return Row(self, off, n)

    def at(self, off: int, n: int) -> Row:
        """A row at a chosen offset (overlapping or closely spaced views); the caller keeps it inside."""
        assert HEAD <= off and off + n + PAD <= self.size - HEAD
        return Row(self, off, n)

    def rows(self, count: int, n: int, shift: int = 0):
        """``count`` rows at one stride."""
        return [self.take(n, shift) for _ in range(count)]

    def pitched(self, count: int, n: int, pitch: int, shift: int = 0):
        """``count`` rows exactly ``pitch`` bytes apart, the first ``shift`` past a 256-byte boundary."""
        assert pitch >= n + PAD
        first = (self.cursor + 255) // 256 * 256 + shift
        self.cursor = first + count * pitch
        assert self.cursor <= self.size - HEAD, "arena too small for its rows"
        return [Row(self, first + i * pitch, n) for i in range(count)]

    def scattered(self, count: int, n: int, seed: int = 0):
        """``count`` rows with gaps that differ (no common stride), listed in a shuffled order."""
        rows = [self.take(n, 0, 256 * ((5 * i + seed) % 3 + (i == 1))) for i in range(count)]
        order = np.random.default_rng(seed + count).permutation(count)
        return [rows[i] for i in order]

    def check(self, what: str = "") -> None:
        got = self._snapshot()
        if np.array_equal(got, self.image):
            return
        bad = np.flatnonzero(got != self.image)
        starts = bad[np.concatenate([[True], np.diff(bad) > 1])]
        runs = "; ".join(f"+{o} (got {got[o]:#04x}, want {self.image[o]:#04x})" for o in starts[:8].tolist())
        raise AssertionError(f"{what}: {bad.size} bytes of the arena differ from the oracle and the guard, in "
                             f"{starts.size} runs starting at {runs}")

    def snapshot(self) -> np.ndarray:
        """The buffer's bytes now (device arenas: after a synchronize)."""
        return self._snapshot()

    def region_equal(self, got: np.ndarray, row: Row, lo: int, hi: int) -> bool:
        """Columns [lo, hi) of one row of a snapshot against the image (to name the region that differs)."""
        return bool(np.array_equal(got[row.off + lo: row.off + hi], self.image[row.off + lo: row.off + hi]))


def arena_bytes(nrows: int, n: int, extra: int = 0) -> int:
    """Room for ``nrows`` rows of ``n`` bytes taken with any shift < 256 and the gaps of scattered()."""
    return nrows * ((n + 255) // 256 * 256 + PAD + 256 + 3 * 256) + extra


class DeviceArena(_ArenaBase):
    """Rows in one torch CUDA buffer (256-byte aligned base)."""

    def __init__(self, nbytes: int):
        import torch

        super().__init__(nbytes)
        self._torch = torch
        raw = torch.full((self.size + 256,), GUARD, dtype=torch.uint8, device="cuda")
        self.buf = raw[(-raw.data_ptr()) % 256:][: self.size]
        self.base = self.buf.data_ptr()

    def _store(self, off, host):
        self.buf[off: off + host.size].copy_(self._torch.from_numpy(np.array(host)))  # (a copy: host may be read-only)

    def _snapshot(self):
        self._torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def tensor(self, row: Row):
        return self.buf[row.off: row.off + row.n]


class HostArena(_ArenaBase):
    """Rows in one host buffer: pinned (``torch`` pinned memory) or pageable (numpy)."""

    def __init__(self, nbytes: int, pinned: bool):
        super().__init__(nbytes)
        if pinned:
            import torch

            self._keep = torch.empty(self.size + 256, dtype=torch.uint8).pin_memory()
            raw = self._keep.numpy()
        else:
            raw = np.empty(self.size + 256, dtype=np.uint8)
        self.buf = raw[(-raw.ctypes.data) % 256:][: self.size]
        self.buf[:] = GUARD
        self.base = self.buf.ctypes.data

    def _store(self, off, host):
        self.buf[off: off + host.size] = host

    def _snapshot(self):
        return self.buf
