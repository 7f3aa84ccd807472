"""Reed-Solomon erasure codec — the framework's "model".

A systematic (k, n) code over GF(2^8): generator ``G = [I_k; E]`` with ``E`` (p x k, p = n - k)
from the reference Vandermonde (default, bit-compatible with ``src/matrix.cu:752-759``) or an MDS
construction. Encode is one GF-GEMM ``parity = E . data``; decode inverts the k x k rows of G that
survived and applies only the rows for erased natives, copying surviving natives in the same pass
(the reference multiplies the full k x k inverse, ``src/matrix.cu:838-905``).

Tensors: chunk rows are uint8 byte rows, either a 2-D ``[rows, C]`` tensor (use
:func:`alloc_rows` to get 256-byte-pitched storage so every row is 16-byte aligned even for odd C)
or a list of 1-D tensors. CUDA tensors run the gfx950 kernels; CPU tensors run the C++ codec.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Sequence

import numpy as np
import torch

from .. import gf
from .._native import cpu, hip
from ..ops.checked import (BatchCheckedRepairPlan, CheckedRepairPlan, check_checked_max_errors, check_erased,
                           cpu_reconstruct_checked)
from ..ops.correct import (BatchCorrectPlan, BatchCorrectReport, CorrectPlan, CorrectReport, check_disjoint,
                           check_max_errors, cpu_correct, make_batch_correct_report)
from ..ops.gemm import Gemm16Plan, GemmPlan
from ..ops.inverse import decode16_device_supported, decode_system16_into_plan, decode_system_into_plan
from ..ops.matrix import decode_matrix, encoding_matrix
from ..ops.rows import PickPart, StripeBatch, as_rows, batch_part, check_parts, null, stripe_rows, window
from ..ops.scrub import (MAX_LOCATE_P, BatchScrubPlan, BatchScrubReport, ScrubPlan, ScrubReport, check_block_bytes,
                         cpu_scrub, make_batch_report)
from ..ops.update import (BatchUpdatePlan, UpdatePlan, batch_ids, check_overlap, check_overlap_batch,
                          cpu_update)

PITCH = 256


def alloc_rows(rows: int, ncols: int, device="cuda", fill: int | None = None) -> torch.Tensor:
    """A [rows, ncols] uint8 view over storage whose row pitch is a multiple of 256 bytes
    (:func:`row_pitch`; large device rows start on 2 MiB boundaries)."""
    pitch = row_pitch(ncols, device)
    align = (2 << 20) if pitch % (2 << 20) == 0 else 0
    base = torch.empty(rows * pitch + align, dtype=torch.uint8, device=device)
    off = (-base.data_ptr()) % align if align else 0
    if fill is not None:
        base.fill_(fill)
    return base.as_strided((rows, ncols), (pitch, 1), off)


def flat_rows(t: torch.Tensor) -> torch.Tensor:
    """The bytes of an :func:`alloc_rows` tensor's rows, pitch padding included, as one 1-D view
    (from the tensor's own storage offset: the rows may start past the allocation's first byte)."""
    return t.as_strided((t.shape[0] * t.stride(0),), (1,))


def _row_align() -> int:
    from ..utils.tune import tune_int

    a = tune_int("row_align", 2 << 20)
    # a power of two of at least 256 (rows stay 16-byte aligned), else the default
    return a if a >= PITCH and (a & (a - 1)) == 0 else 2 << 20


def row_pitch(ncols: int, device="cuda") -> int:
    """Row pitch of :func:`alloc_rows`: ``ncols`` rounded up to 256 bytes (every row 16-byte
    aligned for odd C), and for device rows of at least 8 MiB up to 2 MiB, with the first row on a
    2 MiB boundary. Measured on MI355X (``scripts/membench.hip pitch``,
    ``profiles/headline/r07_pitch``): the k=10 encode pattern (10 rows in, 4 out) streams at
    6.26 TB/s with 2 MiB-aligned rows against 5.93 at 256-byte pitch, the decode pattern (10 in,
    10 out) at 5.77 against 5.33 — the rows' placement in HBM's channel interleave, not the kernel.
    ``GFRS_TUNE=row_align=N`` (bytes, power of two, 256 = the old layout) overrides the large-row
    alignment."""
    p = max(PITCH, (ncols + PITCH - 1) // PITCH * PITCH)
    if torch.device(device).type == "cuda" and ncols >= (8 << 20):
        a = max(PITCH, _row_align())
        p = (ncols + a - 1) // a * a
        p += _row_skew(p)
    return p


def _row_skew(p: int) -> int:
    """Extra pitch for large rows whose 2 MiB-aligned pitch is a multiple of 64 MiB: a quarter of the
    pitch (rounded to 2 MiB). At such a pitch every row's byte x sits at the same offset of a large
    power-of-two block, and the k rows of a stripe stream into the same HBM channels together.
    Measured on MI355X (scripts/membench.hip k16, profiles/headline/r09_k16): 16 rows of 512 MiB
    stream the decode pattern (16 in, 16 out) at 5.35 TB/s with a 512 MiB pitch and 6.41 with 640,
    the encode pattern (16 in, 4 out) at 5.38 / 5.54; 128 MiB rows 4.87 -> 5.36 (decode) at 160, 1 GiB
    rows 4.98 -> 6.15 at 1280. The k16n20_8g step: 5.01-5.02 -> 4.68-4.70 ms (8 MiB: 4.89, 64 MiB:
    4.78-4.80). Rows of the other BASELINE configs (104 MiB, 262 MiB, 8 MiB pitches) are not
    multiples of 64 MiB and keep their pitch. GFRS_TUNE=row_skew=BYTES fixes the skew (0: none)."""
    from ..utils.tune import tune_int

    if p % (64 << 20):
        return 0
    skew = tune_int("row_skew", -1)
    if skew < 0:
        return (p // 4) // (2 << 20) * (2 << 20)
    return skew if skew % (2 << 20) == 0 else 0


class UnrecoverableError(gf.SingularMatrixError):
    """The surviving chunks do not determine the data (singular decode system)."""


class _PlanCache(OrderedDict):
    """Plans keyed by (op, buffers, pattern), least recently used evicted past ``capacity``. The
    plans hold no references to the buffers (``hold_buffers=False``): a key names the exact row
    pointers, so a hit only happens for the caller's live tensors, and a loop over fresh buffers
    does not keep up to ``capacity`` generations of them allocated. A hit runs the plan unexamined, so
    a key names everything the plan was built from: pointer, shape and strides of every tensor (or
    pointer and length of every row), inputs and outputs alike, the ids and the options (docs/API.md;
    tests/test_gpu_plan_cache.py tries each with two calls at one base pointer). A hit
    must never turn into a rebuild while a caller relies on the plan: a hipGraph capture of
    ``encode_batch`` after 64 per-object ``encode`` calls used to miss because the old cache was
    cleared wholesale past 64 entries (and building a plan uploads a descriptor, which a capturing
    stream refuses)."""

    def __init__(self, capacity: int = 512):
        super().__init__()
        self.capacity = capacity

    def get(self, key, default=None):
        if key in self:
            self.move_to_end(key)
            return self[key]
        return default

    def __setitem__(self, key, value):
        super().__setitem__(key, value)
        self.move_to_end(key)
        while len(self) > self.capacity:
            self.popitem(last=False)


class ReedSolomon:
    """(k, n) Reed-Solomon codec.

    Args:
        k: native (data) chunks. n: total chunks (k + parity).
        matrix: ``"vandermonde"`` (reference, not MDS — SURVEY §2.2), ``"cauchy"`` or
            ``"sys_vandermonde"`` (both MDS).
        field: ``"gf256"`` (bytes are GF(2^8) symbols), ``"gf16"`` (the design doc's GF(16)
            method: each byte is two GF(2^4) symbols; needs n <= 16) or ``"gf65536"`` (GF(2^16),
            poly 0x1100B, ``src/galoisfield.cu:22-32``: rows hold little-endian 16-bit symbols, so
            row lengths are even byte counts; n <= 65535).
        cpu_strategy / cpu_threads: multiply strategy and threads of the C++ CPU path.
    """

    def __init__(self, k: int, n: int, matrix: str = "vandermonde", field: str = "gf256",
                 cpu_strategy: str = "simd", cpu_threads: int = 1):
        if not (1 <= k <= n):
            raise ValueError("need 1 <= k <= n")
        self.k, self.n, self.p = k, n, n - k
        self.matrix, self.field = matrix, field
        self.cpu_strategy, self.cpu_threads = cpu_strategy, cpu_threads
        if field == "gf256":
            if n > 256:
                raise ValueError("GF(2^8) codes need n <= 256")
            self.gf = gf.GF256
            self.E = encoding_matrix(matrix, k, self.p)
        elif field == "gf16":
            if n > 16:
                raise ValueError("GF(16) codes need n <= 16")
            self.gf = gf.field(4)
            self.E = self.gf.encoding_matrix(matrix, k, self.p).astype(np.uint8)
        elif field == "gf65536":
            if n > 65535:
                raise ValueError("GF(2^16) codes need n <= 65535")
            self.gf = gf.field(16)
            self.E = self._e16(matrix, k, self.p)
        else:
            raise ValueError(f"unknown field {field!r}")
        dt = np.uint16 if field == "gf65536" else np.uint8
        self._dm: dict = {}
        self._g16_bytes: tuple | None = None  # (the G it was made from, its uint16 bytes)
        self.G = np.vstack([np.eye(k, dtype=dt), self.E]).astype(dt)
        self._plans = _PlanCache()
        self._upd_keys = _PlanCache()  # arguments of a repeated update call -> its key in _plans
        self._g_dev: dict = {}  # (device, id(G)) -> G on device, for the on-device decode system

    @property
    def G(self) -> np.ndarray:
        """The n x k generator [I_k; E]. Assigning a new one drops everything derived from the old
        one: the decode matrices, the cached GEMM plans (their tables hold the old inverse's
        coefficients, keyed on buffers and pattern only) and the device copy of G. Replace it
        rather than editing it in place."""
        return self._G

    @G.setter
    def G(self, g: np.ndarray) -> None:
        self._G = g
        self._dm.clear()
        self._g16_bytes = None
        if hasattr(self, "_plans"):  # (absent during __init__)
            self._plans.clear()
            self._upd_keys.clear()
            self._g_dev.clear()

    @property
    def E(self) -> np.ndarray:
        """The p x k encoding matrix. Assigning a new one drops the cached GEMM plans (the encode
        plans' tables hold the old coefficients); assign G as well for decode."""
        return self._E

    @E.setter
    def E(self, e: np.ndarray) -> None:
        self._E = e
        if hasattr(self, "_plans"):
            self._plans.clear()

    # ---- helpers -----------------------------------------------------------------------------
    @property
    def wide(self) -> bool:
        """GF(2^16) symbols (two bytes each)."""
        return self.field == "gf65536"

    def _e16(self, matrix: str, k: int, p: int) -> np.ndarray:
        f = self.gf
        if matrix in ("vandermonde", "vand", "ref"):  # E[i][j] = (j+1)^i, as the C++ gf16w::vandermonde_ref
            return np.array([[f.pow(j + 1, i) for j in range(k)] for i in range(p)], dtype=np.uint16).reshape(p, k)
        if matrix == "cauchy":
            x = np.arange(k, k + p)[:, None] ^ np.arange(k)[None, :]
            return f.inv(x).astype(np.uint16)
        if matrix in ("sys_vandermonde", "sysvand"):
            n = k + p
            v = np.array([[f.pow(r, j) for j in range(k)] for r in range(n)], dtype=np.int64)
            top = self._invert16(v[:k])
            return f.matmul(v[k:], top).astype(np.uint16)
        raise ValueError(f"unknown matrix kind {matrix!r}")

    @staticmethod
    def _invert16(a: np.ndarray) -> np.ndarray:
        """GF(2^16) inverse through the C++ host Gauss-Jordan (gfrs/gf65536.h)."""
        n = a.shape[0]
        try:
            inv = cpu().gf16_invert([int(v) for v in np.asarray(a).reshape(-1)], n)
        except ValueError as e:
            raise UnrecoverableError(str(e)) from None
        return np.asarray(inv, dtype=np.uint16).reshape(n, n)

    def _maps(self, coeff: np.ndarray) -> np.ndarray | None:
        if self.field in ("gf256", "gf65536"):
            return None
        m, k = coeff.shape
        return np.stack([np.stack([gf.byte_map_gf16_nibbles(int(coeff[i, j])) for j in range(k)]) for i in range(m)])

    def _plan(self, key, inputs, outputs, coeff, copies=None) -> GemmPlan:
        plan = self._plans.get(key)
        if plan is None:
            if self.wide:
                plan = Gemm16Plan(inputs, outputs, coeff, copies=copies, hold_buffers=False)
            else:
                maps = self._maps(coeff)
                plan = GemmPlan(inputs, outputs, None if maps is not None else coeff, maps=maps, copies=copies,
                                hold_buffers=False)
            self._plans[key] = plan
        return plan

    @staticmethod
    def _key(tag, *row_lists):
        return (tag,) + tuple(tuple((int(r.data_ptr()), r.numel()) if r is not None else None for r in rl)
                              for rl in row_lists)

    def _cpu_gemm(self, coeff: np.ndarray, ins: list[torch.Tensor], outs: list[torch.Tensor]) -> None:
        ncols = min(r.numel() for r in ins + outs)
        if self.wide:
            if ncols % 2:
                raise ValueError("GF(2^16) rows hold 16-bit symbols: the column range must be an even byte count")
            cpu().gemm16([int(r.data_ptr()) for r in ins], [int(r.data_ptr()) for r in outs],
                         [int(v) for v in np.asarray(coeff).reshape(-1)], ncols, self.cpu_threads)
        elif self.field == "gf256":
            cpu().gemm([int(r.data_ptr()) for r in ins], [int(r.data_ptr()) for r in outs],
                       np.ascontiguousarray(coeff, dtype=np.uint8).tobytes(), ncols, self.cpu_strategy,
                       self.cpu_threads)
        else:
            maps = self._maps(coeff)
            for i, o in enumerate(outs):
                acc = np.zeros(ncols, dtype=np.uint8)
                for j, x in enumerate(ins):
                    acc ^= maps[i, j][x[:ncols].numpy()]
                o[:ncols].copy_(torch.from_numpy(acc))

    # ---- encode ------------------------------------------------------------------------------
    def encode(self, data, parity=None, stream: torch.cuda.Stream | None = None):
        """parity = E . data. ``data``: [k, C] tensor or k rows. Returns the parity rows."""
        fast = None
        if isinstance(parity, torch.Tensor) and parity.dim() == 2 and parity.is_cuda:
            # repeat calls on the same buffers: one dict lookup, no per-row views (a small-object
            # encode is launch-bound; building 14 row views and their key took longer than the kernel);
            # data as a list of rows keys on each row's pointer and length
            if isinstance(data, torch.Tensor):
                fast = ("enc2d", data.data_ptr(), data.shape, data.stride(), parity.data_ptr(), parity.shape,
                        parity.stride())
            else:
                fast = ("encL", tuple((d.data_ptr(), d.numel()) for d in data), parity.data_ptr(), parity.shape,
                        parity.stride())
            plan = self._plans.get(fast)
            if plan is not None:
                plan.run(stream)
                return parity
        ins = as_rows(data)
        if len(ins) != self.k:
            raise ValueError(f"expected {self.k} data rows, got {len(ins)}")
        ncols = min(r.numel() for r in ins)
        if parity is None:
            parity = alloc_rows(self.p, ncols, ins[0].device)
        outs = as_rows(parity)
        if self.p == 0:
            return parity
        if ins[0].device.type == "cuda":
            plan = self._plan(self._key("enc", ins, outs), ins, outs, self.E)
            if fast is not None:
                self._plans[fast] = plan
            plan.run(stream)
        else:
            self._cpu_gemm(self.E, ins, outs)
        return parity

    def encode_batch(self, data: torch.Tensor, parity: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Encode B same-size stripes in ONE launch: ``data`` [B, k, C] -> parity [B, p, C].

        For small objects (KiB..MiB) a per-stripe launch is dominated by launch overhead; the
        batched descriptor (grid.y = stripe) amortises it (serving path)."""
        if data.dim() != 3 or data.shape[1] != self.k:
            raise ValueError(f"expected [B, {self.k}, C]")
        B, _, C = data.shape
        if parity is None:
            pitch = row_pitch(C, data.device)
            base = torch.empty(B * self.p * pitch, dtype=torch.uint8, device=data.device)
            parity = base.as_strided((B, self.p, C), (self.p * pitch, pitch, 1))
        if self.p == 0:
            return parity
        if data.device.type != "cuda":
            for b in range(B):
                self.encode(data[b], parity[b])
            return parity
        # (the plan holds the parity rows' addresses and their batch stride: the key names them too)
        key = ("encb", int(data.data_ptr()), tuple(data.stride()), tuple(data.shape), int(parity.data_ptr()),
               tuple(parity.stride()), tuple(parity.shape))
        plan = self._plans.get(key)
        if plan is None:
            if self.wide:  # GF(2^16): matrix cores for stripes at fixed strides, else batched v_perm
                plan = Gemm16Plan(data, parity, self.E, hold_buffers=False)
            else:
                maps = self._maps(self.E)
                plan = GemmPlan(data, parity, None if maps is not None else self.E, maps=maps, hold_buffers=False)
            self._plans[key] = plan
        plan.run(stream)
        return parity

    def decode_batch(self, survivors: torch.Tensor, rows: Sequence[int], out: torch.Tensor | None = None,
                     stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Rebuild the erased natives of B stripes that lost the same chunks (one launch):
        ``survivors`` [B, k, C] (chunk ids ``rows``) -> ``out`` [B, k, C] natives. On the GPU the
        surviving natives are copied in the same pass (batched fused copy) and the plan is cached
        per (buffers, pattern), so a repeated call is one kernel launch."""
        rows = [int(r) for r in rows]
        B, k, C = survivors.shape
        if k != self.k:
            raise ValueError(f"expected [B, {self.k}, C]")
        if out is None:
            pitch = row_pitch(C, survivors.device)
            base = torch.empty(B * self.k * pitch, dtype=torch.uint8, device=survivors.device)
            out = base.as_strided((B, self.k, C), (self.k * pitch, pitch, 1))
        pos = {r: j for j, r in enumerate(rows)}
        erased = [i for i in range(self.k) if i not in pos]
        if survivors.device.type != "cuda" or not erased:
            # (no native erased on the GPU: plain copies, ordered on ``stream`` like the plan's launch)
            with torch.cuda.stream(stream) if stream is not None and survivors.device.type == "cuda" else null():
                for r, j in pos.items():
                    if r < self.k:
                        out[:, r].copy_(survivors[:, j], non_blocking=True)
            if not erased:
                return out
            dm = self.decode_matrix(rows)[erased]
            for b in range(B):
                self._cpu_gemm(dm, as_rows(survivors[b]), [out[b, i] for i in erased])
            return out
        key = ("decb", tuple(rows), int(survivors.data_ptr()), tuple(survivors.stride()), tuple(survivors.shape),
               int(out.data_ptr()), tuple(out.stride()), tuple(out.shape))
        plan = self._plans.get(key)
        if plan is None:
            outs = [[out[b, i] for i in erased] for b in range(B)]
            ins = [[survivors[b, j] for j in range(self.k)] for b in range(B)]
            copies = [[out[b, r] if r < self.k else None for r in rows] for b in range(B)]
            if self.wide:
                plan = Gemm16Plan(ins, outs, self._erased_rows(rows, erased), copies=copies, hold_buffers=False)
            else:
                dm = self.decode_matrix(rows)[erased]
                maps = self._maps(dm)
                plan = GemmPlan(ins, outs, None if maps is not None else dm, maps=maps, copies=copies,
                                hold_buffers=False)
            self._plans[key] = plan
        plan.run(stream)
        return out

    # ---- decode ------------------------------------------------------------------------------
    def decode_matrix(self, rows: Sequence[int]) -> np.ndarray:
        rows = tuple(int(r) for r in rows)
        dm = self._dm.get(rows)
        if dm is None:
            if len(rows) != self.k or len(set(rows)) != self.k or min(rows) < 0 or max(rows) >= self.n:
                raise ValueError(f"need {self.k} distinct chunk ids in [0, {self.n})")
            try:
                if self.field == "gf256":
                    dm = decode_matrix(self.G, rows)
                elif self.wide:
                    dm = self._invert16(self.G[list(rows)])
                else:
                    dm = self.gf.decode_matrix(self.G, rows).astype(np.uint8)
            except gf.SingularMatrixError as e:
                raise UnrecoverableError(str(e)) from None
            self._dm[rows] = dm
        return dm

    def _erased_rows(self, rows: Sequence[int], erased: Sequence[int]) -> np.ndarray:
        """Rows ``erased`` of the decode matrix (what a decode GEMM applies). GF(2^16): the C++
        e x e systematic solve (``gf16_decode_rows``) instead of the full k x k inverse — 1.4 ms
        against 38 ms at k=300, e=40 — cached per pattern; other fields: rows of decode_matrix."""
        if not self.wide:
            return self.decode_matrix(rows)[list(erased)]
        rows = tuple(int(r) for r in rows)
        key = ("rows", rows, tuple(int(e) for e in erased))
        dm = self._dm.get(key)
        if dm is None:
            if len(rows) != self.k or len(set(rows)) != self.k or min(rows) < 0 or max(rows) >= self.n:
                raise ValueError(f"need {self.k} distinct chunk ids in [0, {self.n})")
            if self._g16_bytes is None or self._g16_bytes[0] is not self.G:
                self._g16_bytes = (self.G, np.ascontiguousarray(self.G, dtype="<u2").tobytes())
            try:
                raw = cpu().gf16_decode_rows(self._g16_bytes[1], self.k, list(rows), [int(e) for e in key[2]])
            except ValueError as e:
                raise UnrecoverableError(str(e)) from None
            dm = np.frombuffer(raw, dtype="<u2").astype(np.uint16).reshape(len(key[2]), self.k)
            self._dm[key] = dm
        return dm

    def is_recoverable(self, rows: Sequence[int]) -> bool:
        try:
            self.decode_matrix(rows)
            return True
        except UnrecoverableError:
            return False

    def decode(self, survivors, rows: Sequence[int], out=None, stream: torch.cuda.Stream | None = None,
               device_invert: bool = False):
        """Reconstruct the k native rows from k surviving chunks.

        Args:
            survivors: [k, C] tensor or k rows, chunk ``rows[j]`` in position j (the reference's conf
                order, ``src/decode.cu:302-318``).
            rows: the chunk ids (0..n-1) of the survivors.
            out: optional [k, C] destination for the natives.
            device_invert: solve the decode system on the GPU (``gf_invert.hip`` / for GF(2^16)
                ``gf_decode16.hip``, writing the GEMM tables directly); a singular pattern then yields
                zeros and a nonzero ``self.last_status`` instead of an exception (checked lazily, no
                host sync on the hot path). GF(2^16) systems too large for one workgroup's LDS are
                solved on the host.
        """
        fast = None
        if not device_invert and isinstance(out, torch.Tensor) and out.dim() == 2 and out.is_cuda:
            # repeat calls on the same buffers and pattern: one dict lookup (see encode). Survivors as
            # a 2-D tensor key on its pointer / shape / strides; as a list of rows (the usual decode:
            # surviving chunks live in different buffers) on each row's pointer and length — 64
            # per-row views of `out` and a per-row key of both sides cost ~180 us a call at k = 64
            if isinstance(survivors, torch.Tensor):
                if survivors.is_cuda:
                    fast = ("dec2d", tuple(int(r) for r in rows), survivors.data_ptr(), survivors.shape,
                            survivors.stride(), out.data_ptr(), out.shape, out.stride())
            else:
                fast = ("decL", tuple(int(r) for r in rows), tuple((s.data_ptr(), s.numel()) for s in survivors),
                        out.data_ptr(), out.shape, out.stride())
            plan = self._plans.get(fast) if fast is not None else None
            if plan is not None:
                plan.run(stream)
                return out
        ins = as_rows(survivors)
        rows = [int(r) for r in rows]
        if len(ins) != self.k or len(rows) != self.k:
            raise ValueError(f"need exactly k={self.k} survivors")
        ncols = min(r.numel() for r in ins)
        dev = ins[0].device
        if out is None:
            out = alloc_rows(self.k, ncols, dev)
        outs = as_rows(out)
        pos = {r: j for j, r in enumerate(rows)}
        erased = [i for i in range(self.k) if i not in pos]
        copies = [outs[r] if r < self.k else None for r in rows]
        if dev.type != "cuda":
            for j, r in enumerate(rows):
                if r < self.k:
                    outs[r][:ncols].copy_(ins[j][:ncols])
            if erased:
                self._cpu_gemm(self._erased_rows(rows, erased), ins, [outs[i] for i in erased])
            return out
        if not erased:  # pure copy: one fused pass with a single dummy output row would waste work
            with torch.cuda.stream(stream) if stream is not None else null():
                for j, r in enumerate(rows):
                    outs[r][:ncols].copy_(ins[j][:ncols], non_blocking=True)
            return out
        key = self._key(("dec", tuple(rows), device_invert), ins, outs)
        if device_invert and self.field == "gf256":
            plan = self._plans.get(key)
            if plan is None:
                plan = GemmPlan(ins, [outs[i] for i in erased], copies=copies, device_tables=True, hold_buffers=False)
                self._plans[key] = plan
                plan.rows_dev = torch.tensor(rows, dtype=torch.int32, device=dev)
                plan.erased_dev = torch.tensor(erased, dtype=torch.int32, device=dev)
                plan.status = torch.zeros(1, dtype=torch.int32, device=dev)
            # systematic decode solved on device: e x (e+k) Gauss-Jordan, tables written in place
            decode_system_into_plan(self._g_device(dev), plan.rows_dev, plan.erased_dev, plan, status=plan.status,
                                    stream=stream)
            self.last_status = plan.status
        elif device_invert and self.wide and decode16_device_supported(self.n, self.k, len(erased)):
            plan = self._plans.get(key)
            if plan is None:
                plan = Gemm16Plan(ins, [outs[i] for i in erased], copies=copies, device_tables=True,
                                  hold_buffers=False)
                self._plans[key] = plan
                plan.rows_dev = torch.tensor(rows, dtype=torch.int32, device=dev)
                plan.erased_dev = torch.zeros(len(erased), dtype=torch.int32, device=dev)
                plan.status = torch.zeros(1, dtype=torch.int32, device=dev)
            g_dev = self._g_dev.get((dev, id(self.G)))
            if g_dev is None:
                self._g_dev.clear()
                g16 = np.ascontiguousarray(self.G, dtype="<u2").view(np.int16)
                g_dev = self._g_dev[(dev, id(self.G))] = torch.from_numpy(g16).to(dev)
            # the GF(2^16) e x (e+k) solve on device (gf_decode16.hip), tables written in place
            decode_system16_into_plan(g_dev, plan.rows_dev, plan.erased_dev, plan, status=plan.status, stream=stream)
            self.last_status = plan.status
        else:
            plan = self._plan(key, ins, [outs[i] for i in erased], self._erased_rows(rows, erased), copies=copies)
            if fast is not None:
                self._plans[fast] = plan
        plan.run(stream)
        return out

    def _g_device(self, dev: torch.device) -> torch.Tensor:
        """G on ``dev`` for the device solves (GF(2^8)), uploaded once per generator."""
        g_dev = self._g_dev.get((dev, id(self.G)))
        if g_dev is None:
            self._g_dev.clear()
            g_dev = self._g_dev[(dev, id(self.G))] = torch.from_numpy(np.ascontiguousarray(self.G)).to(dev)
        return g_dev

    def _reconstruct_solved(self, ins, outs, survivors, erased, stream) -> None:
        """:meth:`reconstruct` with ``device_solve=True`` on the GPU: the pattern's coefficients come
        from ``gf_repair_solve.hip`` as v_perm tables in the plan's descriptor and, on the matrix-core
        engine, as the bit-matrix built from the raw coefficients. The status is read before the GEMM."""
        from ..ops.repair import solve_patterns

        if self.field != "gf256":
            raise NotImplementedError(f"device_solve is implemented for field='gf256', not {self.field!r}")
        if len(survivors) != self.k or len(set(survivors)) != self.k or min(survivors) < 0 or max(survivors) >= self.n:
            raise ValueError(f"need {self.k} distinct chunk ids in [0, {self.n})")
        if min(erased) < 0 or max(erased) >= self.n or set(erased) & set(survivors):
            raise ValueError(f"erased ids must lie in [0, {self.n}) and be no survivors")
        key = self._key(("repd", tuple(survivors), tuple(erased)), ins, outs)
        plan = self._plans.get(key)
        if plan is None:
            dev = ins[0].device
            plan = GemmPlan(ins, outs, device_tables=True, hold_buffers=False)
            ids = torch.full((self.k + plan.m_pad,), -1, dtype=torch.int32)
            ids[: self.k] = torch.tensor(survivors, dtype=torch.int32)
            ids[self.k: self.k + len(erased)] = torch.tensor(erased, dtype=torch.int32)
            ids = ids.to(dev)
            coeff = torch.empty((plan.m_pad, self.k), dtype=torch.uint8, device=dev)
            status = solve_patterns(self._g_device(dev), ids[: self.k].view(1, -1), ids[self.k:].view(1, -1), plan.m_pad,
                                    coeff_out=coeff, tables_out=plan.desc[plan.layout.tab_off:])
            status = int(status.item())  # the one sync, before anything is written
            if status == 1:
                raise UnrecoverableError(f"reconstruct: erased {erased} cannot be repaired from survivors "
                                         f"{survivors}: singular decode system")
            if status:
                raise RuntimeError(f"the repair solve refused erased {erased} with survivors {survivors}")
            if plan.engine == "mfma":
                plan.set_device_coeff(coeff)
            plan._mark_ready()
            self._plans[key] = plan
        plan.run(stream)

    def reconstruct(self, stripe, erased: Sequence[int], survivors: Sequence[int] | None = None,
                    stream: torch.cuda.Stream | None = None, device_solve: bool = False):
        """In-place repair of an n-row stripe: rewrite rows ``erased`` (natives and/or parity) from k
        surviving rows. One GEMM: rows = G[erased] . inv(G[survivors]) . survivors.

        ``device_solve=True`` (CUDA tensors, ``field="gf256"``) solves the pattern on the GPU
        (``csrc/kernels/gf_repair_solve.hip``) instead of inverting ``G[survivors]`` on the host; the
        GEMM runs on the engine the default call picks, from device-written tables. The first call of a
        pattern reads one status word back before the GEMM is launched (a singular pattern raises
        :class:`UnrecoverableError` with the stripe unchanged); a repeat call is the cached launch.
        ``gf16`` / ``gf65536`` on the GPU raise ``NotImplementedError`` with the flag set; CPU tensors
        ignore it and take the CPU path."""
        rows_all = as_rows(stripe)
        if len(rows_all) != self.n:
            raise ValueError(f"stripe must have n={self.n} rows")
        erased = sorted(set(int(e) for e in erased))
        if survivors is None:
            survivors = [i for i in range(self.n) if i not in erased][: self.k]
        survivors = [int(s) for s in survivors]
        if len(survivors) < self.k:
            raise UnrecoverableError(f"only {len(survivors)} survivors, need k={self.k}")
        if not erased:
            return stripe
        if device_solve and rows_all[0].device.type == "cuda":
            self._reconstruct_solved([rows_all[s] for s in survivors if 0 <= s < self.n],
                                     [rows_all[e] for e in erased if 0 <= e < self.n], survivors, erased, stream)
            return stripe
        dm = self.decode_matrix(survivors)
        coeff = self.gf.matmul(self.G[erased], dm).astype(self.G.dtype)
        ins = [rows_all[s] for s in survivors]
        outs = [rows_all[e] for e in erased]
        if ins[0].device.type == "cuda":
            self._plan(self._key(("rep", tuple(survivors), tuple(erased)), ins, outs), ins, outs, coeff).run(stream)
        else:
            self._cpu_gemm(coeff, ins, outs)
        return stripe

    # ---- batched repair (small objects: B stripes per launch, a pattern per stripe) ------------------
    @staticmethod
    def _erased_raw(erased, n: int) -> np.ndarray:
        """``erased`` of :meth:`reconstruct_batch` as an int64 array, 1-D (one list for every stripe) or
        ``[B, e]`` padded with -1 (a ragged nested list is padded here); ids not yet validated, except
        those of a ragged list. Anything else raises ``ValueError``."""
        what = "reconstruct_batch: erased"
        if isinstance(erased, torch.Tensor):
            if erased.device.type != "cpu":
                raise ValueError(f"{what}: ids are validated on the host and must be a CPU tensor, got {erased.device}")
            if erased.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
                raise ValueError(f"{what}: ids must be integers, got {erased.dtype}")
            a = erased.numpy()
        else:
            try:
                a = np.asarray(erased)
            except ValueError:  # a ragged nested list
                a = None
            if a is None or a.dtype == object:
                try:
                    lists = [[int(e) for e in row] for row in erased]
                except (TypeError, ValueError):
                    raise ValueError(f"{what}: expected ids, B id sequences or an integer [B, e] array") from None
                a = np.full((len(lists), max((len(r) for r in lists), default=0)), -1, dtype=np.int64)
                for b, row in enumerate(lists):
                    if row and not 0 <= min(row) <= max(row) < n:
                        raise ValueError(f"{what}: stripe {b}: ids must lie in [0, {n}), got {row}")
                    a[b, : len(row)] = row
            elif a.size and a.dtype.kind not in "iu":
                raise ValueError(f"{what}: ids must be integers, got {a.dtype}")
        if a.ndim not in (1, 2):
            raise ValueError(f"{what}: expected ids, B id sequences or an integer [B, e] array, got shape {tuple(a.shape)}")
        return np.ascontiguousarray(a, dtype=np.int64)

    def _erased_patterns(self, a: np.ndarray, nstripes: int, solve: bool = True):
        """The validated patterns of a batch from :meth:`_erased_raw`'s array: (``pat`` int64 ``[B]``, -1
        for a stripe with nothing erased; the distinct patterns as ``(survivors, erased)`` id tuples,
        in the order their first stripes come). Ids sorted and deduplicated per stripe, the
        survivors the first k ids not erased, every pattern solved once (``self._dm`` caches) unless
        ``solve`` is False (the caller solves them on the device)."""
        what = "reconstruct_batch: erased"
        shared = a.ndim == 1
        if shared:
            a = a.reshape(1, -1)
        elif a.shape[0] != nstripes:
            raise ValueError(f"{what}: {nstripes} stripes but ids for {a.shape[0]}")
        n = self.n
        if a.size and (a.min() < -1 or a.max() >= n):
            b = int(np.nonzero(((a < -1) | (a >= n)).any(axis=1))[0][0])
            raise ValueError(f"{what}: {'' if shared else f'stripe {b}: '}ids must lie in [0, {n}) (or be the -1 "
                             f"padding), got {a[b].tolist()}")
        s = np.where(a < 0, n, a)
        s.sort(axis=1)
        s[:, 1:][s[:, 1:] == s[:, :-1]] = n  # (an id listed twice counts once)
        s.sort(axis=1)
        count = (s < n).sum(axis=1)
        if count.size and count.max() > self.p:
            b = int(np.nonzero(count > self.p)[0][0])
            raise UnrecoverableError(f"reconstruct_batch: {'every stripe' if shared else f'stripe {b}'} has "
                                     f"{int(count[b])} erasures {s[b, :count[b]].tolist()}, more than p={self.p}")
        s = s[:, : int(count.max()) if count.size else 0]
        index, first = {(): -1}, {}
        pat = np.empty(s.shape[0], dtype=np.int64)
        for b, row in enumerate(s.tolist()):
            er = tuple(e for e in row if e < n)
            q = index.get(er)
            if q is None:
                q = index[er] = len(index) - 1
                first[er] = b
            pat[b] = q
        patterns = []
        for er, b in first.items():
            sv = tuple(i for i in range(n) if i not in er)[: self.k]
            try:
                if solve:
                    self.decode_matrix(sv)
            except UnrecoverableError as e:
                raise UnrecoverableError(f"reconstruct_batch: {'the pattern' if shared else f'stripe {b}'} cannot be "
                                         f"repaired: erased {list(er)} with survivors {list(sv)}: {e}") from None
            patterns.append((sv, er))
        return (np.broadcast_to(pat, (nstripes,)) if shared else pat), patterns

    def reconstruct_batch(self, stripes, erased, parity=None, stream: torch.cuda.Stream | None = None,
                          device_solve: bool = False):
        """:meth:`reconstruct` for B stripes of one shape in ONE launch (grid.y = stripe), each stripe
        with erasures OF ITS OWN: after real failures objects placed over different node sets have
        lost different chunks, and one by one the repairs of small objects are launch-bound.
        ``stripes`` / ``parity``: the forms of :meth:`syndrome_mask_batch` (B stripes of n rows of one
        length C, natives first). ``erased``: a flat sequence of ids shared by every stripe; a
        sequence of B id sequences of differing lengths (0..p ids each; an empty one leaves its stripe
        untouched, its rows are not even read); or an integer ``[B, e]`` numpy array or CPU tensor padded
        with -1 (ids are validated on the host: a CUDA tensor raises ``ValueError``). Per stripe the
        result is exactly that of ``reconstruct(stripe_b, erased_b)``: ids sorted and deduplicated,
        the survivors the first k ids not erased, rows ``erased_b`` rewritten in place and no other
        byte touched. The distinct patterns of the batch are solved once each on the host and the
        kernel (``csrc/kernels/gf_repair.hip``) picks each stripe's coefficient tables by a pattern
        index; the plan is cached on the buffers and the ids, so a repeated call is dict lookups and
        the launch. Raised before a byte is written: ``ValueError`` for bad ids, a wrong B, bad rows,
        or a row to rewrite that overlaps any other row the batch uses (so also for a stripe listed
        twice); :class:`UnrecoverableError` for a stripe with more than p erasures or a singular
        pattern, naming the first such stripe. CPU tensors, and ``gf65536`` on the GPU, loop over the
        stripes with :meth:`reconstruct`. Returns ``stripes``.

        ``device_solve=True`` (CUDA tensors, ``field="gf256"``) builds the coefficient tables on the
        GPU: the ids are validated and de-duplicated into distinct patterns on the host as ever, but no
        pattern is solved there. The descriptor goes up with empty table blocks, one launch of
        ``csrc/kernels/gf_repair_solve.hip`` (a workgroup per distinct pattern) fills them in place and
        the statuses are read back once, the only host sync and only on the first call: the plan is
        cached under a key of its own, so a repeat call is dict lookups and the repair launch, with no
        second solve. The bytes written are those of the default call. A singular pattern raises
        :class:`UnrecoverableError` naming the first stripe that uses it, after the solve and before the
        repair kernel: no stripe is touched. ``gf16`` and ``gf65536`` on the GPU raise
        ``NotImplementedError`` with the flag set; CPU tensors ignore it and take the CPU path."""
        from ..ops.repair import BatchRepairPlan, check_repair_overlap, repair_rows

        batch = StripeBatch(stripes, self.n, parity, self.k)
        solved = bool(device_solve) and batch.device.type == "cuda"
        if solved and self.field != "gf256":
            raise NotImplementedError(f"device_solve is implemented for field='gf256', not {self.field!r}")
        raw = self._erased_raw(erased, self.n)
        kernel = batch.device.type == "cuda" and not self.wide
        key = ("repbd" if solved else "repb", batch.key, raw.shape, raw.tobytes()) if kernel else None
        plan = self._plans.get(key) if kernel else None
        if plan is not None:  # a repeat call on the same buffers and patterns: dict lookups and the launch
            plan.run(stream)
            return stripes
        pat, patterns = self._erased_patterns(raw, batch.nstripes, solve=not solved)
        keep = pat >= 0
        if not keep.any() or batch.ncols == 0:
            return stripes
        if self.wide and batch.ncols % 2:
            raise ValueError("GF(2^16) rows hold 16-bit symbols: the rows must be an even byte count")
        m_pad = max(len(er) for _, er in patterns)
        check_repair_overlap(*repair_rows(batch.ptrs()[keep], pat[keep], [(sv, er, None) for sv, er in patterns], m_pad),
                             batch.ncols)
        if solved:
            plan = BatchRepairPlan(batch, pat, [(sv, er, None) for sv, er in patterns], check=False,
                                   g_dev=self._g_device(batch.device))
            bad = np.nonzero(plan.status)[0]
            if bad.size:
                q = int(bad[0])  # (patterns come in the order of their first stripes)
                sv, er = patterns[q]
                if plan.status[q] != 1:
                    raise RuntimeError(f"the repair solve refused erased {list(er)} with survivors {list(sv)}")
                who = "the pattern" if raw.ndim == 1 else f"stripe {int(np.nonzero(pat == q)[0][0])}"
                err = UnrecoverableError(f"reconstruct_batch: {who} cannot be repaired: erased {list(er)} with "
                                         f"survivors {list(sv)}: singular decode system")
                err.stripes = np.nonzero(np.isin(pat, bad))[0].tolist()  # every stripe with such a pattern
                raise err
            self._plans[key] = plan
            plan.run(stream)
            return stripes
        if kernel:
            full = []
            for sv, er in patterns:
                coeff = self.gf.matmul(self.G[list(er)], self.decode_matrix(sv)).astype(self.G.dtype)
                maps = self._maps(coeff)
                full.append((sv, er, coeff if maps is None else maps))
            plan = self._plans[key] = BatchRepairPlan(batch, pat, full, check=False)
            plan.run(stream)
            return stripes
        for b in np.nonzero(keep)[0]:
            self.reconstruct(batch.rows(int(b)), patterns[int(pat[b])][1], stream=stream)
        return stripes

    # ---- scrub -------------------------------------------------------------------------------
    @property
    def H(self) -> np.ndarray:
        """The p x n parity-check matrix [E | I_p]: H . [data; parity] = 0 for a consistent stripe."""
        return gf.check_matrix(self.E)

    def _scrub(self, what: str, batched: bool, stripes, parity, block_bytes: int, stream, locate: bool):
        """The call behind :meth:`syndrome_mask` and :meth:`scrub` (``locate``) and their batched forms:
        a cached plan on the GPU, else zeros (p = 0, nothing to check) or the CPU form stripe by stripe."""
        if self.field != "gf256":
            raise NotImplementedError(f"{what} is implemented for field='gf256', not {self.field!r}")
        if batched:
            batch = StripeBatch(stripes, self.n, parity, self.k)
            nstripes, ncols, dev = batch.nstripes, batch.ncols, batch.device
        else:
            rows, ncols, dev = stripe_rows(stripes, self.n)
            nstripes = 1
        block_bytes = check_block_bytes(block_bytes)
        # (a single stripe of no bytes still gets its plan, a batch of such stripes none: as ever)
        if dev.type == "cuda" and self.p > 0 and nstripes > 0 and (ncols > 0 or not batched):
            key = ("scrubb", block_bytes) + batch.key if batched else self._key(("scrub", block_bytes), rows)
            plan = self._plans.get(key)
            if plan is None:
                plan = BatchScrubPlan(batch, self.H, block_bytes) if batched else ScrubPlan(rows, self.H, block_bytes)
                self._plans[key] = plan
            return plan.scrub(stream) if locate else plan.syndrome_mask(stream)  # (scrub refuses p > 16 itself)
        if locate and self.p > MAX_LOCATE_P:
            raise NotImplementedError(f"{what} locates chunks for p <= {MAX_LOCATE_P} (p = {self.p}); syndrome_mask"
                                      f"{'_batch' if batched else ''} works for any p")
        nmask = -(-ncols // block_bytes)
        mask = torch.zeros((nstripes, nmask), dtype=torch.int32, device=dev)
        votes = np.zeros((nstripes, self.n), dtype=np.int64)
        unlocated, bad = np.zeros(nstripes, dtype=np.int64), np.zeros(nstripes, dtype=np.int64)
        if dev.type != "cuda" and self.p > 0 and nmask:
            h = self.H
            for b in range(nstripes):
                mask[b], votes[b], unlocated[b], bad[b] = cpu_scrub(h, batch.rows(b) if batched else rows, ncols,
                                                                    block_bytes, self._cpu_gemm, locate)
        if not locate:
            return mask if batched else mask[0]
        report = make_batch_report(votes, unlocated, bad, mask)
        return report if batched else report.report[0]

    def syndrome_mask(self, stripe, block_bytes: int = 65536, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Which column blocks of an n-row stripe (natives first, as for :meth:`reconstruct`) are
        inconsistent: an int32 tensor ``[ceil(C / block_bytes)]`` on the stripe's device, bit
        ``i % 32`` set where row i of the syndrome ``H . stripe`` is nonzero in that block; all zero
        for a consistent stripe. One fused pass that reads the n rows once and stores nothing but
        the mask; no host sync. Only columns ``[0, C)`` count (pitch padding is never read).
        ``block_bytes`` is a power of two >= 4096."""
        return self._scrub("syndrome_mask", False, stripe, None, block_bytes, stream, False)

    def scrub(self, stripe, block_bytes: int = 65536, stream: torch.cuda.Stream | None = None) -> ScrubReport:
        """Check a stripe and name the chunks that are wrong: :meth:`syndrome_mask`, then every byte
        column of the dirty blocks is classified. A column whose syndrome has one nonzero byte
        ``s_i`` votes for parity chunk ``k + i``; one whose syndrome is a multiple of column j of
        ``H`` votes for native chunk j; any other is counted as unlocated (more than one chunk
        wrong in that column). Returns a :class:`~gpu_rscode_amd.ops.scrub.ScrubReport`; on the GPU
        both kernels run back to back with one sync at the end.

        Location needs the columns of ``H`` to be pairwise independent and p >= 2 (checked when the
        plan is built); otherwise every bad column is unlocated and ``suspects`` is empty. Codes
        with p > 16 raise ``NotImplementedError`` (``syndrome_mask`` still works)."""
        return self._scrub("scrub", False, stripe, None, block_bytes, stream, True)

    def heal(self, stripe, report: ScrubReport | None = None) -> ScrubReport:
        """Repair a stripe in place from its own redundancy. Scrubs if no ``report`` is given; a
        clean stripe returns the report. If any column is unlocated, or there are no suspects or
        more than p of them, raises :class:`UnrecoverableError` with the stripe byte-for-byte
        unchanged. Otherwise rewrites the suspects with ``reconstruct(stripe, erased=suspects)``,
        scrubs again and returns that second report: read ``.clean`` from it.

        A column with two wrong chunks is told from one with a single wrong chunk only while no three
        columns of ``H`` are dependent. With p = 2 every three are, so a double error can imitate a
        single one: the stripe is then "healed" into a consistent but wrong one."""
        if self.field != "gf256":
            raise NotImplementedError(f"heal is implemented for field='gf256', not {self.field!r}")
        if report is None:
            report = self.scrub(stripe)
        if report.clean:
            return report
        if report.unlocated > 0 or not report.suspects or len(report.suspects) > self.p:
            raise UnrecoverableError(
                f"{report.bad_columns} inconsistent columns, {report.unlocated} of them unlocated, "
                f"suspects {report.suspects}: not repairable from p={self.p} parity chunks")
        self.reconstruct(stripe, erased=report.suspects)
        return self.scrub(stripe)

    # ---- batched scrub (small objects: B stripes per launch) ---------------------------------------
    def syndrome_mask_batch(self, stripes, parity=None, block_bytes: int = 65536,
                            stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """:meth:`syndrome_mask` for B stripes of one shape in ONE launch (grid.y = stripe): an int32
        ``[B, ceil(C / block_bytes)]`` tensor on the stripes' device, row b the mask of stripe b. No
        host sync. ``stripes``: a ``[B, n, C]`` tensor (any batch and row strides), or a sequence of
        B stripes, each an ``[n, C]`` tensor or a list of n rows, natives first; with ``parity``
        (``[B, p, C]``, what :meth:`encode_batch` returns) ``stripes`` holds the natives ``[B, k, C]``.
        All rows have one length C. Any p."""
        return self._scrub("syndrome_mask_batch", True, stripes, parity, block_bytes, stream, False)

    def scrub_batch(self, stripes, parity=None, block_bytes: int = 65536,
                    stream: torch.cuda.Stream | None = None) -> BatchScrubReport:
        """:meth:`scrub` for B stripes of one shape (the forms of :meth:`syndrome_mask_batch`): on
        the GPU one launch of each kernel and one sync for the whole batch. Returns a
        :class:`~gpu_rscode_amd.ops.scrub.BatchScrubReport`, whose ``report[b]`` equals what
        :meth:`scrub` returns for stripe b alone. p > 16 raises ``NotImplementedError``."""
        return self._scrub("scrub_batch", True, stripes, parity, block_bytes, stream, True)

    def heal_batch(self, stripes, parity=None, report: BatchScrubReport | None = None,
                   device_solve: bool = False) -> BatchScrubReport:
        """Repair the dirty stripes of a batch in place, each from its own redundancy. Scrubs if no
        ``report`` is given. A dirty stripe that passes :meth:`heal`'s rule (no unlocated column, 1..p
        suspects) is rewritten as ``reconstruct(stripe_b, erased=suspects_b)`` would, all such stripes
        in ONE :meth:`reconstruct_batch` call; one that fails it, or whose suspects leave a singular
        decode system, is left byte for byte as it was and listed in ``unhealed``. Nothing
        is raised for it: one bad object does not stop the batch. If anything was rewritten the whole
        batch is scrubbed once more and that second report is returned, else the first; either has
        ``unhealed`` filled in. ``device_solve`` is passed to :meth:`reconstruct_batch`: on the GPU the
        suspects' patterns are then solved there, the singular ones come back from that solve, and the
        others are repaired by a second call (the first wrote nothing); CPU tensors ignore it."""
        if self.field != "gf256":
            raise NotImplementedError(f"heal_batch is implemented for field='gf256', not {self.field!r}")
        if report is None:
            report = self.scrub_batch(stripes, parity)
        batch = StripeBatch(stripes, self.n, parity, self.k)
        solved = bool(device_solve) and batch.device.type == "cuda"
        unhealed = []
        erased = np.full((batch.nstripes, self.p), -1, dtype=np.int64)
        for b in report.dirty:
            rep = report.report[b]
            if rep.unlocated > 0 or not rep.suspects or len(rep.suspects) > self.p:
                unhealed.append(b)
                continue
            sus = sorted(set(int(e) for e in rep.suspects))
            # (with the device solve the singular patterns are found by that solve, below)
            if not solved and not self.is_recoverable([i for i in range(self.n) if i not in sus][: self.k]):
                unhealed.append(b)  # (a singular decode system: nothing is written)
                continue
            erased[b, : len(sus)] = sus
        if solved and (erased >= 0).any():
            try:
                self.reconstruct_batch(stripes, erased, parity, device_solve=True)
            except UnrecoverableError as e:  # raised before a byte is written, with every such stripe
                erased[e.stripes] = -1
                unhealed = sorted(unhealed + e.stripes)
                if (erased >= 0).any():
                    self.reconstruct_batch(stripes, erased, parity, device_solve=True)
            if (erased >= 0).any():
                report = self.scrub_batch(stripes, parity)
        elif (erased >= 0).any():
            self.reconstruct_batch(stripes, erased, parity)
            report = self.scrub_batch(stripes, parity)
        report.unhealed = unhealed
        return report

    # ---- correct: error correction per byte column ---------------------------------------------
    def _correct(self, what: str, batched: bool, stripes, parity, max_errors, block_bytes: int, stream):
        """The call behind :meth:`correct` and :meth:`correct_batch`: everything is validated before
        anything is launched or written; then a cached plan on the GPU, or the CPU form stripe by stripe."""
        if self.field != "gf256":
            raise NotImplementedError(f"{what} is implemented for field='gf256', not {self.field!r}")
        if batched:
            batch = StripeBatch(stripes, self.n, parity, self.k)
            nstripes, ncols, dev = batch.nstripes, batch.ncols, batch.device
        else:
            rows, ncols, dev = stripe_rows(stripes, self.n)
            nstripes = 1
        block_bytes = check_block_bytes(block_bytes)
        max_errors = check_max_errors(max_errors, self.p, self.n)
        if dev.type == "cuda" and nstripes > 0 and (ncols > 0 or not batched):
            key = (("correctb", block_bytes, max_errors) + batch.key if batched
                   else self._key(("correct", block_bytes, max_errors), rows))
            plan = self._plans.get(key)
            if plan is None:
                # (the plan runs the aliasing check: a key names the rows' addresses and lengths, so a hit
                # is for rows that passed it)
                plan = (BatchCorrectPlan(batch, self.H, max_errors, block_bytes) if batched
                        else CorrectPlan(rows, self.H, max_errors, block_bytes))
                self._plans[key] = plan
            return plan.correct(stream)
        if batched:
            check_disjoint(batch.ptrs(), ncols)
        else:
            check_disjoint(np.array([[r.data_ptr() for r in rows]], dtype=np.uint64),
                           np.array([[r.numel() for r in rows]], dtype=np.int64))
        nmask = -(-ncols // block_bytes)
        mask = torch.zeros((nstripes, nmask), dtype=torch.int32, device=dev)
        fixed, by_weight = np.zeros((nstripes, self.n), dtype=np.int64), np.zeros((nstripes, 3), dtype=np.int64)
        unc, bad = np.zeros(nstripes, dtype=np.int64), np.zeros(nstripes, dtype=np.int64)
        if dev.type != "cuda" and nmask:
            h = self.H
            for b in range(nstripes):
                mask[b], fixed[b], by_weight[b], unc[b], bad[b] = cpu_correct(
                    h, batch.rows(b) if batched else rows, ncols, block_bytes, max_errors, self._cpu_gemm)
        report = make_batch_correct_report(fixed, by_weight, unc, bad, mask)
        return report if batched else report.report[0]

    def correct(self, stripe, max_errors: int | None = None, block_bytes: int = 65536,
                stream: torch.cuda.Stream | None = None) -> CorrectReport:
        """Repair silent corruption in place, one byte column at a time: where :meth:`heal` names
        suspect chunks and rewrites them whole (and gives up past p suspects, or when two chunks are
        wrong in one column), this XORs the error values into the wrong bytes alone. ``stripe`` as
        for :meth:`scrub`. For every column with a nonzero syndrome ``s``:

        * weight 1: ``s = e . H[:, j]`` for one chunk j (natives and parity alike): ``stripe[j][c] ^= e``;
        * else, with ``max_errors=2``: the explanations ``s = e1 . H[:, j1] ^ e2 . H[:, j2]`` are
          counted over all pairs of chunks; exactly one is applied, none or more than one (the
          reference Vandermonde matrix is not MDS: some 4-sets of its check columns are dependent)
          leaves the column **uncorrectable**, byte for byte as it was.

        Returns a :class:`~gpu_rscode_amd.ops.correct.CorrectReport`: ``fixed_bytes[j]`` bytes changed
        in chunk j, ``by_weight[w]`` columns corrected with w errors, ``uncorrectable`` columns left,
        ``mask`` the syndrome mask before correction. On the GPU: the syndrome launch, one correct
        launch over the dirty blocks, one sync. ``uncorrectable == 0`` means the stripe is consistent
        afterwards. Nothing but the patched bytes is written.

        ``max_errors`` defaults to ``min(2, p // 2)``; 2 needs p >= 4 (distance 5), else
        ``ValueError``, as for p < 2 and for a stripe in which any row overlaps another. Limits:
        GF(2^8) only, p <= 16 and, for ``max_errors=2``, n <= 64 (``ops.correct.MAX_PAIR_N``), else
        ``NotImplementedError``; ``max_errors=1`` works for any n <= 256. Every refusal leaves the
        buffers unchanged.

        More wrong chunks in a column than ``max_errors`` are beyond the code: most such columns are
        uncorrectable, but three or more errors can imitate a pattern of weight one or two, and the
        column is then "corrected" into a consistent but wrong one (with p = 2 and
        ``max_errors=1`` a double error already can, as in :meth:`heal`). That is inherent to the
        code's distance, not to this decoder."""
        return self._correct("correct", False, stripe, None, max_errors, block_bytes, stream)

    def correct_batch(self, stripes, parity=None, max_errors: int | None = None, block_bytes: int = 65536,
                      stream: torch.cuda.Stream | None = None) -> BatchCorrectReport:
        """:meth:`correct` for B stripes of one shape (the forms of :meth:`syndrome_mask_batch`): on
        the GPU one launch of each kernel and one sync for the whole batch. Returns a
        :class:`~gpu_rscode_amd.ops.correct.BatchCorrectReport`, whose ``report[b]`` equals what
        :meth:`correct` returns for stripe b alone. No row may overlap another row of any stripe (a
        stripe listed twice is refused): ``ValueError`` before anything is written. The limits are
        :meth:`correct`'s."""
        return self._correct("correct_batch", True, stripes, parity, max_errors, block_bytes, stream)

    # ---- checked repair: rebuild the erased chunks, check and correct the survivors ------------------
    def _reconstruct_checked(self, what: str, batched: bool, stripes, parity, erased, max_errors, block_bytes: int,
                             stream):
        """The call behind :meth:`reconstruct_checked` and its batched form: everything is validated
        before anything is launched or written; then a cached plan on the GPU, or the CPU form stripe
        by stripe."""
        if self.field != "gf256":
            raise NotImplementedError(f"{what} is implemented for field='gf256', not {self.field!r}")
        if self.p > MAX_LOCATE_P:
            raise NotImplementedError(f"{what} is implemented for p <= {MAX_LOCATE_P} (p = {self.p})")
        if batched:
            batch = StripeBatch(stripes, self.n, parity, self.k)
            nstripes, ncols, dev = batch.nstripes, batch.ncols, batch.device
        else:
            rows, ncols, dev = stripe_rows(stripes, self.n)
            nstripes = 1
        block_bytes = check_block_bytes(block_bytes)
        x = check_erased(erased, self.n, self.p)
        ns, r = self.n - len(x), self.p - len(x)
        max_errors = check_checked_max_errors(max_errors, r, ns)
        nmask = -(-ncols // block_bytes)
        kernel = dev.type == "cuda" and self.p > 0 and nstripes > 0 and (ncols > 0 or not batched)
        if kernel:
            key = (("rchkb", block_bytes, max_errors, tuple(x)) + batch.key if batched
                   else self._key(("rchk", block_bytes, max_errors, tuple(x)), rows))
            plan = self._plans.get(key)
            if plan is not None:
                return plan.run(stream)
        survivors = [i for i in range(self.n) if i not in x]
        if not self.is_recoverable(survivors[: self.k]):
            raise UnrecoverableError(f"{what}: erased {x} with survivors {survivors[: self.k]}: the survivors do not "
                                     "determine the data")
        if batched:
            check_disjoint(batch.ptrs(), ncols)
        else:
            check_disjoint(np.array([[q.data_ptr() for q in rows]], dtype=np.uint64),
                           np.array([[q.numel() for q in rows]], dtype=np.int64))
        if kernel:
            plan = (BatchCheckedRepairPlan(batch, self.H, x, max_errors, block_bytes, check=False) if batched
                    else CheckedRepairPlan(rows, self.H, x, max_errors, block_bytes, check=False))
            self._plans[key] = plan
            return plan.run(stream)
        mask = torch.zeros((nstripes, nmask), dtype=torch.int32, device=dev)
        fixed, by_weight = np.zeros((nstripes, self.n), dtype=np.int64), np.zeros((nstripes, 3), dtype=np.int64)
        unc, bad = np.zeros(nstripes, dtype=np.int64), np.zeros(nstripes, dtype=np.int64)
        if dev.type != "cuda" and self.p > 0 and nmask:
            t = gf.checked_matrix(self.H, x)[0]
            for b in range(nstripes):
                mask[b], fixed[b], by_weight[b], unc[b], bad[b] = cpu_reconstruct_checked(
                    t, x, batch.rows(b) if batched else rows, ncols, block_bytes, max_errors, self._cpu_gemm)
        report = make_batch_correct_report(fixed, by_weight, unc, bad, mask)
        return report if batched else report.report[0]

    def reconstruct_checked(self, stripe, erased: Sequence[int], max_errors: int | None = None,
                            block_bytes: int = 65536, stream: torch.cuda.Stream | None = None) -> CorrectReport:
        """:meth:`reconstruct` that does not trust its survivors: the erased rows are rebuilt from the
        first k survivors while the other ``r = p - e`` survivors check them, in one pass, and a
        survivor that is silently wrong is corrected in place with the rebuilt rows following it
        (errors-and-erasures decoding). ``reconstruct`` alone would write a wrong byte into every
        rebuilt chunk of such a column, and a later ``scrub`` sees two or more wrong chunks there.

        ``stripe`` as for :meth:`reconstruct`; ``erased``: 0..p ids, sorted and deduplicated here (X).
        With S the other ids ascending, K the first k of S, R the rest and
        ``T = inv(H[:, X + R]) . H`` (``gf.checked_matrix``), per byte column: every erased row gets
        ``T[:e, K] . stripe[K]``, byte for byte what :meth:`reconstruct` writes; the column is bad when
        ``u = T[e:, S] . stripe[S] != 0``, and :meth:`correct`'s rule with the r x (n - e) check
        matrix ``T[e:, S]`` is applied to the survivors: a corrected survivor byte j gets ``^= v`` and
        every erased row ``^= v . T[i][j]``; an uncorrectable column keeps its survivors and the plain
        rebuild. The erased rows are never read, and nothing but the erased rows and the patched
        survivor bytes is written. r >= 1 detects, ``r // 2`` wrong survivors per column are
        corrected (at most 2); r = 1 marks every bad column uncorrectable; r = 0 equals
        :meth:`reconstruct` and reports clean; e = 0 equals :meth:`correct`.

        Returns a :class:`~gpu_rscode_amd.ops.correct.CorrectReport`: ``bad_columns`` the columns
        with u != 0, ``fixed_bytes[j]`` the bytes patched in survivor chunk j (erased ids stay 0),
        ``mask`` bit i set where check row i (survivor ``R[i]``'s re-encoding) is nonzero in that
        block before correction. On the GPU: the hot launch (n - e rows read, e written), with
        r >= 1 one launch over the dirty blocks and one sync for the counts; the plan is cached.

        ``max_errors`` defaults to ``min(2, r // 2)`` and at least 1; 2 needs r >= 4 (``ValueError``)
        and at most 64 survivors (``NotImplementedError``). ``ValueError`` for ids out of range, more
        than p of them, bad rows, or any two rows overlapping; :class:`UnrecoverableError` when K does
        not determine the data; ``NotImplementedError`` for another field or p > 16. Every refusal
        comes before anything is launched and leaves the buffers unchanged."""
        return self._reconstruct_checked("reconstruct_checked", False, stripe, None, erased, max_errors, block_bytes,
                                         stream)

    def reconstruct_checked_batch(self, stripes, erased: Sequence[int], parity=None, max_errors: int | None = None,
                                  block_bytes: int = 65536,
                                  stream: torch.cuda.Stream | None = None) -> BatchCorrectReport:
        """:meth:`reconstruct_checked` for B stripes of one shape (the forms of
        :meth:`syndrome_mask_batch`) under ONE erasure list: a lost node takes the same chunk from
        every stripe. On the GPU one launch of each kernel (grid.y = stripe) and one sync for the whole
        batch. Returns a :class:`~gpu_rscode_amd.ops.correct.BatchCorrectReport`, whose ``report[b]``
        equals what :meth:`reconstruct_checked` returns for stripe b alone. No row may overlap
        another row of any stripe. The limits are :meth:`reconstruct_checked`'s."""
        return self._reconstruct_checked("reconstruct_checked_batch", True, stripes, parity, erased, max_errors,
                                         block_bytes, stream)

    # ---- partial-stripe writes ----------------------------------------------------------------
    def _update_rows(self, what: str, changed, parity, first, second):
        """Validated (changed, parity rows, first rows, second rows, shortest row, device)."""
        changed = [int(j) for j in changed]
        if not 1 <= len(changed) <= self.k or len(set(changed)) != len(changed) or min(changed) < 0 \
                or max(changed) >= self.k:
            raise ValueError(f"{what}: changed must be 1..k distinct native ids in [0, {self.k}), got {changed}")
        par, first = as_rows(parity), as_rows(first)
        second = None if second is None else as_rows(second)
        if len(par) != self.p:
            raise ValueError(f"{what}: expected p={self.p} parity rows, got {len(par)}")
        if len(first) != len(changed) or (second is not None and len(second) != len(changed)):
            raise ValueError(f"{what}: expected {len(changed)} rows per changed native")
        rows = par + first + (second or [])
        for r in rows:
            if not isinstance(r, torch.Tensor) or r.dtype != torch.uint8:
                raise ValueError(f"{what}: rows must be uint8 tensors")
            if r.dim() != 1 or (r.numel() > 1 and r.stride(0) != 1):
                raise ValueError(f"{what}: rows must be contiguous 1-D byte rows")
            if r.device != rows[0].device:
                raise ValueError(f"{what}: all rows must live on one device ({rows[0].device} vs {r.device})")
        return changed, par, first, second, min(r.numel() for r in rows), rows[0].device

    @staticmethod
    def _arg_id(x):
        if isinstance(x, torch.Tensor):
            return (x.data_ptr(), x.shape, x.stride(), x.dtype)
        return None if x is None else tuple((r.data_ptr(), r.numel()) for r in x)

    def _update_again(self, form, changed, args, col0, ncols, stream):
        """A repeated call on the same CUDA buffers: two dict lookups instead of per-row views,
        checks and the key of p + 2 d rows (an update of a few MiB per row is launch-bound, as
        :meth:`encode`). Returns the id of the arguments, or None after running the cached plan."""
        try:
            ident = (form, tuple(changed)) + tuple(self._arg_id(a) for a in args)
            key = self._upd_keys.get(ident)
        except (AttributeError, TypeError):  # not tensors: the full path says what is wrong
            return False
        plan = self._plans.get(key) if key is not None else None
        if plan is None:
            return ident
        plan.run(stream, col0, ncols)
        return None

    def _update(self, what, form, changed, par, first, second, limit, dev, col0, ncols, stream, ident=False):
        col0, ncols = window(col0, ncols, limit)
        store_new = form == "write"
        check_overlap(par, first, second, store_new)
        if dev.type == "cuda":
            if self.wide:
                raise NotImplementedError(f"{what} on the GPU is implemented for field='gf256' and 'gf16', "
                                          f"not {self.field!r} (CPU tensors work)")
            if self.p == 0:
                if store_new:
                    with torch.cuda.stream(stream) if stream is not None else null():
                        for a, b in zip(first, second):
                            a[col0: col0 + ncols].copy_(b[col0: col0 + ncols], non_blocking=True)
                return
            key = self._key(("upd", form, tuple(changed)), par, first, second or [])
            plan = self._plans.get(key)
            if plan is None:
                coeff = self.E[:, changed]
                maps = self._maps(coeff)
                plan = self._plans[key] = UpdatePlan(par, first, second, None if maps is not None else coeff,
                                                     maps=maps, store_new=store_new)
            if ident:
                self._upd_keys[ident] = key
            plan.run(stream, col0, ncols)
            return
        if self.wide and (col0 | ncols) & 1:
            raise ValueError("GF(2^16) rows hold 16-bit symbols: col0 and ncols must be even byte counts")
        cpu_update(self.E[:, changed], par, first, second, col0, ncols, self._cpu_gemm, store_new)

    def update(self, parity, changed: Sequence[int], old, new, col0: int = 0, ncols: int | None = None,
               stream: torch.cuda.Stream | None = None):
        """Partial-stripe write, parity side: over byte columns ``[col0, col0 + ncols)`` ``parity``
        (p rows, in place) becomes the parity of the stripe in which natives ``changed[t]`` hold
        ``new[t]`` instead of ``old[t]``: ``parity_i ^= E[i][changed[t]] . (old[t] ^ new[t])``. Only
        the changed natives and the parity rows are read: ``2 d + 2 p`` rows move, where a re-encode
        moves ``k + p``. ``changed``: 1..k distinct native ids, any order; ``old`` / ``new``: [d, C]
        tensors or lists of d rows, left unchanged. ``ncols`` defaults to the shortest row minus
        ``col0``; bytes outside the window are never touched. No parity row may overlap another row
        and no ``new`` row an ``old`` row (``ValueError``). Returns ``parity``."""
        ident = self._update_again("pair", changed, (parity, old, new), col0, ncols, stream)
        if ident is None:
            return parity
        ch, par, first, second, limit, dev = self._update_rows("update", changed, parity, old, new)
        self._update("update", "pair", ch, par, first, second, limit, dev, col0, ncols, stream, ident)
        return parity

    def update_delta(self, parity, changed: Sequence[int], delta, col0: int = 0, ncols: int | None = None,
                     stream: torch.cuda.Stream | None = None):
        """:meth:`update` from ``delta[t] = old[t] ^ new[t]``, what a data node ships to a parity
        node: ``d + 2 p`` rows move. Returns ``parity``."""
        ident = self._update_again("delta", changed, (parity, delta), col0, ncols, stream)
        if ident is None:
            return parity
        ch, par, first, _, limit, dev = self._update_rows("update_delta", changed, parity, delta, None)
        self._update("update_delta", "delta", ch, par, first, None, limit, dev, col0, ncols, stream, ident)
        return parity

    def write(self, stripe, changed: Sequence[int], new, col0: int = 0, ncols: int | None = None,
              stream: torch.cuda.Stream | None = None):
        """Partial-stripe write into an n-row stripe (natives first, as for :meth:`reconstruct`): over
        byte columns ``[col0, col0 + ncols)`` natives ``changed[t]`` are overwritten with ``new[t]``
        and the parity rows updated, in one pass. ``new`` must not overlap the stripe. Returns
        ``stripe``."""
        ident = self._update_again("write", changed, (stripe, new), col0, ncols, stream)
        if ident is None:
            return stripe
        rows = as_rows(stripe)
        if len(rows) != self.n:
            raise ValueError(f"stripe must have n={self.n} rows")
        old = [rows[int(j)] for j in changed if 0 <= int(j) < self.k]
        ch, par, first, second, limit, dev = self._update_rows("write", changed, rows[self.k:], old, new)
        self._update("write", "write", ch, par, first, second, limit, dev, col0, ncols, stream, ident)
        return stripe

    # ---- batched partial-stripe writes (small objects: B stripes per launch) -------------------------
    def _update_batch(self, what, form, par, ids, first, second, col0, ncols, stream):
        """The batched call behind update_batch / update_delta_batch / write_batch: ``par``, ``first``
        and ``second`` are parts (ops.update.batch_part), ``ids`` the raw ``changed`` argument."""
        nstripes = first.nstripes

        def key(a):
            return ("updb", form, par.key, first.key, None if second is None else second.key, a.shape, a.tobytes())
        if first.device.type == "cuda" and isinstance(ids, np.ndarray):
            # a repeat call on the same buffers and ids: dict lookups and the launches
            plan = self._plans.get(key(ids))
            if plan is not None:
                plan.run(stream, col0, ncols)
                return
        ids = batch_ids(ids, nstripes, self.k, f"{what}: changed")
        check_parts(par, first, second, self.p, ids.shape[1])
        if nstripes == 0:
            return
        col0, ncols = window(col0, ncols, first.ncols)
        store_new = form == "write"
        dev = first.device
        fp = first.ptrs()
        sp = None if second is None else second.ptrs()
        check_overlap_batch(par.ptrs() if self.p else fp[:, :0], fp, sp, first.ncols, store_new)
        if dev.type == "cuda" and self.wide:
            raise NotImplementedError(f"{what} on the GPU is implemented for field='gf256' and 'gf16', "
                                      f"not {self.field!r} (CPU tensors work)")
        if self.wide and (col0 | ncols) & 1:
            raise ValueError("GF(2^16) rows hold 16-bit symbols: col0 and ncols must be even byte counts")
        if self.p == 0 or ncols == 0:
            if store_new and ncols:  # nothing to update: a write only copies
                with torch.cuda.stream(stream) if stream is not None and dev.type == "cuda" else null():
                    for b in range(nstripes):
                        for a, c in zip(first.rows(b), second.rows(b)):
                            a[col0: col0 + ncols].copy_(c[col0: col0 + ncols], non_blocking=True)
            return
        if dev.type == "cuda":
            maps = self._maps(self.E)
            plan = BatchUpdatePlan(par, first, second, changed=ids, coeff=None if maps is not None else self.E,
                                   maps=maps, store_new=store_new, check=False)
            self._plans[key(ids)] = plan
            plan.run(stream, col0, ncols)
            return
        for b in range(nstripes):
            cpu_update(self.E[:, ids[b]], par.rows(b), first.rows(b), None if second is None else second.rows(b),
                       col0, ncols, self._cpu_gemm, store_new)

    @staticmethod
    def _batch_ids_fast(changed, nstripes):
        """``changed`` as the int32 ``[B, d]`` array a plan is keyed on, unvalidated; or ``changed`` itself
        when it is anything :func:`~gpu_rscode_amd.ops.update.batch_ids` has to look at first."""
        if isinstance(changed, torch.Tensor):
            if changed.device.type != "cpu" or changed.dtype not in (torch.int32, torch.int64):
                return changed
            a = changed.numpy()
        else:
            try:
                a = np.asarray(changed)
            except ValueError:
                return changed
        if a.dtype.kind not in "iu" or a.ndim not in (1, 2) or a.size == 0:
            return changed
        if a.ndim == 1:
            a = np.broadcast_to(a, (nstripes, a.shape[0]))
        if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
            return changed
        return np.ascontiguousarray(a, dtype=np.int32)

    def update_batch(self, parity, changed, old, new, col0: int = 0, ncols: int | None = None,
                     stream: torch.cuda.Stream | None = None):
        """:meth:`update` for B stripes of one shape in ONE launch (grid.y = stripe), each stripe with
        changed natives of its own: small overwrites of small objects are launch-bound one by one.
        ``parity``: ``[B, p, C]``, in place; ``old`` / ``new``: ``[B, d, C]``, only read. Each is a
        tensor with any batch and row strides (last stride 1) or a sequence of B items, each a
        ``[rows, C]`` tensor or a list of rows; all rows have one length C and the window ``[col0,
        col0 + ncols)`` is shared by the batch. ``changed``: a sequence of d ids (every stripe changes
        the same natives) or ``[B, d]`` ids as a nested list, an integer numpy array or a CPU integer
        tensor (the ids are validated on the host: a CUDA tensor raises ``ValueError``); each row
        holds 1..k distinct ids in ``[0, k)`` in any order, d the same for every stripe. Per stripe
        the result is exactly that of :meth:`update`. No parity row may overlap any other row of any
        stripe and no ``new`` row an ``old`` row (``ValueError``, nothing written). CPU tensors loop
        over the stripes. Returns ``parity``."""
        par = batch_part(parity, "parity")
        self._update_batch("update_batch", "pair", par, self._batch_ids_fast(changed, par.nstripes),
                           batch_part(old, "old"), batch_part(new, "new"), col0, ncols, stream)
        return parity

    def update_delta_batch(self, parity, changed, delta, col0: int = 0, ncols: int | None = None,
                           stream: torch.cuda.Stream | None = None):
        """:meth:`update_batch` from ``delta[b][t] = old ^ new`` (``[B, d, C]``), as :meth:`update_delta`.
        Returns ``parity``."""
        par = batch_part(parity, "parity")
        self._update_batch("update_delta_batch", "delta", par, self._batch_ids_fast(changed, par.nstripes),
                           batch_part(delta, "delta"), None, col0, ncols, stream)
        return parity

    def write_batch(self, stripes, changed, new, parity=None, col0: int = 0, ncols: int | None = None,
                    stream: torch.cuda.Stream | None = None):
        """:meth:`write` for B stripes of one shape in ONE launch: over the window natives
        ``changed[b][t]`` of stripe b are overwritten with ``new[b][t]`` and its parity rows updated,
        in one pass. ``stripes``: ``[B, n, C]`` (natives first), or the natives ``[B, k, C]`` with
        ``parity`` ``[B, p, C]``, in the forms of :meth:`syndrome_mask_batch`; ``new``: ``[B, d, C]``
        and ``changed`` as for :meth:`update_batch`. ``new`` must not overlap the rows that are
        written. Returns ``stripes``."""
        batch = StripeBatch(stripes, self.n, parity, self.k)
        ids = self._batch_ids_fast(changed, batch.nstripes)
        if not isinstance(ids, np.ndarray):
            ids = batch_ids(ids, batch.nstripes, self.k, "write_batch: changed")
        par = PickPart(batch, np.broadcast_to(np.arange(self.k, self.n), (batch.nstripes, self.p)), tag="parity")
        # (the old rows are picked by id: _update_batch validates the ids before any row is looked up)
        self._update_batch("write_batch", "write", par, ids, PickPart(batch, ids), batch_part(new, "new"), col0,
                           ncols, stream)
        return stripes

    def verify(self, data, parity) -> bool:
        """True when ``parity`` is the encoding of ``data`` (recomputes and compares)."""
        ins = as_rows(data)
        ref = self.encode(ins)
        got = as_rows(parity)
        return all(torch.equal(a[: b.numel()], b[: a.numel()]) for a, b in zip(as_rows(ref), got))
