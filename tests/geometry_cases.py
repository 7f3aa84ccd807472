"""Shared pieces of tests/test_geometry_cases.py and tests/test_gpu_geometry.py: the launch arithmetic
of the GEMM engines as integer Python, and row lengths, windows and grid caps derived from it.

A streaming kernel goes wrong in the arithmetic around its launch: tail lanes after the last group,
the block -> (tile, column block) mapping, capped grids with a ragged last lap, the remainder a
chunked kernel hands on, a persistent block's chunk run. This module mirrors that arithmetic

* ``make_grid`` / ``grid_cap`` (csrc/kernels/gf_gemm.hip, gf_gemm16.hip), ``map_block``
  (csrc/include/gfrs/perm_device.h), ``persistent_slots`` (csrc/include/gfrs/device_cache.h);
* the routing of ``run()`` in gf_gemm.hip, ``launch_gf_gemm16_batched`` and of ``GemmPlan.run`` /
  ``Gemm16Plan.run`` (which kernel a window falls to);
* the chunk split of the matrix-core forms (chunks of 256, 128, 512 or 1024 bytes and what is left),

derives the cases of six families from each engine's own units (:func:`cases`), classifies every
case (:func:`classify`) and replays a launch as a list of stores (:func:`stores`). The replay is the
numpy engine of the CPU module: with no fault it must write exactly the window, and with one planted
fault (:data:`FAULTS`) the sweep must fail. :func:`sweep` is the one driver of both modules: rows of
a guard-filled arena (tests/capi_cases.py), the oracle's columns expected in the window, the whole
buffer compared. Only numpy, ``gpu_rscode_amd.gf`` and the two case modules are used here.

Units (C++ names): a *group* is 16 bytes (one lane's ``u32x4``); ``kBlock`` = 256 lanes per block;
an *item* is what ``make_grid`` counts (one lane's work: one group, two groups, one byte or one
symbol); the k-split kernel has 64 groups per block; a *chunk* is ``kBlockCols`` / ``kBC`` /
``kCols`` / ``kChunkBytes`` bytes of every row.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import capi_cases as cc
import engine_cases as ec
from gpu_rscode_amd.gf import GF256

KBLOCK = 256  # kBlock
KSPLIT_GROUPS = 64  # groups per k-split block (one wave's lanes; 8 waves split k)
MAX_GRID_BLOCKS = 0xFFFFFFFF // KBLOCK  # kMaxGridBlocks
LUT_MAX_NCB = 2048
FILL = 0x5A  # outputs and copy destinations before the launch (differs from cc.GUARD)
BATCH = 3
TUNE_DEFAULT = {"rows_lat_groups": 1 << 22, "short_lanes": 0, "ksplit_lanes": 1 << 17, "gf16_short_groups": 32768,
                "fp4_free_cus": 0, "fp4": ""}
ONE_SLOT = 1000000  # GFRS_TUNE=fp4_free_cus=ONE_SLOT: persistent_slots returns 1 for one M-group


# ---- the mirror -------------------------------------------------------------------------------------
def tile_for(m: int) -> int:
    t = 1
    while t < m and t < 16:
        t <<= 1
    return t


def pad_m(m: int) -> int:
    t = tile_for(m)
    return (m + t - 1) // t * t


def grid_cap(ntiles: int) -> int:
    return MAX_GRID_BLOCKS // ntiles // 8 * 8


@dataclass(frozen=True)
class Grid:
    nblk: int    # column blocks of work
    ncb: int     # column blocks of the grid (capped: the kernel strides over the rest)
    blocks: int  # gridDim.x


def make_grid(items: int, ntiles: int, max_blocks: int = 0) -> Grid:
    nblk = (items + KBLOCK - 1) // KBLOCK
    ncb = nblk
    if max_blocks > 0 and ncb > max_blocks:
        ncb = max_blocks
    ncb = min(ncb, grid_cap(ntiles))
    ncb8 = ncb if ncb < 8 else (ncb + 7) // 8 * 8
    return Grid(nblk, ncb, ncb8 * ntiles)


def map_block(bid: int, blocks: int, ntiles: int):
    """(tile, cb0) of block ``bid`` in a grid of ``blocks``."""
    if blocks % (8 * ntiles) != 0:
        return bid % ntiles, bid // ntiles
    xcd, local = bid & 7, bid >> 3
    return local % ntiles, (local // ntiles) * 8 + xcd


def mapping(g: Grid, ntiles: int) -> str:
    if g.blocks % (8 * ntiles) != 0:
        return "plain"
    return "dealt_padded" if g.blocks != g.ncb * ntiles else "dealt_unpadded"


def visits(g: Grid, ntiles: int):
    """[(tile, cb, lap)] of every live block's loop ``for (cb = cb0; cb < nblk; cb += ncb)`` and the
    [(tile, cb0)] of the padding blocks that must return at once."""
    live, dead = [], []
    for bid in range(g.blocks):
        tile, cb0 = map_block(bid, g.blocks, ntiles)
        if cb0 >= g.ncb:
            dead.append((tile, cb0))
            continue
        live += [(tile, cb, lap) for lap, cb in enumerate(range(cb0, g.nblk, g.ncb))]
    return live, dead


def persistent_slots(occ: int, groups: int, nchunks: int, free_cus: int = 0, cus: int = 256) -> int:
    full = cus * occ // groups
    if groups == 1 and free_cus > 0:
        return min(max(1, full - free_cus), nchunks)
    return min(max(8, full // 8 * 8), (nchunks + 7) // 8 * 8)


def fp4_geometry(k: int, m: int, mg_cap: int = 8):
    """(mg, groups) of ``geometry()`` in gf_mfma_fp4.hip."""
    ksteps, mtiles = (k + 15) // 16 * 2, (m + 3) // 4
    mg = 1
    while mg < mtiles and mg < mg_cap:
        mg <<= 1
    while mg > 1 and mg * ksteps > 137 - 2:
        mg >>= 1
    if ksteps == 16 and ((mg == 8 and 4 < mtiles < 8) or (mg == 4 and mtiles == 3)):
        mg = mtiles
    return mg, (mtiles + mg - 1) // mg


def fp4_route(k: int, m: int, copies: bool, forced: str = "") -> str:
    mg, groups = fp4_geometry(k, m)
    wide = 112 < k <= 128
    built = {"v1": True, "ar": groups == 1 and wide, "tm": groups == 1 and wide and 5 <= mg <= 8}
    if forced and built[forced]:
        return forced
    if groups != 1 or not wide:
        return "v1"
    return {4: "ar", 5: "tm", 6: "tm", 7: "tm", 8: "tm" if copies else "ar"}.get(mg, "v1")


def geometry16(k: int, m: int, mg_cap: int = 2):
    """(mg, groups) of ``geometry16()`` in gf_mfma16.hip (the LDS bound does not bind below k = 300)."""
    mtiles = (m + 3) // 4
    mg = 1
    for cand in (2, 1):
        if cand > mg_cap:
            continue
        if mg == 1 or (mtiles + cand - 1) // cand * cand < (mtiles + mg - 1) // mg * mg:
            mg = cand
    return mg, (mtiles + mg - 1) // mg


# ---- launches ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lanes:
    """One launch of a kernel that gives every lane an item: ``ngroups`` groups of ``gbytes`` from
    ``col0``, then ``tail`` lanes of ``tbytes`` each; a block covers ``vpb`` of these. ``loop``: the
    kernel strides over column blocks (else one block per column block and no early return)."""
    kernel: str
    col0: int
    ngroups: int
    gbytes: int
    tail: int
    tbytes: int
    ntiles: int
    mt: int
    max_blocks: int = 0
    vpb: int = KBLOCK
    loop: bool = True
    copies: bool = True
    always_padded: bool = False  # the LDS-table kernel: ncb = min(nblk, 2048) rounded up to 8

    @property
    def items(self):
        per = max(1, self.vpb // KBLOCK)  # groups per lane
        return (self.ngroups + self.tail + per - 1) // per

    @property
    def grid(self) -> Grid:
        if self.always_padded:
            nblk = (self.items + KBLOCK - 1) // KBLOCK
            ncb = (min(nblk, LUT_MAX_NCB) + 7) // 8 * 8
            return Grid(nblk, ncb, ncb * self.ntiles)
        if self.kernel == "ksplit":
            ncb = (self.ngroups + KSPLIT_GROUPS - 1) // KSPLIT_GROUPS
            return Grid(ncb, ncb, ncb * self.ntiles)
        return make_grid(self.items, self.ntiles, self.max_blocks)


@dataclass(frozen=True)
class Chunks:
    """One persistent launch over ``fps`` chunks of ``chunk`` bytes per stripe; the last chunk of a
    stripe holds ``partial`` bytes when that is not 0 (GF(2^16) matrix cores only). Block ``s`` of
    ``slots`` takes chunks s, s + slots, ... of the launch; chunk q is chunk q % fps of stripe q // fps."""
    kernel: str
    col0: int
    chunk: int
    fps: int
    batch: int
    slots: int
    groups: int
    rows_per_group: int
    partial: int = 0
    copies: bool = True

    @property
    def nchunks(self):
        return self.fps * self.batch


def _valu(k, m_pad, batch, col0, n, *, cfg=None, max_blocks=0, bytewise=False, copies=True, tune=TUNE_DEFAULT):
    """``run()`` of gf_gemm.hip: the launches of one v_perm call. ``cfg`` = (vec, pf) or None."""
    if n <= 0:
        return []
    tile = tile_for(m_pad)
    auto = cfg is None and max_blocks == 0 and not bytewise and not (col0 & 15)
    lanes = (n // 16 + n % 16) * batch * (m_pad // tile)
    ksplit = auto and 32 <= k <= 256 and lanes < tune["ksplit_lanes"]
    if ksplit:
        tile = min(tile, 8)
    if auto and not ksplit and tile >= 8:
        while tile > 1 and lanes < tune["short_lanes"]:
            tile //= 2
            lanes *= 2
    nt = m_pad // tile
    if ksplit:
        out = [Lanes("ksplit", col0, n // 16, 16, 0, 1, nt, tile, vpb=KSPLIT_GROUPS, loop=False, copies=copies)]
        if n // 16 == 0:
            out = []
        if n % 16:
            out.append(Lanes("byte", col0 + n // 16 * 16, n % 16, 1, 0, 1, nt, tile))
        return out
    if bytewise or (col0 & 15) or (cfg and cfg[0] < 0):
        return [Lanes("byte_serial" if cfg and cfg[0] < 0 else "byte", col0, n, 1, 0, 1, nt, tile, max_blocks)]
    small = (n // 16 + n % 16) * batch <= tune["rows_lat_groups"]
    rows_ok = tile <= 4 and k in (4, 8, 10, 16)
    if cfg is None and max_blocks == 0 and rows_ok and small:
        return [Lanes("rows_lat", col0, n // 16, 16, n % 16, 1, nt, tile, loop=False, copies=copies)]
    if cfg is None and not copies and max_blocks == 0 and k == 10 and tile == 4:
        return [Lanes("rows", col0, n // 16, 16, n % 16, 1, nt, tile, loop=False, copies=False)]
    vec, pf = cfg if cfg else (2 if tile >= 16 else 1, 2)
    if pf <= 0:
        mt = tile if pf == 0 else -pf
        assert vec == 1 and max_blocks == 0 and m_pad % mt == 0 and mt <= 4 and k in (4, 8, 10, 16)
        return [Lanes("rows_lat" if small else "rows", col0, n // 16, 16, n % 16, 1, m_pad // mt, mt, loop=False)]
    u = 16 * vec
    return [Lanes(f"vec_v{vec}", col0, n // u, u, n % u, 1, nt, tile, max_blocks)]


def _valu16(k, m_pad, batch, col0, n, *, symwise=False, max_blocks=0, tune=TUNE_DEFAULT):
    """``launch_gf_gemm16_batched`` of gf_gemm16.hip."""
    if n <= 0:
        return []
    cap = 1 if n // 16 * batch < tune["gf16_short_groups"] else 8
    mt = min(tile_for(m_pad), cap)
    nt = m_pad // mt
    if symwise or (col0 & 15):
        return [Lanes("sym", col0, n // 2, 2, 0, 2, nt, mt, max_blocks)]
    if mt <= 4 and cap > 1:
        return [Lanes("vec16_g2", col0, n // 16, 16, n % 16 // 2, 2, nt, mt, max_blocks, vpb=2 * KBLOCK)]
    return [Lanes("vec16_g1", col0, n // 16, 16, n % 16 // 2, 2, nt, mt, max_blocks)]


def _slots(groups, nchunks, tune, occ=2):
    """Slots of a persistent grid. At the default the count does not depend on the occupancy for the
    chunk counts used here (round8(nchunks) <= 24 < 256 CUs / groups)."""
    s = persistent_slots(occ, groups, nchunks, tune["fp4_free_cus"])
    assert tune["fp4_free_cus"] or nchunks > 24 or s == (nchunks + 7) // 8 * 8
    return s


# ---- engines ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Engine:
    name: str
    base: str         # its name in engine_cases.ENGINES8 / ENGINES16
    w: int
    kind: str         # valu | lut | i8 | fp4 | valu16 | mfma16
    k: int
    m: int            # the shape with several output tiles (engine_cases)
    m1: int | None    # a one-tile shape of the same kernel, or None where the kernel has one tile only
    families: tuple
    cfg: tuple | None = None      # (vec, pf) of GemmPlan.run(vec=, pf=, nt=True)
    shift: int = 0                # row start past a 256-byte boundary (the byte and symbol kernels)
    batch: int = 1
    tune: tuple = ()              # GFRS_TUNE keys the native code reads once: a child process per setting
    form: str | None = None       # FP4 form the plan must report
    copies: tuple = ("alternate",)  # copy modes run ("none": the copy-free instantiation)
    l_shapes: tuple = ()          # (k, m) of family L
    one_tile_only: bool = False

    def tuned(self) -> dict:
        return {**TUNE_DEFAULT, **dict(self.tune)}

    @property
    def sym(self) -> int:
        return self.w // 8


def _engines():
    E, out = Engine, []
    e8, e16 = ec.ENGINES8, ec.ENGINES16
    lane, cap = ("T", "B", "W"), ("T", "B", "S", "W")
    out.append(E("vec", "vec", 8, "valu", *e8["vec"][:2], 9, cap, cfg=(2, 2)))
    out.append(E("valu_wide", "valu_wide", 8, "valu", *e8["valu_wide"][:2], 8, lane))
    out.append(E("valu_wide+vec", "valu_wide", 8, "valu", *e8["valu_wide"][:2], 8, ("T", "B"), tune=(("ksplit_lanes", 0),)))
    out.append(E("valu_wide+narrow", "valu_wide", 8, "valu", *e8["valu_wide"][:2], None, ("T", "B"),
                 tune=(("ksplit_lanes", 0), ("short_lanes", 10 ** 12))))
    out.append(E("byte", "byte", 8, "valu", *e8["byte"][:2], 9, cap, shift=3))
    out.append(E("byte_serial", "byte", 8, "valu", *e8["byte"][:2], 9, ("T", "B", "S"), cfg=(-1, 2)))
    out.append(E("lut", "lut", 8, "lut", *e8["lut"][:2], 9, lane))
    out.append(E("mfma_i8", "mfma_i8", 8, "i8", *e8["mfma_i8"][:2], None, ("T", "W", "L"), copies=("none",),
                 l_shapes=((32, 20),)))
    fp4 = {"v1": ((128, 12), (100, 17)), "ar": ((128, 16), (128, 32)), "tm": ((128, 20), (128, 26), (128, 32))}
    for f, shapes in fp4.items():
        cp = ("alternate",) if f == "tm" else ("alternate", "none")
        out.append(E(f"mfma_{f}", f"mfma_{f}", 8, "fp4", *e8[f"mfma_{f}"][:2], None, ("T", "W", "L"), form=f, copies=cp,
                     l_shapes=shapes))
        out.append(E(f"mfma_{f}+one_slot", f"mfma_{f}", 8, "fp4", *e8[f"mfma_{f}"][:2], None, ("L",), form=f, copies=cp,
                     l_shapes=shapes, tune=(("fp4_free_cus", ONE_SLOT),)))
        out.append(E(f"mfma_{f}+forced", f"mfma_{f}", 8, "fp4", 128, 24, None, ("L",), form=f, copies=cp,
                     l_shapes=((128, 24),), tune=(("fp4", f),)))
    out.append(E("batched_valu", "batched_valu", 8, "valu", *e8["batched_valu"][:2], 9, ("Q", "W"), batch=BATCH))
    out.append(E("batched_fp4", "batched_fp4", 8, "fp4", *e8["batched_fp4"][:2], None, ("Q", "W", "L"), batch=BATCH,
                 copies=("alternate", "none"), l_shapes=((128, 32),)))
    out.append(E("batched_fp4+one_slot", "batched_fp4", 8, "fp4", *e8["batched_fp4"][:2], None, ("L",), batch=BATCH,
                 copies=("alternate", "none"), l_shapes=((128, 32),), tune=(("fp4_free_cus", ONE_SLOT),)))
    for name, (k, m, _, tile) in e8.items():
        if name.startswith("rows"):
            pf = int(name.rsplit("pf", 1)[1])
            m1 = None if pf == 0 else tile
            for knob in ((), (("rows_lat_groups", 0),)):
                out.append(E(name + ("+throughput" if knob else ""), name, 8, "valu", k, m, m1, lane if not knob else ("T", "B"),
                             cfg=(1, pf), tune=knob, one_tile_only=pf == 0))
    # rows latency form without fused copies (COPY = false): the default launch of a small copy-free plan
    out.append(E("rows_k10_pf0+nocopy", "rows_k10_pf0", 8, "valu", 10, 4, None, ("T", "B"), copies=("none",),
                 one_tile_only=True))
    out.append(E("valu16_g1", "valu16_g1", 16, "valu16", *e16["valu16_g1"][:2], 1, cap))
    out.append(E("valu16_g2", "valu16_g2", 16, "valu16", *e16["valu16_g2"][:2], None, cap, tune=(("gf16_short_groups", 0),),
                 one_tile_only=True))
    out.append(E("sym", "sym", 16, "valu16", *e16["sym"][:2], 1, cap, shift=2))
    out.append(E("mfma", "mfma", 16, "mfma16", *e16["mfma"][:2], None, ("T", "W", "L"), copies=("alternate", "none"),
                 l_shapes=((20, 12),)))
    # one slot needs one M-group: geometry16(20, 12) has three (3 M-tiles, MG = 1), (20, 8) has one (MG = 2)
    out.append(E("mfma+one_slot", "mfma", 16, "mfma16", 20, 8, None, ("L",), copies=("alternate", "none"),
                 l_shapes=((20, 8),), tune=(("fp4_free_cus", ONE_SLOT),)))
    out.append(E("batched_valu16", "batched_valu16", 16, "valu16", *e16["batched_valu16"][:2], 1, ("Q", "W"), batch=BATCH))
    out.append(E("batched_mfma", "batched_mfma", 16, "mfma16", *e16["batched_mfma"][:2], None, ("Q", "W", "L"), batch=BATCH,
                 l_shapes=((20, 12),)))
    out.append(E("batched_mfma+one_slot", "batched_mfma", 16, "mfma16", 20, 8, None, ("L",), batch=BATCH,
                 l_shapes=((20, 8),), tune=(("fp4_free_cus", ONE_SLOT),)))
    return {e.name: e for e in out}


ENGINES = _engines()
FAMILIES = ("T", "B", "S", "W", "L", "Q")


@dataclass(frozen=True)
class Case:
    family: str
    k: int
    m: int
    nrow: int        # bytes per row
    col0: int
    n: int           # window [col0, col0 + n)
    max_blocks: int = 0

    def __str__(self):
        mb = f" max_blocks={self.max_blocks}" if self.max_blocks else ""
        return f"{self.family}: k={self.k} m={self.m} row={self.nrow} window=[{self.col0}, {self.col0 + self.n}){mb}"


def plan(e: Engine, c: Case, copies: bool = True):
    """The launches one ``plan.run(col0, n, max_blocks)`` of engine ``e`` makes, in order: the mirror
    of GemmPlan.run / Gemm16Plan.run and of the native launchers behind them."""
    tune, k, m, B, col0, n = e.tuned(), c.k, c.m, e.batch, c.col0, c.n
    m_pad = pad_m(m)
    bytewise = e.shift % 16 != 0
    if n <= 0:
        return []
    if e.w == 16:
        if e.kind == "mfma16" and c.max_blocks == 0 and col0 % 4 == 0:
            mg, groups = geometry16(k, m)
            fps = n // 1024 + (1 if n % 1024 else 0)
            return [Chunks("mfma16", col0, 1024, fps, B, _slots(groups, fps * B, tune, 4), groups, 4 * mg, n % 1024, copies)]
        return _valu16(k, m_pad, B, col0, n, symwise=bytewise, max_blocks=c.max_blocks, tune=tune)
    valu = dict(copies=copies, tune=tune)
    if e.kind == "fp4" and col0 % 2 == 0:
        mg, groups = fp4_geometry(k, m)
        form = "ar" if B > 1 else fp4_route(k, m, copies, tune["fp4"])
        chunk = 128 if form == "ar" and mg > 4 else 256
        nch = n // chunk
        out = [Chunks(f"fp4_{form}", col0, chunk, nch, B, _slots(groups, nch * B, tune), groups, 4 * mg, 0, copies)] if nch else []
        # (the single-stripe remainder goes through launch_gf_gemm's default: copies = true)
        return out + _valu(k, m_pad, B, col0 + nch * chunk, n - nch * chunk, **{**valu, "copies": copies or B == 1})
    if e.kind == "lut" and col0 % 16 == 0:
        nt = m_pad // tile_for(m_pad)
        out = [Lanes("lut", col0, n // 16, 16, 0, 1, nt, tile_for(m_pad), always_padded=True)] if n // 16 else []
        return out + _valu(k, m_pad, 1, col0 + n // 16 * 16, n % 16, bytewise=True, **valu)
    if e.kind == "i8" and col0 % 4 == 0:
        groups, nch = (m + 7) // 8, n // 512
        slots = min(max(8, 512 // groups // 8 * 8), (nch + 7) // 8 * 8)
        out = [Chunks("i8", col0, 512, nch, 1, slots, groups, 8, 0, False)] if nch else []
        return out + _valu(k, m_pad, 1, col0 + nch * 512, n - nch * 512, **valu)
    if bytewise:
        return _valu(k, m_pad, B, col0, n, max_blocks=c.max_blocks, bytewise=True, **valu)
    if e.cfg is not None and B == 1 and e.kind == "valu":
        return _valu(k, m_pad, 1, col0, n, cfg=e.cfg, max_blocks=c.max_blocks, bytewise=e.cfg[0] < 0, tune=tune)
    return _valu(k, m_pad, B, col0, n, max_blocks=c.max_blocks, **valu)


def runs(e: Engine, k: int, m: int, copy: str) -> bool:
    """Whether shape (k, m) with this copy mode is in the engine's list: the FP4 router must send it to
    the form the engine is named for (8 M-tiles at k = 128: A-resident without copies, tile-major with)."""
    if e.kind != "fp4" or e.batch > 1 or e.form is None:
        return True
    return fp4_route(k, m, copy != "none", e.tuned()["fp4"]) == e.form


def unit(e: Engine, m: int) -> int:
    """Bytes per lane item of the engine's lane kernel on whole aligned rows (u of the case lists)."""
    for l in plan(e, Case("T", e.k, m, 1 << 16, 0, 1 << 16)):
        if isinstance(l, Lanes):
            return max(16, l.gbytes * l.vpb // KBLOCK) if l.kernel != "ksplit" else 16
    return 16


def chunk_of(e: Engine, k: int, m: int, copies: bool = True) -> int:
    for l in plan(e, Case("L", k, m, 1 << 16, 0, 1 << 16), copies):
        if isinstance(l, Chunks):
            return l.chunk
    return 0


# ---- the case lists ---------------------------------------------------------------------------------
B_ITEMS = (1, 63, 64, 65, 255, 256, 257, 7 * 256, 7 * 256 + 1, 8 * 256, 8 * 256 + 1, 9 * 256 + 1, 16 * 256, 16 * 256 + 1)
S_MAX_BLOCKS = (1, 2, 3, 8, 9)
Q_ITEMS = (1, 255, 257, 8 * 256 + 1)
L_DEFAULT, L_ONE_SLOT, L_I8 = (1, 7, 8, 9, 17), (1, 2, 3, 4, 5, 8, 9), (1, 7, 8, 9)
L_REMAINDERS = (0, 2, 77)
L16_FPS, L16_TAILS = (1, 2, 3), (0, 2, 4, 126, 128, 130, 1022)


def _first_lane_kernel(e: Engine, m: int) -> str:
    return next((l.kernel for l in plan(e, Case("B", e.k, m, 1 << 16, 0, 1 << 16)) if isinstance(l, Lanes)), "none")


def _length(e: Engine, m: int, items: int, t: int):
    """Row bytes with ``items`` lane items of which the tail lanes hold ``t`` bytes (t < u); None
    where the tail lanes alone outnumber the items. The byte and symbol kernels have one byte or
    symbol per item and no tail lanes; the k-split and LDS-table kernels count groups only (the tail
    is a second launch), the k-split kernel in blocks of 64: the list's 256 reads as 64 there."""
    kern, s = _first_lane_kernel(e, m), e.sym
    if kern in ("byte", "byte_serial", "sym"):
        return items * s
    if kern == "lut":
        return items * 16 + t
    if kern == "ksplit":
        q, r = divmod(items + 1, 256)
        return (q * KSPLIT_GROUPS + r - 1) * 16 + t
    if kern == "vec16_g2":  # items = (ngroups + tail symbols + 1) / 2 over 16-byte groups; t < 32
        ng = 2 * items - t // 16 - t % 16 // s
        return None if ng < 0 else ng * 16 + t % 16
    u = unit(e, m)
    if items < t // s:
        return None
    return (items - t // s) * u + t


def _tails(e: Engine, m: int, which=None):
    """Tail bytes: every residue of the lane unit, or its edges 0, one symbol, u less one symbol."""
    u, s = unit(e, m), e.sym
    return list(range(0, u, s)) if which is None else sorted({0, s, u - s})


@lru_cache(maxsize=None)
def cases(name: str, family: str) -> tuple:
    e = ENGINES[name]
    if family not in e.families:
        return ()
    out, s = [], e.sym
    shapes = [e.m] + ([e.m1] if e.m1 is not None and e.m1 != e.m else [])

    def whole(fam, m, n, mb=0, k=e.k):
        if n and n > 0:
            out.append(Case(fam, k, m, n, 0, n, mb))

    if family == "T":
        u = unit(e, e.m)
        for g0 in (248, 249) if u == 32 else (248,):
            for t in _tails(e, e.m):
                whole("T", e.m, u * g0 + t)
    elif family == "B":
        for m in shapes:
            for items in B_ITEMS:
                for t in _tails(e, m, "edges"):
                    whole("B", m, _length(e, m, items, t))
    elif family == "Q":
        for items in Q_ITEMS:
            for t in _tails(e, e.m, "edges"):
                whole("Q", e.m, _length(e, e.m, items, t))
    elif family == "S":
        u = unit(e, e.m)
        for mb in S_MAX_BLOCKS:
            for nblk in sorted({mb - 1, mb, mb + 1, 2 * mb + 1, 3 * mb - 1}):
                if nblk >= 1:  # the last block: 100 items, the tail lanes among them
                    whole("S", e.m, _length(e, e.m, (nblk - 1) * 256 + 100, u - s), mb)
    elif family == "W":
        # (matrix-core engines: chunk * 5 + 77 is shorter than the window start 16 * 256, so the row
        # has as many whole chunks as put two of them behind that start; the ragged 77 stays)
        ch = chunk_of(e, e.k, e.m)
        n = ch * max(5, 16 * 256 // ch + 2) + 76 + s if ch else unit(e, e.m) * 600 + 12 - s
        for col0 in (0, 16, 16 * 256, 1, 2, 4, 15, 17) + ((ch + 2,) if ch else ()):
            for end in (n, n - 1, n - 16, n - 17):
                if col0 < end and (e.w == 8 or (col0 | end) % 2 == 0):
                    out.append(Case("W", e.k, e.m, n, col0, end - col0))
    elif family == "L":
        one = e.tuned()["fp4_free_cus"] > 0
        for k, m in e.l_shapes:
            if e.kind == "mfma16":
                for fps in L16_FPS:
                    for t in L16_TAILS:
                        whole("L", m, (fps - (1 if t else 0)) * 1024 + t, k=k)
                continue
            counts = L_I8 if e.kind == "i8" else (1, 2, 3) if e.batch > 1 and one else L_ONE_SLOT if one else L_DEFAULT
            # (the chunk depends on the form, and the form on whether the plan has copies)
            for ch in sorted({chunk_of(e, k, m, cp != "none") for cp in e.copies if runs(e, k, m, cp)}):
                for nch in counts:
                    for r in L_REMAINDERS if one or nch in (1, 9) else (0, 77):
                        whole("L", m, nch * ch + r, k=k)
    return tuple(dict.fromkeys(out))


def classify(e: Engine, c: Case, copies: bool = True) -> dict:
    """What a case exercises, by the names the issue and the CPU module use."""
    ls = plan(e, c, copies)
    d = {"kernels": tuple(l.kernel for l in ls), "tags": set()}
    tags = d["tags"]
    for i, l in enumerate(ls):
        if isinstance(l, Chunks):
            own = [len(range(sl, l.nchunks, l.slots)) for sl in range(l.slots)]
            tags |= {f"chunks_{'0' if o == 0 else '1' if o == 1 else 'even' if o % 2 == 0 else 'odd'}" for o in own}
            if l.batch > 1 and any((sl + l.slots) // l.fps != sl // l.fps for sl in range(l.slots) if sl + l.slots < l.nchunks):
                tags.add("crosses_stripe")
            if l.partial:
                tags |= {f"tail_valid_{min(4, max(0, l.partial - off))}" for off in range(0, 1024, 4)}
            d.update(nchunks=l.nchunks, slots=l.slots, chunk=l.chunk)
            continue
        g = l.grid
        d.update(ngroups=l.ngroups, tail=l.tail, items=l.items, nblk=g.nblk, ncb=g.ncb, ntiles=l.ntiles)
        if i > 0:
            tags.add("remainder")
            if l.col0 % 16:
                tags.add("remainder_off_grid")
        how = "plain" if l.kernel == "ksplit" else mapping(g, l.ntiles)  # (the k-split kernel maps plainly)
        if l.always_padded:  # (its ncb already holds the padding)
            how = "dealt_padded" if g.nblk < g.ncb else "dealt_unpadded"
        tags.add(f"{how}_{'one' if l.ntiles == 1 else 'several'}")
        if l.tail:
            tags.add(f"tail_{l.tail * l.tbytes}")
            first, last = l.ngroups // l.vpb, (l.ngroups + l.tail - 1) // l.vpb
            if first != last:
                tags.add("tail_split")
            if last * l.vpb >= l.ngroups:
                tags.add("tail_only_block")
            laps = (g.nblk + g.ncb - 1) // g.ncb
            if laps > 1 and g.nblk % g.ncb:
                tags.add("ragged_lap_with_tail")
        if g.ncb and g.nblk > g.ncb:
            tags.add("laps")
    d["route"] = ls[0].kernel if ls else None
    return d


# ---- replay: a launch as stores ---------------------------------------------------------------------
FAULTS = {
    # fault -> (engine, family) whose sweep must catch it
    "tail_as_group": ("vec", "T"),
    "tail_block_dropped": ("vec", "T"),
    "padded_blocks_live": ("rows_k10_pf-1", "B"),
    "ragged_lap_skipped": ("vec", "S"),
    "remainder_at_col0": ("mfma_v1", "L"),
    "even_run_last_dropped": ("mfma_ar+one_slot", "L"),
    "phantom_stored": ("mfma_tm", "L"),
    "stripe_not_wrapped": ("batched_fp4+one_slot", "L"),
    "window_rounded_down": ("vec", "W"),
    "copies_tile_gt0": ("lut", "B"),
}


@dataclass
class Store:
    stripe: int
    rows: tuple | None  # output rows [r0, r1), or None: the fused copies
    lo: int             # byte columns [lo, hi) of the row
    hi: int


def _lane_stores(l: Lanes, m: int, fault=None):
    g, out = l.grid, []
    live, dead = visits(g, l.ntiles)
    # (loop = False: one block per column block, nblk = ncb, and the padding blocks do not return
    # early: their lane index is past the items)
    total = l.ngroups + l.tail
    col0 = l.col0
    tail0 = col0 + l.ngroups * l.gbytes
    laps = (g.nblk + g.ncb - 1) // g.ncb if g.ncb else 0
    blocks = [(t, cb, lap, False) for t, cb, lap in live]
    if fault == "padded_blocks_live":  # a padding block works on column block cb0 as if it were whole
        blocks += [(t, cb0, 0, True) for t, cb0 in dead]
    for tile, cb, lap, forced in blocks:
        if fault == "ragged_lap_skipped" and laps > 1 and g.nblk % g.ncb and lap == laps - 1:
            continue
        v0, v1 = cb * l.vpb, (cb + 1) * l.vpb if forced else min((cb + 1) * l.vpb, total)
        spans = []
        if v0 < l.ngroups or forced:
            spans.append((col0 + v0 * l.gbytes, col0 + (v1 if forced else min(v1, l.ngroups)) * l.gbytes))
        if v1 > l.ngroups and not forced:
            t0, t1 = max(v0, l.ngroups) - l.ngroups, v1 - l.ngroups
            if not (fault == "tail_block_dropped" and v0 >= l.ngroups):
                spans.append((tail0 + t0 * l.tbytes, tail0 + (t1 * l.tbytes if fault != "tail_as_group" else t0 * l.tbytes + 16)))
        out += [("out", tile, lo, hi) for lo, hi in spans]
    res = []
    for _, tile, lo, hi in out:
        r0 = tile * l.mt
        if r0 < m:
            res.append((("rows", r0, min(r0 + l.mt, m)), lo, hi))
        do_copy = tile > 0 if fault == "copies_tile_gt0" else tile == 0
        if do_copy and l.copies:
            res.append((("copy",), lo, hi))
    return res


def _chunk_stores(l: Chunks, m: int, fault=None):
    res = []
    for sl in range(l.slots):
        mine = list(range(sl, l.nchunks, l.slots))
        if fault == "even_run_last_dropped" and mine and len(mine) % 2 == 0:
            mine = mine[:-1]
        if fault == "phantom_stored" and mine:
            mine.append(mine[-1] + l.slots)
        for i, q in enumerate(mine):
            b, ch = q // l.fps, q % l.fps
            if fault == "stripe_not_wrapped" and i > 0:
                b, ch = mine[0] // l.fps, mine[0] % l.fps + (q - mine[0])
            if b >= l.batch:  # (a phantom past the last stripe: past the end of the last one)
                ch, b = ch + (b - l.batch + 1) * l.fps, l.batch - 1
            lo = l.col0 + ch * l.chunk
            hi = lo + (l.partial if l.partial and ch == l.fps - 1 else l.chunk)
            for g in range(l.groups):
                r0 = g * l.rows_per_group
                if r0 < m:
                    res.append((b, ("rows", r0, min(r0 + l.rows_per_group, m)), lo, hi))
            if l.copies:
                res.append((b, ("copy",), lo, hi))
    return res


def stores(e: Engine, c: Case, copies: bool = True, fault=None):
    """[(stripe, target, lo, hi)] in launch order: target ("rows", r0, r1) of the outputs or ("copy",)."""
    out = []
    if fault == "window_rounded_down":  # the vector path taken at the aligned address below col0
        c = Case(c.family, c.k, c.m, c.nrow, c.col0 // 16 * 16, c.n, c.max_blocks)
    ls = plan(e, c, copies)
    for i, l in enumerate(ls):
        if isinstance(l, Chunks):
            out += _chunk_stores(l, c.m, fault)
            continue
        if fault == "remainder_at_col0" and i > 0 and isinstance(ls[0], Chunks):
            l = Lanes(**{**l.__dict__, "col0": c.col0})
        for target, lo, hi in _lane_stores(l, c.m, fault):
            out += [(b, target, lo, hi) for b in range(e.batch)]
    return out


# ---- the sweep --------------------------------------------------------------------------------------
def as_bytes(sym: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(sym)
    return a if a.dtype == np.uint8 else a.astype("<u2").view(np.uint8).reshape(a.shape[0], -1)


@lru_cache(maxsize=None)
def oracle(w: int, k: int, m: int, nbytes: int, stripe: int = 0):
    """(coeff [m, k], data bytes [k, nbytes], oracle bytes [m, nbytes]) of one shape at its longest
    row, computed once and sliced (a GEMM is column-wise): ``GF256.gemm`` / ``gf.field(16).gemm``."""
    nsym = (nbytes + w // 8 - 1) // (w // 8)
    coeff = np.random.default_rng([w, k, m]).integers(0, 1 << w, size=(m, k)).astype(np.int64)  # one matrix, every stripe
    coeff[0, 0], coeff[m - 1, k - 1] = 0, 1
    data = np.random.default_rng([w, k, m, stripe, 1]).integers(0, 1 << w, size=(k, nsym)).astype(ec.sym_dtype(w))
    want = GF256.gemm(coeff.astype(np.uint8), data) if w == 8 else ec.field(16).gemm(coeff, data)
    res = (coeff, as_bytes(data), as_bytes(np.asarray(want).astype(ec.sym_dtype(w))))
    for a in res:
        a.setflags(write=False)
    return res


@lru_cache(maxsize=None)
def longest(name: str, k: int, m: int) -> int:
    return max(c.nrow for f in FAMILIES for c in cases(name, f) if (c.k, c.m) == (k, m))


def layouts(e: Engine):
    """(layout, copy mode) pairs an engine's cases run on."""
    if e.batch > 1:
        return [("uniform", cp) for cp in e.copies]
    out = [("uniform", cp) for cp in e.copies]
    if e.shift == 0:
        out.append(("scattered", e.copies[0]))
    return out


class Setup:
    """The rows of one case in one arena: inputs stored, outputs and copy destinations filled with
    FILL, the oracle's window expected in the image."""

    def __init__(self, arena_cls, e: Engine, c: Case, layout: str, copy: str):
        self.e, self.c, self.layout, self.copy = e, c, layout, copy
        k, m, n, B = c.k, c.m, c.nrow, e.batch
        self.arena = a = arena_cls(cc.arena_bytes(B * (2 * k + m), n))
        pitch = (n + 255) // 256 * 256 + cc.PAD
        if B > 1:  # stripes at fixed strides; outputs and copy rows of a stripe at one stride
            ins = a.pitched(B * k, n, pitch)
            both = a.pitched(B * (m + k), n, pitch)
            self.ins = [ins[b * k:(b + 1) * k] for b in range(B)]
            self.outs = [both[b * (m + k): b * (m + k) + m] for b in range(B)]
            cps = [both[b * (m + k) + m: (b + 1) * (m + k)] for b in range(B)]
        elif layout == "scattered":
            self.ins, self.outs, cps = [a.scattered(k, n, 1)], [a.scattered(m, n, 2)], [a.scattered(k, n, 3)]
        else:
            self.ins = [[a.take(n, e.shift) for _ in range(k)]]
            self.outs = [[a.take(n, e.shift) for _ in range(m)]]
            cps = [[a.take(n, e.shift) for _ in range(k)]]
        self.copies = None if copy == "none" else [[r if j % 2 else None for j, r in enumerate(st)] for st in cps]
        nmax = longest(e.name, k, m)
        self.ref = [oracle(e.w, k, m, nmax, b) for b in range(B)]
        fill = np.full(n, FILL, dtype=np.uint8)
        for b in range(B):
            for j, r in enumerate(self.ins[b]):
                r.put(self.ref[b][1][j, :n])
            for r in self.outs[b] + [r for r in cps[b]]:
                r.put(fill)
        self.unused = [r for st in cps for j, r in enumerate(st) if copy == "none" or j % 2 == 0]

    @property
    def coeff(self):
        return self.ref[0][0]

    def expect(self):
        lo, hi = self.c.col0, self.c.col0 + self.c.n
        for b in range(self.e.batch):
            _, data, want = self.ref[b]
            for i, r in enumerate(self.outs[b]):
                r.expect(want[i, lo:hi], lo)
            for j, r in enumerate(self.copies[b] if self.copies else []):
                if r is not None:
                    r.expect(data[j, lo:hi], lo)

    def where(self, off: int) -> str:
        """An arena offset as (row kind, stripe, row, column) and its place relative to the window."""
        best = None
        kinds = [("input", self.ins), ("output", self.outs), ("copy", self.copies or [])]
        for kind, stripes in kinds:
            for b, st in enumerate(stripes):
                for j, r in enumerate(st):
                    if r is not None and r.off <= off and (best is None or r.off > best[3].off):
                        best = (kind, b, j, r)
        for r in self.unused:
            if r.off <= off and (best is None or r.off > best[3].off):
                best = ("unused copy destination", 0, -1, r)
        if best is None:
            return f"arena offset {off}: guard before the first row"
        kind, b, j, r = best
        col = off - r.off
        lo, hi = self.c.col0, self.c.col0 + self.c.n
        if col >= r.n:
            place = f"guard: {col - r.n} bytes past the end of the row (pitch gap)"
        elif lo <= col < hi:
            place = "inside the window"
        else:
            place = f"in the row, outside the window ({lo - col} before it)" if col < lo else \
                f"in the row, outside the window ({col - hi} past it)"
        return f"{kind} row {j} of stripe {b}, column {col}: {place}"

    def check(self):
        """None, or what differs first."""
        got = self.arena.snapshot()
        bad = np.flatnonzero(got != self.arena.image)
        if bad.size == 0:
            return None
        o = int(bad[0])
        return f"{bad.size} bytes differ; first at {self.where(o)}: got {int(got[o]):#04x}, want {int(self.arena.image[o]):#04x}"


def numpy_engine(fault=None):
    """The reference engine (``fault`` None) or one with a planted geometry fault: the replayed stores
    of the mirror written into a host arena through the same Row objects, oracle bytes in the
    outputs and input bytes in the copies."""
    def launch(s: Setup):
        e, c = s.e, s.c
        buf = s.arena.buf
        for b, target, lo, hi in stores(e, c, s.copies is not None, fault):
            _, data, want = s.ref[b]
            if target[0] == "copy" and s.copies is None:
                continue
            if target[0] == "rows":
                pairs = [(s.outs[b][i], want[i]) for i in range(target[1], target[2])]
            else:
                pairs = [(r, data[j]) for j, r in enumerate(s.copies[b]) if r is not None]
            for r, src in pairs:
                a, z = r.off + lo, min(r.off + hi, buf.size)
                if a >= z:
                    continue
                vals = np.full(hi - lo, 0x3C, dtype=np.uint8)
                have = max(0, min(hi, src.size) - lo)
                vals[:have] = src[lo: lo + have]
                buf[a:z] = vals[: z - a]
    return launch


def host_arena(nbytes: int):
    return cc.HostArena(nbytes, pinned=False)


def sweep(name: str, family: str, launch, arena_cls=host_arena, stop_at_first: bool = False) -> list:
    """Every case of one engine and family on every layout, a fresh arena per case: ``launch(setup)``
    runs the engine, the whole arena is compared. Returns one line per failed case: engine, case,
    class and the first differing byte's place."""
    e = ENGINES[name]
    failures = []
    for c in cases(name, family):
        for layout, copy in layouts(e):
            if not runs(e, c.k, c.m, copy):
                continue
            s = Setup(arena_cls, e, c, layout, copy)
            launch(s)
            s.expect()
            msg = s.check()
            if msg:
                cl = classify(e, c, copy != "none")
                failures.append(f"{name} [{layout}, copies {copy}] {c}; kernels {cl['kernels']}, class {sorted(cl['tags'])}: {msg}")
                if stop_at_first:
                    return failures
    return failures


# Settings whose one child ran longer than the slowest case of tests/test_gpu_engines.py in the same
# run on an MI355X (4.8 s and 4.3 s against 3.2 s) and so are cut by family, one child per family.
SPLIT_BY_FAMILY = ((("rows_lat_groups", 0),), (("ksplit_lanes", 0),))


def child_units():
    """[(setting, [(engine, family), ...])]: the sweeps of the engines behind a GFRS_TUNE key that the
    native code reads once. One child process per setting runs all of that setting's sweeps; the
    settings of SPLIT_BY_FAMILY have one child per family."""
    out = []
    for setting in sorted({e.tune for e in ENGINES.values() if e.tune}):
        sweeps = [(e.name, f) for e in ENGINES.values() if e.tune == setting for f in e.families]
        if setting in SPLIT_BY_FAMILY:
            out += [(setting, [sw for sw in sweeps if sw[1] == f]) for f in FAMILIES if any(sw[1] == f for sw in sweeps)]
        else:
            out.append((setting, sweeps))
    return out
