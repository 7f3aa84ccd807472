"""Pure-numpy Galois-field oracle, GF(2^w) for w in {4, 8, 16}.

Independent of the C++/HIP code paths; every native result is tested against it.

Parity with the reference:
  * GF(2^8), primitive polynomial 0x11D (``src/matrix.cu:49``, ``src/cpu-rs.c:37``),
  * GF(2^4) poly 0x13 and GF(2^16) poly 0x1100B (``src/galoisfield.cu:22-25``, unbuilt there),
  * the reference's ``gf_pow`` quirk ``pow(0, e) == 1`` (``src/matrix.cu:204-208``) in
    :meth:`GF.pow_ref`, which the reference Vandermonde ``E[i][j] = (j+1)^i`` depends on for k >= 256.
"""
from __future__ import annotations

import itertools
from functools import lru_cache

import numpy as np

POLYS = {4: 0x13, 8: 0x11D, 16: 0x1100B}


class SingularMatrixError(ValueError):
    """Raised when a GF matrix has no inverse (an unrecoverable erasure pattern)."""


class GF:
    """GF(2^w) arithmetic over numpy integer arrays."""

    def __init__(self, w: int = 8, poly: int | None = None):
        if w not in POLYS and poly is None:
            raise ValueError(f"unsupported field width {w}")
        self.w = w
        self.poly = poly if poly is not None else POLYS[w]
        self.order = 1 << w
        self.dtype = np.uint8 if w <= 8 else np.uint16
        n = self.order - 1
        exp = np.zeros(2 * n, dtype=np.int64)
        log = np.full(self.order, -1, dtype=np.int64)
        x = 1
        for i in range(n):
            exp[i] = exp[i + n] = x
            log[x] = i
            x <<= 1
            if x & self.order:
                x ^= self.poly
        if np.any(log[1:] < 0):
            raise ValueError(f"polynomial {self.poly:#x} is not primitive for w={w}")
        self.exp = exp
        self.log = log

    # ---- scalar / elementwise -----------------------------------------------------------------
    def mul(self, a, b):
        a = np.asarray(a, dtype=np.int64)
        b = np.asarray(b, dtype=np.int64)
        r = self.exp[(self.log[a] + self.log[b]) % (self.order - 1)]
        return np.where((a == 0) | (b == 0), 0, r).astype(np.int64)

    def inv(self, a):
        a = np.asarray(a, dtype=np.int64)
        if np.any(a == 0):
            raise ZeroDivisionError("inverse of 0 in GF")
        return self.exp[(self.order - 1 - self.log[a]) % (self.order - 1)]

    def div(self, a, b):
        return self.mul(a, self.inv(b))

    def pow(self, a: int, e: int) -> int:
        if e == 0:
            return 1
        if a == 0:
            return 0
        return int(self.exp[(int(self.log[a]) * e) % (self.order - 1)])

    def pow_ref(self, a: int, e: int) -> int:
        """Reference ``gf_pow``: exp[(log a * e) % 255] with log(0) treated as 510 -> pow(0,e)=1."""
        la = 2 * (self.order - 1) if a == 0 else int(self.log[a])
        return int(self.exp[(la * e) % (self.order - 1)])

    def mul_table(self, c: int) -> np.ndarray:
        """Row ``c * x`` for every x in the field (the map a coefficient applies to a symbol)."""
        return self.mul(c, np.arange(self.order)).astype(self.dtype)

    # ---- matrices -------------------------------------------------------------------------------
    def matmul(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        a = np.asarray(a, dtype=np.int64)
        b = np.asarray(b, dtype=np.int64)
        out = np.zeros((a.shape[0], b.shape[1]), dtype=np.int64)
        for t in range(a.shape[1]):
            out ^= self.mul(a[:, t : t + 1], b[t : t + 1, :])
        return out.astype(self.dtype)

    def gemm(self, coeff: np.ndarray, data: np.ndarray) -> np.ndarray:
        """out[i] = XOR_j coeff[i,j] * data[j] for (m x k) coeff and (k x C) symbol rows."""
        coeff = np.asarray(coeff)
        data = np.asarray(data)
        m, k = coeff.shape
        out = np.zeros((m, data.shape[1]), dtype=self.dtype)
        for i in range(m):
            for j in range(k):
                c = int(coeff[i, j])
                if c == 0:
                    continue
                out[i] ^= data[j] if c == 1 else self.mul_table(c)[data[j]]
        return out

    def invert(self, a: np.ndarray) -> np.ndarray:
        """Gauss-Jordan with row pivoting; raises SingularMatrixError."""
        a = np.array(a, dtype=np.int64)
        n = a.shape[0]
        r = np.eye(n, dtype=np.int64)
        for c in range(n):
            nz = np.nonzero(a[c:, c])[0]
            if nz.size == 0:
                raise SingularMatrixError(f"singular matrix (no pivot in column {c})")
            p = c + int(nz[0])
            if p != c:
                a[[c, p]] = a[[p, c]]
                r[[c, p]] = r[[p, c]]
            ip = int(self.inv(a[c, c]))
            a[c] = self.mul(a[c], ip)
            r[c] = self.mul(r[c], ip)
            for row in range(n):
                if row != c and a[row, c]:
                    f = int(a[row, c])
                    a[row] ^= self.mul(f, a[c])
                    r[row] ^= self.mul(f, r[c])
        return r.astype(self.dtype)

    def is_invertible(self, a: np.ndarray) -> bool:
        try:
            self.invert(a)
            return True
        except SingularMatrixError:
            return False

    # ---- coding matrices ------------------------------------------------------------------------
    def vandermonde_ref(self, k: int, p: int) -> np.ndarray:
        """Reference encoding block E[i][j] = (j+1)^i (``src/matrix.cu:752-759``)."""
        return np.array([[self.pow_ref((j + 1) % self.order, i) for j in range(k)] for i in range(p)], dtype=self.dtype)

    def cauchy(self, k: int, p: int) -> np.ndarray:
        """MDS Cauchy block C[i][j] = 1/(x_i + y_j), x_i = k+i, y_j = j."""
        if k + p > self.order:
            raise ValueError("cauchy needs k + p <= field order")
        return np.array([[int(self.inv((k + i) ^ j)) for j in range(k)] for i in range(p)], dtype=self.dtype)

    def sys_vandermonde(self, k: int, p: int) -> np.ndarray:
        """MDS systematic Vandermonde: V[k:] @ inv(V[:k]) with V[r][j] = r^j, r = 0..n-1."""
        n = k + p
        if n > self.order:
            raise ValueError("sys_vandermonde needs k + p <= field order")
        v = np.array([[self.pow(r, j) for j in range(k)] for r in range(n)], dtype=np.int64)
        return self.matmul(v[k:], self.invert(v[:k]))

    def encoding_matrix(self, kind: str, k: int, p: int) -> np.ndarray:
        if kind in ("vandermonde", "vand", "ref"):
            return self.vandermonde_ref(k, p)
        if kind == "cauchy":
            return self.cauchy(k, p)
        if kind in ("sys_vandermonde", "sysvand"):
            return self.sys_vandermonde(k, p)
        raise ValueError(f"unknown matrix kind {kind!r}")

    def generator(self, e: np.ndarray) -> np.ndarray:
        k = e.shape[1]
        return np.vstack([np.eye(k, dtype=self.dtype), e.astype(self.dtype)])

    def decode_matrix(self, g: np.ndarray, rows) -> np.ndarray:
        rows = list(rows)
        return self.invert(np.asarray(g)[rows])

    def singular_patterns(self, g: np.ndarray, k: int):
        """All k-subsets of generator rows that are NOT invertible (SURVEY §2.2 census)."""
        n = g.shape[0]
        return [s for s in itertools.combinations(range(n), k) if not self.is_invertible(np.asarray(g)[list(s)])]


@lru_cache(maxsize=None)
def field(w: int = 8) -> GF:
    return GF(w)


GF256 = field(8)


# ---- GF(2)-linear byte maps (what the gfx950 v_perm kernel applies) ------------------------------
def byte_map_gf256(c: int) -> np.ndarray:
    """x -> c*x over GF(2^8)."""
    return GF256.mul_table(int(c)).astype(np.uint8)


def byte_map_gf16_nibbles(c: int) -> np.ndarray:
    """The design doc's "GF(16) method" (``doc/design.tex:190-209``, tables ``src/gf16.h``): each
    byte is two independent GF(2^4) symbols, both multiplied by c."""
    f = field(4)
    t = f.mul_table(int(c) & 15).astype(np.int64)
    x = np.arange(256)
    return ((t[x >> 4] << 4) | t[x & 15]).astype(np.uint8)


def is_linear(byte_map: np.ndarray) -> bool:
    x = np.arange(256)
    basis = byte_map[1 << np.arange(8)].astype(np.int64)
    pred = np.zeros(256, dtype=np.int64)
    for b in range(8):
        pred ^= np.where((x >> b) & 1, basis[b], 0)
    return bool(np.array_equal(pred, byte_map.astype(np.int64))) and byte_map[0] == 0


def perm_record(byte_map: np.ndarray) -> np.ndarray:
    """8 uint32 words: the v_perm 3-chunk tables of a GF(2)-linear byte map (see
    ``csrc/include/gfrs/gf256.h``): T0[v]=L(v), T1[v]=L(v<<3) (v<8), T2[v]=L(v<<6) (v<4)."""
    bm = np.asarray(byte_map, dtype=np.uint8)
    t0 = bm[np.arange(8)]
    t1 = bm[np.arange(8) << 3]
    t2 = bm[np.arange(4) << 6]
    words = np.zeros(8, dtype=np.uint32)
    words[0:2] = np.frombuffer(t0.tobytes(), dtype="<u4")
    words[2:4] = np.frombuffer(t1.tobytes(), dtype="<u4")
    words[4] = np.frombuffer(t2.tobytes(), dtype="<u4")[0]
    return words


def perm_apply(words: np.ndarray, x: np.ndarray) -> np.ndarray:
    """Host emulation of the device lookup (for tests)."""
    b = np.asarray(words, dtype="<u4").tobytes()
    t0 = np.frombuffer(b[0:8], dtype=np.uint8)
    t1 = np.frombuffer(b[8:16], dtype=np.uint8)
    t2 = np.frombuffer(b[16:20], dtype=np.uint8)
    x = np.asarray(x, dtype=np.uint8)
    return t0[x & 7] ^ t1[(x >> 3) & 7] ^ t2[x >> 6]


# ---- GF(2^16) as four byte maps (what the gfx950 w = 16 kernel applies) --------------------------
def perm_quads16(coeff: np.ndarray) -> np.ndarray:
    """(m, k) GF(2^16) coefficients -> (m, k, 4, 8) uint32 v_perm records, the four byte maps of
    each multiply in the order q = 2 * src_byte + dst_byte (``csrc/include/gfrs/gf65536.h``
    perm_quad): c * (l | h << 8) = [L_ll(l) ^ L_hl(h)] | [L_lh(l) ^ L_hh(h)] << 8. Vectorised over
    all coefficients."""
    f = field(16)
    c = np.asarray(coeff, dtype=np.int64)
    m, k = c.shape
    imgs = f.mul(c.reshape(-1, 1), (1 << np.arange(16)).reshape(1, -1))  # (m*k, 16) images of the bits
    out = np.zeros((m * k, 4, 8), dtype=np.uint32)

    def table(basis: np.ndarray, nbits: int) -> np.ndarray:  # (N, nbits) -> (N, 2**nbits) XOR combos
        t = np.zeros((basis.shape[0], 1 << nbits), dtype=np.int64)
        for v in range(1, 1 << nbits):
            for b in range(nbits):
                if v >> b & 1:
                    t[:, v] ^= basis[:, b]
        return t

    def pack(t: np.ndarray) -> np.ndarray:  # (N, 4) bytes -> (N,) little-endian words
        return (t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | (t[:, 3] << 24)).astype(np.uint32)

    for src in range(2):
        for dst in range(2):
            basis = (imgs[:, 8 * src: 8 * src + 8] >> (8 * dst)) & 0xFF  # (N, 8) byte images
            t0, t1, t2 = table(basis[:, 0:3], 3), table(basis[:, 3:6], 3), table(basis[:, 6:8], 2)
            q = 2 * src + dst
            out[:, q, 0], out[:, q, 1] = pack(t0[:, 0:4]), pack(t0[:, 4:8])
            out[:, q, 2], out[:, q, 3] = pack(t1[:, 0:4]), pack(t1[:, 4:8])
            out[:, q, 4] = pack(t2)
    return out.reshape(m, k, 4, 8)


def quad_apply16(quad: np.ndarray, x: np.ndarray) -> np.ndarray:
    """Host emulation of the device lookup of one GF(2^16) coefficient on uint16 symbols (tests)."""
    x = np.asarray(x, dtype=np.uint16)
    lo, hi = (x & 0xFF).astype(np.uint8), (x >> 8).astype(np.uint8)
    ol = perm_apply(quad[0], lo) ^ perm_apply(quad[2], hi)
    oh = perm_apply(quad[1], lo) ^ perm_apply(quad[3], hi)
    return (ol.astype(np.uint16) | (oh.astype(np.uint16) << 8)).astype(np.uint16)


# ---- scrub: syndrome check and corrupt-chunk location ----------------------------------------------
def check_matrix(e: np.ndarray) -> np.ndarray:
    """The p x n parity-check matrix H = [E | I_p] of the systematic code with encoding block E:
    H . [data; parity] = 0 exactly for a consistent stripe (characteristic 2: E.data ^ parity)."""
    e = np.asarray(e, dtype=np.uint8)
    return np.hstack([e, np.eye(e.shape[0], dtype=np.uint8)])


def columns_independent(h: np.ndarray) -> bool:
    """True when no column of H is zero and no two are multiples of each other: a one-chunk error
    then has a syndrome that names its chunk."""
    h = np.asarray(h, dtype=np.int64)
    seen = set()
    for j in range(h.shape[1]):
        col = h[:, j]
        nz = np.nonzero(col)[0]
        if nz.size == 0:
            return False
        key = tuple(int(v) for v in GF256.mul(col, int(GF256.inv(int(col[nz[0]])))))  # first nonzero scaled to 1
        if key in seen:
            return False
        seen.add(key)
    return True


def scrub_oracle(h: np.ndarray, rows, block_bytes: int = 65536):
    """Plain numpy scrub of an n-row stripe against the check matrix ``h`` (p x n): returns
    ``(mask, votes, unlocated, bad_columns)``.

    ``mask[b]`` has bit ``i % 32`` set when syndrome row i is nonzero anywhere in columns
    ``[b * block_bytes, (b + 1) * block_bytes)``. Every column with a nonzero syndrome s is counted
    in ``bad_columns`` and classified: one nonzero ``s_i`` votes for parity chunk ``k + i``; several
    vote for the native chunk j whose column of ``h`` s is a multiple of; anything else, and every
    bad column when p < 2 or the columns of ``h`` are not pairwise independent, is ``unlocated``."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    k = n - p
    data = np.stack([np.asarray(r, dtype=np.uint8) for r in rows]) if not isinstance(rows, np.ndarray) else rows
    c = data.shape[1]
    s = GF256.gemm(h, data)
    nblk = -(-c // block_bytes)
    bits = np.zeros(nblk, dtype=np.uint32)
    for i in range(p):
        bits[np.unique(np.nonzero(s[i])[0] // block_bytes)] |= np.uint32(1 << (i % 32))
    mask = bits.view(np.int32)
    votes = np.zeros(n, dtype=np.int64)
    nzc = (s != 0).sum(axis=0)
    bad = nzc > 0
    bad_columns = int(bad.sum())
    if p < 2 or not columns_independent(h):
        return mask, votes, bad_columns, bad_columns
    single = nzc == 1
    for i in range(p):
        votes[k + i] = int((single & (s[i] != 0)).sum())
    pending = nzc > 1
    for j in range(k):
        col = h[:, j]
        r = int(np.nonzero(col)[0][0])
        e = GF256.mul(s[r], int(GF256.inv(int(col[r]))))
        match = pending & (e != 0)
        for i in range(p):
            match &= GF256.mul(e, int(col[i])) == s[i]
        votes[j] = int(match.sum())
        pending &= ~match
    return mask, votes, int(pending.sum()), bad_columns


# ---- correct: error correction per byte column -----------------------------------------------------
def correct_oracle(h: np.ndarray, rows, max_errors: int):
    """Plain numpy error correction of an n-row stripe against the check matrix ``h`` (p x n), one
    byte column at a time: returns ``(fixed_rows, fixed_bytes[n], by_weight[3], uncorrectable,
    bad_columns)``; ``rows`` is not modified.

    A column with syndrome ``s = h . rows[:, c] != 0`` is repaired with the smallest set of chunks
    that explains it. When p < 2 or the columns of ``h`` are not pairwise independent it is
    uncorrectable. Otherwise, if ``s = e . h[:, j]`` for a chunk j and e != 0 (then unique), byte
    ``rows[j][c]`` gets ``^= e`` (weight 1). Otherwise, with ``max_errors == 2``, every pair j1 < j2
    is solved for ``s = e1 . h[:, j1] ^ e2 . h[:, j2]`` on a nonsingular 2 x 2 row minor and checked
    on all p rows with e1, e2 != 0: exactly one such explanation over all pairs is applied (weight
    2); none, or more than one, leaves the column uncorrectable and byte for byte as it was.
    ``fixed_bytes[j]`` counts the bytes changed in chunk j, ``by_weight[w]`` the columns corrected
    with w errors (``by_weight[0]`` stays 0)."""
    if max_errors not in (1, 2):
        raise ValueError(f"max_errors must be 1 or 2, got {max_errors}")
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    out = np.array(np.stack([np.asarray(r, dtype=np.uint8) for r in rows]) if not isinstance(rows, np.ndarray)
                   else rows, dtype=np.uint8)
    fixed_bytes, by_weight = np.zeros(n, dtype=np.int64), np.zeros(3, dtype=np.int64)
    bad = np.nonzero(GF256.gemm(h, out).any(axis=0))[0]
    if bad.size == 0:
        return out, fixed_bytes, by_weight, 0, 0
    if p < 2 or not columns_independent(h):
        return out, fixed_bytes, by_weight, int(bad.size), int(bad.size)
    mul = np.stack([GF256.mul_table(c) for c in range(256)])  # mul[a][b]
    inv = np.zeros(256, dtype=np.int64)
    inv[1:] = GF256.inv(np.arange(1, 256))
    s = GF256.gemm(h, out[:, bad])  # p x m: the bad columns only
    pending = np.ones(bad.size, dtype=bool)
    for j in range(n):
        r = int(np.nonzero(h[:, j])[0][0])
        e = mul[inv[h[r, j]]][s[r]]
        hit = pending & (e != 0) & (mul[h[:, j][:, None], e[None, :]] == s).all(axis=0)
        out[j, bad[hit]] ^= e[hit]
        fixed_bytes[j] += int(hit.sum())
        pending &= ~hit
    by_weight[1] = int((~pending).sum())
    if max_errors == 2 and pending.any():
        todo = np.nonzero(pending)[0]
        st = s[:, todo]
        count = np.zeros(todo.size, dtype=np.int64)
        found = np.zeros((4, todo.size), dtype=np.int64)  # j1, j2, e1, e2 of a column's first explanation
        for j1, j2 in itertools.combinations(range(n), 2):
            a, b = next((a, b) for a, b in itertools.combinations(range(p), 2)
                        if mul[h[a, j1], h[b, j2]] != mul[h[a, j2], h[b, j1]])  # (pairwise independent: there is one)
            idet = inv[mul[h[a, j1], h[b, j2]] ^ mul[h[a, j2], h[b, j1]]]
            e1 = mul[idet][mul[h[b, j2]][st[a]] ^ mul[h[a, j2]][st[b]]]  # Cramer's rule, characteristic 2
            e2 = mul[idet][mul[h[b, j1]][st[a]] ^ mul[h[a, j1]][st[b]]]
            ok = (e1 != 0) & (e2 != 0)
            ok &= ((mul[h[:, j1][:, None], e1[None, :]] ^ mul[h[:, j2][:, None], e2[None, :]]) == st).all(axis=0)
            first = ok & (count == 0)
            found[:, first] = np.stack([np.full(int(first.sum()), j1), np.full(int(first.sum()), j2),
                                        e1[first], e2[first]])
            count += ok
        for x in np.nonzero(count == 1)[0]:
            j1, j2, e1, e2 = (int(v) for v in found[:, x])
            c = bad[todo[x]]
            out[j1, c] ^= e1
            out[j2, c] ^= e2
            fixed_bytes[j1] += 1
            fixed_bytes[j2] += 1
        by_weight[2] = int((count == 1).sum())
        pending[todo[count == 1]] = False
    return out, fixed_bytes, by_weight, int(pending.sum()), int(bad.size)


# ---- partial-stripe writes: the delta identity -----------------------------------------------------
def update_oracle(e: np.ndarray, parity, changed, old, new) -> np.ndarray:
    """Plain numpy parity update over GF(2^8): the parity rows of the stripe in which natives
    ``changed[t]`` hold ``new[t]`` instead of ``old[t]``, from the old parity alone:
    ``parity ^ E[:, changed] . (old ^ new)``. ``e`` is the p x k encoding block; ``parity`` [p, C],
    ``old`` and ``new`` [d, C]. Returns a new array."""
    e = np.asarray(e, dtype=np.uint8)
    parity = np.asarray(parity, dtype=np.uint8)
    delta = np.asarray(old, dtype=np.uint8) ^ np.asarray(new, dtype=np.uint8)
    return parity ^ GF256.gemm(e[:, [int(j) for j in changed]], delta)


# ---- repair: rewrite erased rows from the first k survivors -----------------------------------------
def reconstruct_oracle(g: np.ndarray, rows, erased) -> np.ndarray:
    """Plain numpy repair over GF(2^8): the n-row stripe ``rows`` with rows ``erased`` (any ids in
    ``[0, n)``, sorted and deduplicated here) recomputed from the first k rows not erased:
    ``G[erased] . inv(G[survivors]) . rows[survivors]``. ``g`` is the n x k generator. Returns a new
    array; raises :class:`SingularMatrixError` for a pattern whose survivors do not determine the data
    and ``ValueError`` when fewer than k rows survive."""
    g = np.asarray(g, dtype=np.uint8)
    out = np.array(rows, dtype=np.uint8)
    n, k = g.shape
    erased = sorted(set(int(e) for e in erased))
    if not erased:
        return out
    survivors = [i for i in range(n) if i not in erased][:k]
    if len(survivors) < k:
        raise ValueError(f"only {len(survivors)} survivors, need k={k}")
    coeff = GF256.matmul(g[erased], GF256.invert(g[survivors]))
    out[erased] = GF256.gemm(coeff, out[survivors])
    return out


def repair_coeff_oracle(g: np.ndarray, survivors, erased) -> np.ndarray:
    """Plain numpy form of the route ``csrc/kernels/gf_repair_solve.hip`` takes to the repair
    coefficients ``G[erased] . inv(G[survivors])`` (e x k over GF(2^8), columns in the order of
    ``survivors``, rows in the order of ``erased``) of a systematic generator ``g = [I; E]``, without
    the k x k inverse. With Mn the natives that are no survivors and P the parity survivors (as many),
    the systematic solve ``X = inv(G[P, Mn]) . B'`` gives the rows of the natives in Mn, where
    ``B'[r][c]`` is ``G[P_r][survivors_c]`` for a native survivor and ``[survivors_c == P_r]`` for a
    parity one; an erased parity row x is its base row (``G[x][survivors_c]`` for a native survivor,
    0 for a parity one) plus ``G[x, Mn] . X``. Raises :class:`SingularMatrixError` where
    ``G[P, Mn]`` is singular (exactly where ``G[survivors]`` is) and ``ValueError`` for lists that are
    not k distinct survivors in ``[0, n)`` and erased ids in ``[0, n)`` that are no survivors."""
    g = np.asarray(g, dtype=np.uint8)
    n, k = g.shape
    sv = [int(s) for s in survivors]
    er = [int(x) for x in erased]
    if len(sv) != k or len(set(sv)) != k or min(sv) < 0 or max(sv) >= n:
        raise ValueError(f"need {k} distinct survivor ids in [0, {n})")
    if er and (min(er) < 0 or max(er) >= n or set(er) & set(sv)):
        raise ValueError(f"erased ids must lie in [0, {n}) and be no survivors")
    native = np.array([s < k for s in sv], dtype=bool)
    mn = [i for i in range(k) if i not in set(sv)]
    par = [s for s in sv if s >= k]
    sv_nat = [s if s < k else 0 for s in sv]  # (a parity survivor's column index is never used)

    def base(ids, identity: bool) -> np.ndarray:
        b = np.where(native[None, :], g[np.ix_(ids, sv_nat)], 0).astype(np.uint8)
        if identity:
            b |= (np.array(ids)[:, None] == np.array(sv)[None, :]).astype(np.uint8)
        return b

    x = np.zeros((0, k), dtype=np.uint8)
    if mn:  # (|P| == |Mn|: the k survivors are distinct)
        x = GF256.matmul(GF256.invert(g[np.ix_(par, mn)]), base(par, True))
    out = np.zeros((len(er), k), dtype=np.uint8)
    for i, e in enumerate(er):
        if e < k:
            out[i] = x[mn.index(e)]
        else:
            out[i] = base([e], False)[0]
            if mn:
                out[i] ^= GF256.matmul(g[[e]][:, mn], x)[0]
    return out


# ---- checked repair: rebuild erased rows, check and correct the survivors with the surplus parity ----
def checked_matrix(h: np.ndarray, erased) -> tuple[np.ndarray, list, list, list]:
    """``(T, X, S, R)`` of a degraded stripe under the check matrix ``h`` (p x n): X the erased ids
    (sorted, deduplicated; at most p), S the other ids ascending, R the last ``r = p - |X|`` of S (K, the
    first k of S, are the survivors a rebuild reads) and ``T = inv(h[:, X + R]) . h``, so that
    ``T[:, X + R] = I_p``. Rows ``0..e-1`` of T rebuild the erased rows from K (they are zero on R),
    rows ``e..p-1`` check survivor ``R[i]`` against K (they are zero on X). Raises
    :class:`SingularMatrixError` when K does not determine the data."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    x = sorted(set(int(e) for e in erased))
    if x and not 0 <= x[0] <= x[-1] < n:
        raise ValueError(f"erased ids must lie in [0, {n}), got {x}")
    if len(x) > p:
        raise ValueError(f"{len(x)} erasures, more than p={p}")
    s = [i for i in range(n) if i not in x]
    r = s[n - p:]
    t = GF256.matmul(GF256.invert(h[:, x + r]), h).astype(np.uint8)
    return t, x, s, r


def reconstruct_checked_oracle(h: np.ndarray, rows, erased, max_errors: int | None = None):
    """Plain numpy errors-and-erasures repair of an n-row stripe against the check matrix ``h`` (p x n):
    returns ``(rows_out, fixed_bytes[n], by_weight[3], uncorrectable, bad_columns, T)``; ``rows`` is
    not modified and its erased rows are never read.

    With :func:`checked_matrix`'s T, X, S, K, R and e = |X|, r = p - e, per byte column c: every erased
    row ``X[i]`` gets ``w_i = T[i, K] . rows[K, c]`` (what :func:`reconstruct_oracle` writes); the
    column is bad when ``u = T[e:, S] . rows[S, c] != 0``, and :func:`correct_oracle`'s rule with the
    r x (n - e) check matrix ``T[e:, S]`` is applied to the survivors (r < 2: uncorrectable). A
    corrected survivor byte j gets ``^= v`` and each erased row then ``^= v . T[i][j]``, the value
    rebuilt from the corrected survivors; an uncorrectable column keeps its survivors and ``w``.
    ``fixed_bytes`` counts survivor bytes by chunk id (erased ids stay 0). ``max_errors``: 1 or 2,
    default ``min(2, r // 2)`` and at least 1."""
    h = np.asarray(h, dtype=np.uint8)
    p, n = h.shape
    t, x, s, _ = checked_matrix(h, erased)
    e, r = len(x), p - len(x)
    k = n - p
    out = np.array(np.stack([np.asarray(q, dtype=np.uint8) for q in rows]) if not isinstance(rows, np.ndarray)
                   else rows, dtype=np.uint8)
    fixed_bytes, by_weight = np.zeros(n, dtype=np.int64), np.zeros(3, dtype=np.int64)
    if e:
        out[x] = GF256.gemm(t[:e][:, s[:k]], out[s[:k]])
    if r == 0:
        return out, fixed_bytes, by_weight, 0, 0, t
    if max_errors is None:
        max_errors = max(1, min(2, r // 2))
    surv = out[s]
    fixed, fb, by_weight, uncorrectable, bad_columns = correct_oracle(t[e:][:, s], surv, max_errors)
    fixed_bytes[s] = fb
    if e:
        out[x] ^= GF256.gemm(t[:e][:, s], fixed ^ surv)
    out[s] = fixed
    return out, fixed_bytes, by_weight, uncorrectable, bad_columns, t
