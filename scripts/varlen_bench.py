#!/usr/bin/env python3
"""Time the variable-length batch against what a caller with mixed object sizes does today.

One process, one code ((10, 14) cauchy by default), ``--objects`` objects whose chunk lengths are
drawn by a fixed seed, log-uniform on [``--min-bytes``, ``--max-bytes``] and rounded to 16. All of
them live side by side in one ``[n, T]`` arena (the packed form: offsets that are multiples of 16, so
the launch is on the vector form). On those buffers, interleaved round by round:

  * ``varlen_encode``            ``VarlenCodec.encode``: one launch,
  * ``loop_encode``              a loop of cached ``rs.encode`` calls, one per object,
  * ``padded_encode_batch``      ``rs.encode_batch`` on a copy padded to the longest object,
  * ``varlen_reconstruct_e``     ``VarlenCodec.reconstruct``, e = 1 and 4 lost chunks per stripe, a
                                 pattern per stripe,
  * ``loop_reconstruct_e``       a loop of cached ``rs.reconstruct`` calls.

Control: ``--objects`` uniform objects of ``--uniform-bytes`` through ``VarlenCodec`` and through
``encode_batch`` / ``reconstruct_batch`` on the same rows: what the block map costs where it buys
nothing. A window is ``--iters`` calls between two synchronisations, timed by the host clock (what a
caller waits for: the loops are host-bound) and, on a GPU, by device events. Reported per call: the
median and the range over ``--rounds`` interleaved rounds, the bytes the call moves (rows read plus
rows written, ``sum_b (k + e_b) C_b``; for the padded call the padded rows) and TB/s over them. Every
result is checked once against the clean stripes before anything is timed. The order of the calls
rotates by one per round, so that no call always follows a host-bound loop. Prints one JSON line.
``--device cpu`` runs a small size on CPU tensors.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--code", default="10:14", help="k:n")
    ap.add_argument("--matrix", default="cauchy")
    ap.add_argument("--objects", type=int, default=None)
    ap.add_argument("--min-bytes", type=int, default=None, help="shortest chunk of the mixed batch")
    ap.add_argument("--max-bytes", type=int, default=None, help="longest chunk of the mixed batch")
    ap.add_argument("--uniform-bytes", type=int, default=None, help="chunk of the uniform control")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--rounds", type=int, default=None, help="interleaved rounds")
    ap.add_argument("--iters", type=int, default=None, help="calls per timed window")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args(argv)
    small = args.device == "cpu"
    for name, big, little in (("objects", 256, 8), ("min_bytes", 4096, 64), ("max_bytes", 1 << 20, 2048),
                              ("uniform_bytes", 65536, 512), ("rounds", 15, 2), ("iters", 5, 1)):
        if getattr(args, name) is None:
            setattr(args, name, little if small else big)
    return args


def draw_lengths(np, count: int, lo: int, hi: int, seed: int):
    """Log-uniform on [lo, hi], rounded to a multiple of 16 (at least 16)."""
    u = np.random.default_rng(seed).uniform(np.log(lo), np.log(hi), size=count)
    return np.maximum((np.exp(u) / 16).round().astype(np.int64) * 16, 16)


class Arena:
    """``count`` stripes of n rows side by side in one ``[n, T]`` tensor, consistent, with the clean
    copy kept for checks. ``views[b]`` is stripe b as an ``[n, C_b]`` view."""

    def __init__(self, torch, np, rs, lengths, device, seed):
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        total = int(self.offsets[-1])
        torch.manual_seed(seed)
        self.t = torch.randint(0, 256, (rs.n, total), dtype=torch.uint8, device=device)
        self.views = [self.t[:, int(a): int(b)] for a, b in zip(self.offsets[:-1], self.offsets[1:])]
        for v in self.views:
            rs.encode(v[: rs.k], v[rs.k:])
        self.clean = self.t.clone()


def main(argv=None) -> int:
    args = parse_args(argv)
    import numpy as np
    import torch

    from gpu_rscode_amd import ReedSolomon, VarlenCodec

    cuda = args.device == "cuda"
    k, n = (int(v) for v in args.code.split(":"))
    rs = ReedSolomon(k, n, matrix=args.matrix)
    vl = VarlenCodec(rs)
    p, nobj = rs.p, args.objects
    rs._plans.capacity = 8 * nobj + 64  # every object's encode and repair plans stay cached: the loops never rebuild one

    def sync():
        if cuda:
            torch.cuda.synchronize()

    rng = np.random.default_rng(args.seed + 1)

    def patterns(e):
        return np.stack([np.sort(rng.permutation(n)[:e]) for _ in range(nobj)]).astype(np.int64)

    calls, moved, checks = {}, {}, []

    def add(name, fn, nbytes, check=None):
        calls[name], moved[name] = fn, int(nbytes)
        if check is not None:
            checks.append((name, fn, check))

    def same(arena):
        return lambda: bool(torch.equal(arena.t, arena.clean))

    # ---- the mixed batch ---------------------------------------------------------------------------
    lengths = draw_lengths(np, nobj, args.min_bytes, args.max_bytes, args.seed)
    mixed = Arena(torch, np, rs, lengths, args.device, args.seed)
    data, par = mixed.t[:k], mixed.t[k:]
    total, longest = int(lengths.sum()), int(lengths.max())
    add("varlen_encode", lambda: vl.encode(data, par, offsets=mixed.offsets), n * total, same(mixed))
    add("loop_encode", lambda: [rs.encode(v[:k], v[k:]) for v in mixed.views], n * total, same(mixed))
    padded = torch.zeros((nobj, k, longest), dtype=torch.uint8, device=args.device)
    for b, v in enumerate(mixed.views):
        padded[b, :, : v.shape[1]] = v[:k]
    padded_par = torch.zeros((nobj, p, longest), dtype=torch.uint8, device=args.device)

    def padded_ok():
        return all(bool(torch.equal(padded_par[b, :, : v.shape[1]], v[k:])) for b, v in enumerate(mixed.views))
    add("padded_encode_batch", lambda: rs.encode_batch(padded, padded_par), n * nobj * longest, padded_ok)
    lost = {e: patterns(e) for e in (1, min(4, p))}
    for e, ids in lost.items():
        lists = [row.tolist() for row in ids]
        add(f"varlen_reconstruct_{e}", lambda ids=ids: vl.reconstruct(mixed.t, ids, offsets=mixed.offsets),
            (k + e) * total, same(mixed))
        add(f"loop_reconstruct_{e}", lambda lists=lists: [rs.reconstruct(v, er) for v, er in zip(mixed.views, lists)],
            (k + e) * total, same(mixed))

    # ---- the uniform control -----------------------------------------------------------------------
    c = args.uniform_bytes // 16 * 16
    uni = Arena(torch, np, rs, np.full(nobj, c, dtype=np.int64), args.device, args.seed + 2)
    as3d = uni.t.view(n, nobj, c).permute(1, 0, 2)  # the same rows as [B, n, C]
    ud, up, bd, bp = uni.t[:k], uni.t[k:], as3d[:, :k], as3d[:, k:]
    add("uniform_varlen_encode", lambda: vl.encode(ud, up, offsets=uni.offsets), n * nobj * c, same(uni))
    add("uniform_encode_batch", lambda: rs.encode_batch(bd, bp), n * nobj * c, same(uni))
    for e, ids in lost.items():
        add(f"uniform_varlen_reconstruct_{e}", lambda ids=ids: vl.reconstruct(uni.t, ids, offsets=uni.offsets),
            (k + e) * nobj * c, same(uni))
        add(f"uniform_reconstruct_batch_{e}", lambda ids=ids: rs.reconstruct_batch(as3d, ids), (k + e) * nobj * c,
            same(uni))

    # ---- every call once, checked: a repair of a clean stripe must leave it as it was; then damage the
    # rows the repairs rewrite and check that they come back
    for name, fn, check in checks:
        fn()
        sync()
        if not check():
            print(json.dumps({"error": f"{name}: wrong result"}))
            return 1
    for arena in (mixed, uni):
        for e, ids in lost.items():
            for b, v in enumerate(arena.views):
                v[ids[b].tolist()] = 0x5A
            calls[f"{'varlen' if arena is mixed else 'uniform_varlen'}_reconstruct_{e}"]()
            sync()
            if not torch.equal(arena.t, arena.clean):
                print(json.dumps({"error": f"varlen reconstruct of {e} lost chunks: wrong result"}))
                return 1

    # ---- timing: interleaved rounds ------------------------------------------------------------------
    def window(fn):
        sync()
        if cuda:
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        if cuda:
            t.record()
        sync()
        host = (time.perf_counter() - t0) * 1e6 / args.iters
        return host, (s.elapsed_time(t) * 1e3 / args.iters if cuda else host)

    for fn in calls.values():
        window(fn)
    host = {name: [] for name in calls}
    dev = {name: [] for name in calls}
    names = list(calls)
    for r in range(args.rounds):
        # the order rotates by one call per round: a window that follows a host-bound loop (the GPU nearly
        # idle for 100 ms, its clocks down) runs slow, and with a fixed order that was always the same call
        for name in names[r % len(names):] + names[: r % len(names)]:
            fn = calls[name]
            h, d = window(fn)
            host[name].append(h)
            dev[name].append(d)

    timings = {}
    for name in calls:
        med = statistics.median(host[name])
        timings[name] = {
            "median_us": round(med, 2), "min_us": round(min(host[name]), 2), "max_us": round(max(host[name]), 2),
            "device_median_us": round(statistics.median(dev[name]), 2),
            "bytes": moved[name], "TBps": round(moved[name] / med / 1e6, 4),
        }

    def ratio(a, b):
        return round(timings[a]["median_us"] / timings[b]["median_us"], 3)

    ratios = {
        "loop_encode / varlen_encode": ratio("loop_encode", "varlen_encode"),
        "padded_encode_batch / varlen_encode": ratio("padded_encode_batch", "varlen_encode"),
        "padded bytes / varlen bytes": round(moved["padded_encode_batch"] / moved["varlen_encode"], 3),
        "uniform_varlen_encode / uniform_encode_batch": ratio("uniform_varlen_encode", "uniform_encode_batch"),
    }
    for e in lost:
        ratios[f"loop_reconstruct_{e} / varlen_reconstruct_{e}"] = ratio(f"loop_reconstruct_{e}", f"varlen_reconstruct_{e}")
        ratios[f"uniform_varlen_reconstruct_{e} / uniform_reconstruct_batch_{e}"] = ratio(
            f"uniform_varlen_reconstruct_{e}", f"uniform_reconstruct_batch_{e}")
    res = {
        "device": torch.cuda.get_device_name(0) if cuda else "cpu", "code": [k, n], "matrix": args.matrix,
        "objects": nobj, "seed": args.seed, "rounds": args.rounds, "iters": args.iters,
        "mixed": {"min_bytes": int(lengths.min()), "max_bytes": longest, "mean_bytes": round(total / nobj, 1),
                  "sum_bytes": total},
        "uniform_bytes": c, "clock": "host clock around a synchronise, per call", "timings": timings, "ratios": ratios,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
