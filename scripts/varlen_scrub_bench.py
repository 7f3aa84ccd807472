#!/usr/bin/env python3
"""Time the scrub of a variable-length batch against what a caller with mixed object sizes does today.

One process, one code ((10, 14) cauchy by default), ``--objects`` objects whose chunk lengths are drawn
by a fixed seed, log-uniform on [``--min-bytes``, ``--max-bytes``] and rounded to 16 (the batch of
scripts/varlen_bench.py). All of them live side by side in one ``[n, T]`` arena (the packed form, on the
vector form of the kernel). On those buffers, interleaved round by round:

  * ``varlen_syndrome_mask``     ``VarlenCodec.syndrome_mask``: one launch, nothing stored when clean,
  * ``loop_syndrome_mask``       a loop of cached ``rs.syndrome_mask`` calls, one per object,
  * ``padded_syndrome_mask_batch``  ``rs.syndrome_mask_batch`` on a copy padded to the longest object,
  * ``varlen_encode``            ``VarlenCodec.encode`` on the same buffers: the yardstick of the kernel. It
                                 reads the same rows (k of the n) and also stores p of them,
  * ``varlen_scrub_clean``       ``VarlenCodec.scrub`` (both kernels and the sync) on the clean batch,
  * ``varlen_scrub_one_chunk``   the same with one chunk of one object (a copy of the arena) overwritten,
  * ``varlen_heal_32``           ``VarlenCodec.heal`` of 32 objects with one overwritten chunk each: scrub,
                                 one repair launch, scrub again; the damage is put back before each call
                                 by one copy that is inside the timed window (``restore_32`` times it alone).

Control: ``--objects`` uniform objects of ``--uniform-bytes`` through ``VarlenCodec.syndrome_mask`` and
through ``syndrome_mask_batch`` on the same rows: what the work list costs where it buys nothing.

A window is ``--iters`` calls between two synchronisations, timed by the host clock (what a caller waits
for) and, on a GPU, by device events. Reported per call: the median and the min-max range over
``--rounds`` interleaved rounds (at least five), the bytes the call reads and TB/s over them. Every
result is checked once before anything is timed. The order of the calls rotates by one per round, so
that no call always follows a host-bound loop. Prints one JSON line. ``--device cpu`` runs a small size
on CPU tensors.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--code", default="10:14", help="k:n")
    ap.add_argument("--matrix", default="cauchy")
    ap.add_argument("--objects", type=int, default=None)
    ap.add_argument("--min-bytes", type=int, default=None, help="shortest chunk of the mixed batch")
    ap.add_argument("--max-bytes", type=int, default=None, help="longest chunk of the mixed batch")
    ap.add_argument("--uniform-bytes", type=int, default=None, help="chunk of the uniform control")
    ap.add_argument("--block-bytes", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--rounds", type=int, default=None, help="interleaved rounds, at least 5")
    ap.add_argument("--iters", type=int, default=None, help="calls per timed window")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args(argv)
    small = args.device == "cpu"
    for name, big, little in (("objects", 256, 8), ("min_bytes", 4096, 64), ("max_bytes", 1 << 20, 2048),
                              ("uniform_bytes", 65536, 512), ("rounds", 15, 5), ("iters", 5, 1)):
        if getattr(args, name) is None:
            setattr(args, name, little if small else big)
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    import numpy as np
    import torch

    from gpu_rscode_amd import ReedSolomon, VarlenCodec
    from varlen_bench import Arena, draw_lengths

    cuda = args.device == "cuda"
    k, n = (int(v) for v in args.code.split(":"))
    rs = ReedSolomon(k, n, matrix=args.matrix)
    vl = VarlenCodec(rs)
    nobj, bb = args.objects, args.block_bytes
    rs._plans.capacity = 8 * nobj + 64  # every object's plan stays cached: the loop never rebuilds one

    def sync():
        if cuda:
            torch.cuda.synchronize()

    calls, moved, checks = {}, {}, []

    def add(name, fn, nbytes, check=None):
        calls[name], moved[name] = fn, int(nbytes)
        if check is not None:
            checks.append((name, fn, check))

    # ---- the mixed batch ---------------------------------------------------------------------------
    lengths = draw_lengths(np, nobj, args.min_bytes, args.max_bytes, args.seed)
    mixed = Arena(torch, np, rs, lengths, args.device, args.seed)
    total, longest = int(lengths.sum()), int(lengths.max())
    nwords = int(sum(-(-int(c) // bb) for c in lengths))

    def clean_mask(m):
        return m.blocks.numel() == nwords and not bool(m.blocks.any()) and not bool(m.stripes.any())
    add("varlen_syndrome_mask", lambda: vl.syndrome_mask(mixed.t, offsets=mixed.offsets, block_bytes=bb), n * total,
        clean_mask)
    add("loop_syndrome_mask", lambda: [rs.syndrome_mask(v, block_bytes=bb) for v in mixed.views], n * total,
        lambda ms: not any(bool(m.any()) for m in ms))
    padded = torch.zeros((nobj, n, longest), dtype=torch.uint8, device=args.device)
    for b, v in enumerate(mixed.views):
        padded[b, :, : v.shape[1]] = v
    add("padded_syndrome_mask_batch", lambda: rs.syndrome_mask_batch(padded, block_bytes=bb), n * nobj * longest,
        lambda m: not bool(m.any()))
    add("varlen_encode", lambda: vl.encode(mixed.t[:k], mixed.t[k:], offsets=mixed.offsets), n * total,
        lambda _: bool(torch.equal(mixed.t, mixed.clean)))
    add("varlen_scrub_clean", lambda: vl.scrub(mixed.t, offsets=mixed.offsets, block_bytes=bb), n * total,
        lambda r: bool(r.clean.all()))
    # one chunk of one object wrong, in a copy of the arena (the median object by length)
    one = mixed.t.clone()
    victim = int(np.argsort(lengths)[nobj // 2])
    lo, hi = int(mixed.offsets[victim]), int(mixed.offsets[victim + 1])
    one[3, lo:hi] ^= 0x5A
    add("varlen_scrub_one_chunk", lambda: vl.scrub(one, offsets=mixed.offsets, block_bytes=bb), n * total,
        lambda r: r.dirty == [victim] and r.report[victim].suspects == [3]
        and int(r.bad_columns[victim]) == hi - lo)
    # 32 damaged objects (every eighth by length order), healed; the damage put back by one copy
    nheal = min(32, nobj)
    hurt = np.sort(np.argsort(lengths)[:: max(1, nobj // nheal)][:nheal])
    work = mixed.t.clone()
    dirty = mixed.t.clone()
    for i, b in enumerate(hurt):
        dirty[(3 * i) % n, int(mixed.offsets[b]): int(mixed.offsets[b + 1])] ^= 0xC3

    def heal():
        work.copy_(dirty)
        return vl.heal(work, offsets=mixed.offsets)
    add("varlen_heal_32", heal, n * total * 2 + n * int(lengths[hurt].sum()),
        lambda r: bool(r.clean.all()) and r.unhealed == [] and bool(torch.equal(work, mixed.clean)))
    add("restore_32", lambda: work.copy_(dirty), 2 * n * total)

    # ---- the uniform control -----------------------------------------------------------------------
    c = args.uniform_bytes // 16 * 16
    uni = Arena(torch, np, rs, np.full(nobj, c, dtype=np.int64), args.device, args.seed + 2)
    as3d = uni.t.view(n, nobj, c).permute(1, 0, 2)  # the same rows as [B, n, C]
    add("uniform_varlen_syndrome_mask", lambda: vl.syndrome_mask(uni.t, offsets=uni.offsets, block_bytes=bb),
        n * nobj * c, lambda m: not bool(m.blocks.any()))
    add("uniform_syndrome_mask_batch", lambda: rs.syndrome_mask_batch(as3d, block_bytes=bb), n * nobj * c,
        lambda m: not bool(m.any()))

    for name, fn, check in checks:
        out = fn()
        sync()
        if not check(out):
            print(json.dumps({"error": f"{name}: wrong result"}))
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
        for name in names[r % len(names):] + names[: r % len(names)]:
            h, d = window(calls[name])
            host[name].append(h)
            dev[name].append(d)

    timings = {}
    for name in calls:
        med = statistics.median(host[name])
        timings[name] = {
            "median_us": round(med, 2), "min_us": round(min(host[name]), 2), "max_us": round(max(host[name]), 2),
            "device_median_us": round(statistics.median(dev[name]), 2),
            "device_min_us": round(min(dev[name]), 2), "device_max_us": round(max(dev[name]), 2),
            "bytes": moved[name], "TBps": round(moved[name] / med / 1e6, 4),
        }

    def ratio(a, b):
        return round(timings[a]["median_us"] / timings[b]["median_us"], 3)

    ratios = {
        "loop_syndrome_mask / varlen_syndrome_mask": ratio("loop_syndrome_mask", "varlen_syndrome_mask"),
        "padded_syndrome_mask_batch / varlen_syndrome_mask": ratio("padded_syndrome_mask_batch", "varlen_syndrome_mask"),
        "padded bytes / varlen bytes": round(moved["padded_syndrome_mask_batch"] / moved["varlen_syndrome_mask"], 3),
        "varlen_syndrome_mask / varlen_encode": ratio("varlen_syndrome_mask", "varlen_encode"),
        "uniform_varlen_syndrome_mask / uniform_syndrome_mask_batch": ratio("uniform_varlen_syndrome_mask",
                                                                           "uniform_syndrome_mask_batch"),
    }
    res = {
        "device": torch.cuda.get_device_name(0) if cuda else "cpu", "code": [k, n], "matrix": args.matrix,
        "objects": nobj, "seed": args.seed, "rounds": args.rounds, "iters": args.iters, "block_bytes": bb,
        "mixed": {"min_bytes": int(lengths.min()), "max_bytes": longest, "mean_bytes": round(total / nobj, 1),
                  "sum_bytes": total},
        "uniform_bytes": c, "healed_objects": int(hurt.size),
        "clock": "host clock around a synchronise, per call", "timings": timings, "ratios": ratios,
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
