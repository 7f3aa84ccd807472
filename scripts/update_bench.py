#!/usr/bin/env python3
"""Time the in-place parity update against the re-encode it replaces.

One process, one device-resident stripe in ``alloc_rows`` buffers per code: (10, 14) with
107,374,183-byte chunks and (128, 160) with 8 MiB chunks by default. After a warm-up of every call
it alternates, round by round,

  * ``update`` for d = 1, 2, 4 changed natives   (2 d + 2 p rows moved; past 8 changed natives the
    update runs as passes of 8 and each pass reads and writes the parity rows again),
  * ``update_delta`` for d = 1                    (d + 2 p rows moved),
  * ``write`` for d = 1                           (the native overwritten in the same pass: 3 d + 2 p),
  * ``encode``                                    (k + p rows moved),

each timed with device events over ``--reps`` calls, and prints the median and the spread (min,
max) over the rounds, the achieved bytes/s over the rows each call moves, and the first d at which
``update`` no longer beats ``encode`` (``--sweep`` adds further d to find it). No time is fixed in
advance: the comparison is ``encode`` on the same buffers in the same run. Prints one JSON object
per code (also appended to ``--out``).

``--batch`` times the batched small-object form instead: B stripes of ``--batch-codes`` (256 stripes of
(10, 14) with 64 KiB and with 1 MiB chunks, and of (128, 160) with 64 KiB chunks), d = 1 with a random
native per stripe, alternating ``update_batch`` (one launch), a loop of B cached ``update`` calls on
the same buffers (B launches) and ``encode_batch`` on the same buffers.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_CODES = "10:14:107374183,128:160:8388608"
DEFAULT_BATCH_CODES = "10:14:65536:256,10:14:1048576:256,128:160:65536:256"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codes", default=DEFAULT_CODES, help="comma-separated k:n:bytes-per-chunk")
    ap.add_argument("--matrix", default="cauchy")
    ap.add_argument("--rounds", type=int, default=15, help="alternations of the timed calls")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--sweep", default="8", help="further d for update, comma-separated (where k allows)")
    ap.add_argument("--batch", action="store_true", help="time update_batch for the --batch-codes shapes instead")
    ap.add_argument("--batch-codes", default=DEFAULT_BATCH_CODES, help="comma-separated k:n:bytes-per-chunk:stripes")
    ap.add_argument("--out", default=None, help="also append the JSON lines here")
    return ap.parse_args(argv)


def spread(ms: list[float]) -> dict:
    return {"median_us": round(statistics.median(ms) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2),
            "max_us": round(max(ms) * 1e3, 2)}


def bench_code(torch, k: int, n: int, C: int, args) -> dict:
    from gpu_rscode_amd import ReedSolomon, alloc_rows, flat_rows
    from gpu_rscode_amd.ops import fill_random_
    from gpu_rscode_amd.ops.update import MAX_D

    p = n - k
    rs = ReedSolomon(k, n, matrix=args.matrix)
    ds = sorted({1, 2, 4} | {int(d) for d in args.sweep.split(",") if d})
    ds = [d for d in ds if d <= k]
    dmax = max(ds)
    stripe = alloc_rows(n, C, "cuda")
    fresh = alloc_rows(dmax, C, "cuda")
    fill_random_(flat_rows(stripe), seed=1)
    fill_random_(flat_rows(fresh), seed=2)
    data, parity = stripe[:k], stripe[k:]
    rs.encode(data, parity)
    step = 3 if k % 3 else 1
    changed = {d: [(3 + step * t) % k for t in range(d)] for d in ds}
    assert all(len(set(c)) == d for d, c in changed.items())

    # once, untimed: an update, then a write, leave the parity equal to an encode of the natives
    d0 = ds[-1]
    old = torch.stack([data[j] for j in changed[d0]])
    rs.update(parity, changed[d0], old, fresh[:d0])
    for t, j in enumerate(changed[d0]):
        data[j].copy_(fresh[t])
    assert rs.verify(data, parity), "update differs from a re-encode"
    rs.write(stripe, changed[1], fresh[1:2])
    assert rs.verify(data, parity) and torch.equal(data[changed[1][0]], fresh[1]), "write differs from a re-encode"
    del old

    def window(fn, reps) -> float:
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / reps

    # `old` rows of their own (not the stripe's natives): every call of the timed loop reads the same
    # bytes; what the parity rows then hold is of no interest, the encode puts them right again
    olds = alloc_rows(dmax, C, "cuda")
    fill_random_(flat_rows(olds), seed=3)
    calls, rows = {}, {}
    for d in ds:
        calls[f"update_d{d}"] = (lambda d=d: rs.update(parity, changed[d], olds[:d], fresh[:d]))
        rows[f"update_d{d}"] = 2 * d + 2 * p * -(-d // MAX_D)
    calls["update_delta_d1"] = lambda: rs.update_delta(parity, changed[1], olds[:1])
    rows["update_delta_d1"] = 1 + 2 * p
    calls["write_d1"] = lambda: rs.write(stripe, changed[1], fresh[:1])
    rows["write_d1"] = 3 + 2 * p
    calls["encode"] = lambda: rs.encode(data, parity)
    rows["encode"] = k + p
    for fn in calls.values():  # warm-up: code objects, plans, the allocator's blocks
        window(fn, 3)
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, args.reps))
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C}, "rounds": args.rounds, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    med = {name: statistics.median(ms) for name, ms in times.items()}
    for name, ms in times.items():
        res[name] = spread(ms)
        res[name]["rows_moved"] = rows[name]
        res[name]["TBps"] = round(rows[name] * C / (med[name] * 1e-3) / 1e12, 3)
        res[name]["over_encode"] = round(med[name] / med["encode"], 3)
    slower = [d for d in ds if med[f"update_d{d}"] >= med["encode"]]
    res["update_stops_beating_encode_at_d"] = slower[0] if slower else None
    res["d_timed"] = ds
    res["bytes_predict_update_d1_over_encode"] = round((2 + 2 * p) / (k + p), 3)
    rs.encode(data, parity)
    assert rs.verify(data, parity)
    return res


def bench_batch(torch, k: int, n: int, C: int, B: int, args) -> dict:
    """update_batch against a loop of B cached update calls and against encode_batch, d = 1."""
    import numpy as np

    from gpu_rscode_amd import ReedSolomon
    from gpu_rscode_amd.models.rs import row_pitch
    from gpu_rscode_amd.ops import fill_random_

    p = n - k
    rs = ReedSolomon(k, n, matrix=args.matrix)
    pitch = row_pitch(C, "cuda")

    def rows(r, seed):  # [B, r, C] over pitched storage, as encode_batch allocates its parity
        base = torch.empty(B * r * pitch, dtype=torch.uint8, device="cuda")
        fill_random_(base, seed=seed)
        return base.as_strided((B, r, C), (r * pitch, pitch, 1))

    data, parity, fresh, olds = rows(k, 1), rows(p, 2), rows(1, 3), rows(1, 4)
    ids = np.random.default_rng(5).integers(0, k, size=(B, 1))
    rs.encode_batch(data, parity)

    # once, untimed: the batched update of every stripe's own native leaves a consistent stripe
    for b in range(B):
        olds[b, 0].copy_(data[b, int(ids[b, 0])])
    rs.update_batch(parity, ids, olds, fresh)
    for b in range(B):
        data[b, int(ids[b, 0])].copy_(fresh[b, 0])
    assert not bool(rs.syndrome_mask_batch(data, parity).any()), "update_batch differs from a re-encode"

    def window(fn, reps) -> float:
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        t.record()
        t.synchronize()
        return s.elapsed_time(t) / reps

    # the loop's arguments made once: a repeated update call is dict lookups and one launch
    single = [(parity[b], [int(ids[b, 0])], olds[b], fresh[b]) for b in range(B)]

    def loop():
        for par, ch, old, new in single:
            rs.update(par, ch, old, new)

    calls = {"update_batch": lambda: rs.update_batch(parity, ids, olds, fresh), "update_loop": loop,
             "encode_batch": lambda: rs.encode_batch(data, parity)}
    for fn in calls.values():  # warm-up: code objects, plans, the allocator's blocks
        window(fn, 3)
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, args.reps))
    med = {name: statistics.median(ms) for name, ms in times.items()}
    moved = {"update_batch": 2 + 2 * p, "update_loop": 2 + 2 * p, "encode_batch": k + p}
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "stripes": B, "d": 1}, "rounds": args.rounds,
           "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name, ms in times.items():
        res[name] = spread(ms)
        res[name]["rows_moved_per_stripe"] = moved[name]
        res[name]["TBps"] = round(moved[name] * C * B / (med[name] * 1e-3) / 1e12, 3)
    res["loop_over_batch"] = round(med["update_loop"] / med["update_batch"], 2)
    res["batch_over_encode_batch"] = round(med["update_batch"] / med["encode_batch"], 3)
    res["bytes_predict_batch_over_encode_batch"] = round((2 + 2 * p) / (k + p), 3)
    rs.encode_batch(data, parity)
    assert not bool(rs.syndrome_mask_batch(data, parity).any())
    return res


def main(argv=None) -> int:
    args = parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        print("update_bench.py needs a GPU", file=sys.stderr)
        return 2
    base_tune = os.environ.pop("GFRS_TUNE", None)
    if base_tune:
        print(f"ignoring GFRS_TUNE={base_tune}", file=sys.stderr)
    lines = []
    for spec in (args.batch_codes if args.batch else args.codes).split(","):
        if args.batch:
            line = json.dumps(bench_batch(torch, *(int(v) for v in spec.split(":")), args))
        else:
            k, n, C = (int(v) for v in spec.split(":"))
            line = json.dumps(bench_code(torch, k, n, C, args))
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
