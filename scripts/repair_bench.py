#!/usr/bin/env python3
"""Time the batched repair against the loop of single repairs it replaces.

One process; per shape B device-resident stripes of ``--cols`` bytes at ``--code k:n`` in one pitched
``[B, n, C]`` buffer, encoded, with chunks ``(b + t) % n`` (``t < --erasures``) of stripe b overwritten:
a pattern per stripe. After one untimed repair (checked with ``syndrome_mask_batch``) and a warm-up of
every call it alternates, round by round,

  * ``reconstruct_batch``   one call, one launch, per-stripe coefficient tables (k + e rows moved),
  * ``reconstruct_loop``    B cached ``reconstruct`` calls on the same buffers (B launches),
  * ``decode_batch``        ONE pattern shared by the batch (natives 0..e-1 lost) on the same shapes:
                            the shared-table bound (it also copies the surviving natives: 2 k rows moved),
  * ``encode_batch``        on the same buffers (k + p rows moved),
  * ``heal_batch``          end to end (scrub, one batched repair, scrub again) with ONE bad chunk per
                            stripe, chunk ``b % n``, put back before every call outside the timed window,

each window timed twice over the same calls: by device events, and by the host clock around a
synchronise. Prints per shape one JSON object (also appended to ``--out``) with the median and the
spread (min, max) over the rounds of both clocks, the ratios of the medians, and whether the batched
call and the loop are apart by more than both spreads. No time is fixed in advance.

Without ``--code`` it runs the recorded shapes: 256 x 64 KiB and 256 x 1 MiB at (10, 14) with one and
four erasures per stripe, and 256 x 64 KiB at (128, 160) with one.

``--fresh`` times what the above leaves out, the FIRST call: ``reconstruct_batch`` on fresh buffers with
B distinct patterns that nobody has solved (planning plus launch, host clock up to a synchronise) with
the host solve and with ``device_solve=True``, round by round in turn with the codec's caches emptied,
then the cached call of both plans, and a single ``reconstruct`` both ways: 256 x 64 KiB at (10, 14)
with 1 and 4 erasures and at (128, 160) with 1 and 32. ``--device cpu`` runs small shapes end to end.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_SHAPES = "10:14:65536:256:1,10:14:65536:256:4,10:14:1048576:256:1,10:14:1048576:256:4,128:160:65536:256:1"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default=None, help="k:n (with --cols, --stripes, --erasures: one shape)")
    ap.add_argument("--cols", type=int, default=65536, help="bytes per chunk")
    ap.add_argument("--stripes", type=int, default=256)
    ap.add_argument("--erasures", type=int, default=1, help="erased chunks per stripe")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated k:n:cols:stripes:erasures (no --code)")
    ap.add_argument("--matrix", default="cauchy")
    ap.add_argument("--rounds", type=int, default=9, help="alternations of the timed calls")
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines here")
    ap.add_argument("--fresh", action="store_true",
                    help="time the FIRST reconstruct_batch / reconstruct call on fresh buffers and patterns, with the "
                         "host solve and with device_solve=True, and the cached call of both")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                    help="with --fresh: cpu runs small shapes end to end (device_solve is ignored there)")
    return ap.parse_args(argv)


def spread(ms: list[float]) -> dict:
    return {"median_us": round(statistics.median(ms) * 1e3, 2), "min_us": round(min(ms) * 1e3, 2),
            "max_us": round(max(ms) * 1e3, 2)}


def apart(a: list[float], b: list[float]) -> bool:
    """Medians apart by more than both spreads."""
    gap = abs(statistics.median(a) - statistics.median(b))
    return gap > max(a) - min(a) and gap > max(b) - min(b)


def bench_shape(torch, k: int, n: int, C: int, B: int, e: int, args) -> dict:
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

    stripes, noise = rows(n, 1), rows(1, 2)
    data, parity = stripes[:, :k], stripes[:, k:]
    rs.encode_batch(data, parity)
    erased = (np.arange(B)[:, None] + np.arange(e)[None, :]) % n
    flat = stripes.as_strided((B * n, C), (pitch, 1))  # row b * n + i = chunk i of stripe b
    one_bad = torch.from_numpy(np.arange(B) * n + np.arange(B) % n).cuda()
    all_bad = torch.from_numpy((np.arange(B)[:, None] * n + erased).reshape(-1)).cuda()

    def damage(idx):
        flat.index_copy_(0, idx, noise[:, 0].repeat_interleave(idx.numel() // B, dim=0))

    # once, untimed: the batched repair of every stripe's own chunks leaves consistent stripes
    good = data.clone()
    damage(all_bad)
    assert bool(rs.syndrome_mask_batch(stripes).any(dim=1).all())
    rs.reconstruct_batch(stripes, erased)
    assert not bool(rs.syndrome_mask_batch(stripes).any()) and torch.equal(data, good), "reconstruct_batch is wrong"
    del good

    def window(fn, reps, before=None) -> tuple[float, float]:
        """(device-event ms, host-clock ms) per call over the same ``reps`` calls."""
        ev = host = 0.0
        for _ in range(reps if before else 1):
            if before:
                before()
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.record()
            for _ in range(1 if before else reps):
                fn()
            t.record()
            torch.cuda.synchronize()
            host += (time.perf_counter() - t0) * 1e3
            ev += s.elapsed_time(t)
        return ev / reps, host / reps

    # the loop's arguments made once; the shared pattern of decode_batch: natives 0..e-1 lost
    single = [(stripes[b], [int(i) for i in erased[b]]) for b in range(B)]

    def loop():
        for stripe, ids in single:
            rs.reconstruct(stripe, ids)

    shared = list(range(e, k)) + list(range(k, k + e))
    survivors, out = rows(k, 3), rows(k, 4)
    calls = {"reconstruct_batch": (lambda: rs.reconstruct_batch(stripes, erased), None),
             "reconstruct_loop": (loop, None),
             "decode_batch": (lambda: rs.decode_batch(survivors, shared, out), None),
             "encode_batch": (lambda: rs.encode_batch(data, parity), None)}
    if p <= 16:  # (scrub locates chunks for p <= 16)
        calls["heal_batch"] = (lambda: rs.heal_batch(stripes), lambda: damage(one_bad))
    for fn, before in calls.values():  # warm-up: code objects, plans, the allocator's blocks
        window(fn, 2, before)
    times = {name: ([], []) for name in calls}
    for _ in range(args.rounds):
        for name, (fn, before) in calls.items():
            ev, host = window(fn, args.reps, before)
            times[name][0].append(ev)
            times[name][1].append(host)
    moved = {"reconstruct_batch": k + e, "reconstruct_loop": k + e, "decode_batch": 2 * k, "encode_batch": k + p}
    res = {"shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "stripes": B, "erasures": e},
           "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    med = {name: statistics.median(ev) for name, (ev, _) in times.items()}
    for name, (ev, host) in times.items():
        res[name] = {"events": spread(ev), "host": spread(host)}
        if name in moved:
            res[name]["rows_moved_per_stripe"] = moved[name]
            res[name]["TBps"] = round(moved[name] * C * B / (med[name] * 1e-3) / 1e12, 3)
    for clock, i in (("events", 0), ("host", 1)):
        a, b = times["reconstruct_batch"][i], times["reconstruct_loop"][i]
        res[f"loop_over_batch_{clock}"] = round(statistics.median(b) / statistics.median(a), 2)
        res[f"batch_beats_loop_{clock}"] = statistics.median(a) < statistics.median(b) and apart(a, b)
    res["batch_over_decode_batch"] = round(med["reconstruct_batch"] / med["decode_batch"], 3)
    res["batch_over_encode_batch"] = round(med["reconstruct_batch"] / med["encode_batch"], 3)
    res["bytes_predict_batch_over_decode_batch"] = round((k + e) / (2 * k), 3)
    assert not bool(rs.syndrome_mask_batch(stripes).any()), "the stripes are not consistent after the timed calls"
    return res


def fresh_patterns(np, n: int, e: int, B: int, seed: int):
    """``[B, e]`` erased ids, distinct patterns as far as the code has them (C(n, e) < B: reused in turn)."""
    import itertools
    import math

    rng = np.random.default_rng(seed)
    if math.comb(n, e) <= 4 * B:
        every = list(itertools.combinations(range(n), e))
        pick = [every[i] for i in rng.permutation(len(every))[:B]]
    else:
        pick = set()
        while len(pick) < B:
            pick.add(tuple(sorted(int(i) for i in rng.choice(n, size=e, replace=False))))
        pick = sorted(pick)
    return np.array([pick[b % len(pick)] for b in range(B)], dtype=np.int64), len(pick)


def bench_fresh(torch, k: int, n: int, C: int, B: int, e: int, args) -> dict:
    """The first ``reconstruct_batch`` call of B stripes with patterns nobody has solved yet (planning
    plus launch, timed by the host clock up to a device synchronise) with the host solve and with
    ``device_solve=True``, then the cached call of both plans, round by round in turn; and one
    ``reconstruct`` of a single stripe both ways. Every round takes fresh buffers and fresh patterns and
    empties the codec's caches first, so no decode matrix and no plan is reused."""
    import numpy as np

    from gpu_rscode_amd import ReedSolomon

    dev = args.device
    rs = ReedSolomon(k, n, matrix=args.matrix)
    cuda = dev == "cuda"
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    torch.manual_seed(1)

    def stripes_for(count):
        t = torch.zeros((count, n, C), dtype=torch.uint8, device=dev)
        t[:, :k] = torch.randint(0, 256, (count, k, C), dtype=torch.uint8, device=dev)
        if cuda:
            rs.encode_batch(t[:, :k], t[:, k:])
        else:
            for b in range(count):
                rs.encode(t[b, :k], t[b, k:])
        return t

    def forget():
        rs._dm.clear()
        rs._plans.clear()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def cached(fn):
        """Per call over ``--reps`` calls of a cached plan: device events on the GPU, else the host clock."""
        if not cuda:
            return timed(lambda: [fn() for _ in range(args.reps)]) / args.reps
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        s.record()
        for _ in range(args.reps):
            fn()
        t.record()
        sync()
        return s.elapsed_time(t) / args.reps

    good = stripes_for(B)
    names = ("host_solve", "device_solve")
    first = {m: [] for m in names}
    again = {m: [] for m in names}
    one_first = {m: [] for m in names}
    one_again = {m: [] for m in names}
    npat = 0
    for rnd in range(-1, args.rounds):  # round -1 is the warm-up: code objects, the allocator's blocks
        erased, npat = fresh_patterns(np, n, e, B, 100 + rnd)
        for m in names if rnd % 2 else names[::-1]:
            flag = m == "device_solve"
            work = good.clone()
            for b in range(B):
                work[b, erased[b].tolist()] = 0xEE
            forget()
            t_first = timed(lambda: rs.reconstruct_batch(work, erased, device_solve=flag))
            assert torch.equal(work, good), f"reconstruct_batch({m}) is wrong"
            t_again = cached(lambda: rs.reconstruct_batch(work, erased, device_solve=flag))
            one = good[0].clone()
            ids = erased[0].tolist()
            one[ids] = 0xEE
            forget()
            t_one = timed(lambda: rs.reconstruct(one, ids, device_solve=flag))
            assert torch.equal(one, good[0]), f"reconstruct({m}) is wrong"
            t_one_again = cached(lambda: rs.reconstruct(one, ids, device_solve=flag))
            if rnd >= 0:
                first[m].append(t_first)
                again[m].append(t_again)
                one_first[m].append(t_one)
                one_again[m].append(t_one_again)
    res = {"fresh": True, "shape": {"k": k, "n": n, "matrix": args.matrix, "cols": C, "stripes": B, "erasures": e,
                                    "distinct_patterns": npat},
           "rounds": args.rounds, "reps": args.reps,
           "device": torch.cuda.get_device_name(0) if cuda else "cpu (device_solve is ignored there)"}
    for m in names:
        res[m] = {"batch_first_call_host_clock": spread(first[m]), "batch_cached_call": spread(again[m]),
                  "single_first_call_host_clock": spread(one_first[m]), "single_cached_call": spread(one_again[m])}
    for what, t in (("batch_first_call", first), ("batch_cached_call", again), ("single_first_call", one_first),
                    ("single_cached_call", one_again)):
        a, b = t["host_solve"], t["device_solve"]
        res[f"{what}_host_over_device"] = round(statistics.median(a) / statistics.median(b), 2)
        res[f"{what}_apart"] = apart(a, b)
    return res


FRESH_SHAPES = "10:14:65536:256:1,10:14:65536:256:4,128:160:65536:256:1,128:160:65536:256:32"
FRESH_SHAPES_CPU = "10:14:1024:8:1,10:14:1024:8:4,128:160:256:3:1,128:160:256:3:32"


def main_fresh(args) -> int:
    import torch

    if args.device == "cuda" and not torch.cuda.is_available():
        print("repair_bench.py --fresh --device cuda needs a GPU", file=sys.stderr)
        return 2
    if args.code:
        k, n = (int(v) for v in args.code.split(":"))
        shapes = [(k, n, args.cols, args.stripes, args.erasures)]
    else:
        spec = args.shapes
        if spec == DEFAULT_SHAPES:
            spec = FRESH_SHAPES if args.device == "cuda" else FRESH_SHAPES_CPU
        shapes = [tuple(int(v) for v in s.split(":")) for s in spec.split(",")]
    lines = []
    for shape in shapes:
        line = json.dumps(bench_fresh(torch, *shape, args))
        print(line, flush=True)
        lines.append(line)
        if args.device == "cuda":
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main(argv=None) -> int:
    args = parse_args(argv)
    if args.fresh:
        return main_fresh(args)
    if args.device != "cuda":
        print("repair_bench.py --device cpu needs --fresh", file=sys.stderr)
        return 2
    import torch

    if not torch.cuda.is_available():
        print("repair_bench.py needs a GPU", file=sys.stderr)
        return 2
    base_tune = os.environ.pop("GFRS_TUNE", None)
    if base_tune:
        print(f"ignoring GFRS_TUNE={base_tune}", file=sys.stderr)
    if args.code:
        k, n = (int(v) for v in args.code.split(":"))
        shapes = [(k, n, args.cols, args.stripes, args.erasures)]
    else:
        shapes = [tuple(int(v) for v in spec.split(":")) for spec in args.shapes.split(",")]
    lines = []
    for shape in shapes:
        line = json.dumps(bench_shape(torch, *shape, args))
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
