#!/usr/bin/env python3
"""Time `QuerySelector.select` per call -- the vision-query selection in front of a forward, without the forward -- for a bank held as the CPU
dict `load_query_bank(path)` reads from a file (what `online_update` leaves in the model; the code of the dict path) and for a resident
`QueryBank` (integer tables on the host, one upload, one mq_bank_select_fwd launch).

  online : 40 labels x 100 rows, NUM_QUERY_PER_CLASS 5, 8 images sharing one caption, T = 256, C = 256, one scale: every call draws
  lvis   : the chunk protocol, 31 captions of 40 labels x 2 images = 62 items with their own label lists, 5 rows per label (no draw)

Each path: `--warmup` calls (default 3), then `--calls` timed ones (default 20), each from the call to the end of a device synchronise.  One
JSON line per shape: every call of both paths, the medians, the dict path's spread (max - min) and the ratio of the medians.  Before timing,
both paths are run once after the same `np.random.seed` and must give equal outputs.

`--row-add`: per shape a second JSON line for the launch alone, from device events around it (ops.start_timing): mq_bank_select_fwd against
mq_bank_select_add_fwd (VISION_QUERY.ADD_VISION_LAYER, a seeded non-zero `tunable_vision_linear.weight`), `--calls` x 10 launches each,
alternating in blocks of `--calls`.  The addend costs one more fp32 row read per real output row: the line reports that traffic, the time it
would take at the bytes/s the plain launch achieves (the bound), and the measured difference beside it.

    python tools/query_select_bench.py [--calls 20] [--warmup 3] [--shape online|lvis|both] [--row-add]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.modeling.query_selector import QuerySelector  # noqa: E402
from mq_det_amd.query_bank import QueryBank  # noqa: E402

DEV = torch.device("cuda:0")
C, T, K = 256, 256, 5
ROW_ADD = False


def make_bank(n_labels, rows, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(n_labels * rows, 1, C, generator=g)
    labels = torch.arange(1, n_labels + 1).repeat_interleave(rows)
    bank = QueryBank(DEV)
    assert bank.update(feats.to(DEV), labels.to(DEV), rows) == n_labels * rows
    return bank


def selectors(bank, tmp):
    """(dict path, resident path): the first reads the bank back from the file `online_update` writes"""
    cfg = get_cfg()
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS = K
    path = os.path.join(tmp, "bank.pth")
    bank.save(path)
    plain, resident = QuerySelector(cfg), QuerySelector(cfg)
    plain.load_query_bank(path)
    resident.load_query_bank(bank)
    return plain, resident


def caption(labels, rng, per=3):
    """label -> `per` consecutive token positions somewhere in the caption (40 labels x 3 tokens fill about half of T)"""
    starts = np.sort(rng.choice(T // per, len(labels), replace=False)) * per
    return {int(l): list(range(int(s), int(s) + per)) for l, s in zip(labels, starts)}


def timed(sel, args, calls, warmup):
    out = []
    for r in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sel.select(*args)
        torch.cuda.synchronize()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def launch_us(sel, args, calls):
    """mean device time of the bank_select launch over `calls` selects, in microseconds, and its algorithmic bytes"""
    from mq_det_amd import ops
    ops.start_timing()
    try:
        for _ in range(calls):
            sel.select(*args)
    finally:
        rec = ops.stop_timing()
    n, ms, nbytes = rec["bank_select"]
    assert n == calls and set(rec) == {"bank_select"}, rec
    return ms * 1e3 / n, nbytes // n


def measure_row_add(shape, bank, args, calls, warmup, extra):
    cfg = get_cfg()
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS = K
    plain = QuerySelector(cfg)
    plain.load_query_bank(bank)
    cfg = get_cfg()
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS, cfg.VISION_QUERY.ADD_VISION_LAYER = K, True
    add = QuerySelector(cfg)
    add.load_query_bank(bank)
    wv = torch.randn(1000, C, generator=torch.Generator().manual_seed(3))
    add.load_state_dict({"tunable_vision_linear.weight": wv}, strict=True)
    add.to(DEV)
    np.random.seed(1)
    v0, i0 = plain.select(*args)
    np.random.seed(1)
    v1, i1 = add.select(*args)
    real = (v0 != 0).any(-1)                                   # the rows the tables name (a seeded bank row is never all zeros)
    # (the sum of an fp16-rounded row would be rounded twice: compare against the rows selected in fp32)
    np.random.seed(1)
    v32, _ = plain.select(args[0], args[1], args[2], args[3], torch.float32)
    want = ((v32 + wv.to(DEV)[None, :v0.shape[1]]) * real[..., None]).to(v0.dtype)
    assert torch.equal(i0, i1) and torch.equal(v1, want)
    for sel in (plain, add):
        for _ in range(warmup):
            sel.select(*args)
    t = {"plain": [], "add": []}
    for _ in range(10):                                        # alternating blocks
        for name, sel in (("plain", plain), ("add", add)):
            us, nbytes = launch_us(sel, args, calls)
            t[name].append(us)
            if name == "plain":
                plain_bytes = nbytes
    med = lambda xs: float(np.median(xs))      # noqa: E731
    extra_bytes = int(real.sum()) * C * 4
    rate = plain_bytes / (med(t["plain"]) * 1e-6)               # bytes/s the plain launch achieves
    print(json.dumps(dict(shape=shape, row_add=True, **extra, real_rows=int(real.sum()), launches_per_block=calls,
                          select_fwd_us=[round(x, 2) for x in t["plain"]], select_add_fwd_us=[round(x, 2) for x in t["add"]],
                          select_fwd_median_us=round(med(t["plain"]), 2), select_add_fwd_median_us=round(med(t["add"]), 2),
                          select_fwd_spread_us=round(max(t["plain"]) - min(t["plain"]), 2), select_fwd_bytes=plain_bytes,
                          extra_read_bytes=extra_bytes, select_fwd_GBps=round(rate / 1e9, 1),
                          extra_read_bound_us=round(extra_bytes / rate * 1e6, 2),
                          measured_difference_us=round(med(t["add"]) - med(t["plain"]), 2))), flush=True)


def measure(shape, bank, args, calls, warmup, extra):
    with tempfile.TemporaryDirectory() as tmp:
        plain, resident = selectors(bank, tmp)
    outs = []
    for sel in (plain, resident):
        np.random.seed(1)
        outs.append(sel.select(*args))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    base, res = timed(plain, args, calls, warmup), timed(resident, args, calls, warmup)
    med = lambda xs: float(np.median(xs))      # noqa: E731
    print(json.dumps(dict(shape=shape, **extra, vision=list(outs[0][0].shape), idx=list(outs[0][1].shape), draws=not resident.deterministic(args[0][0]),
                          dict_path_ms=[round(x, 3) for x in base], resident_ms=[round(x, 3) for x in res], dict_path_median_ms=round(med(base), 3),
                          resident_median_ms=round(med(res), 3), dict_path_spread_ms=round(max(base) - min(base), 3),
                          speedup=round(med(base) / med(res), 2), faster_by_more_than_spread=bool(med(base) - med(res) > max(base) - min(base)))),
          flush=True)
    if ROW_ADD:
        measure_row_add(shape, bank, args, calls, warmup, extra)


def online(calls, warmup):
    rng = np.random.default_rng(0)
    labels = list(range(1, 41))
    pm = caption(labels, rng)
    args = ([labels] * 8, [pm] * 8, T, DEV, torch.float16)
    measure("online", make_bank(40, 100, 1), args, calls, warmup, dict(labels=40, rows_per_label=100, k=K, items=8, T=T, C=C))


def lvis(calls, warmup):
    rng = np.random.default_rng(1)
    chunks = [list(range(1 + 40 * c, 41 + 40 * c)) for c in range(31)]
    maps = [caption(labs, rng) for labs in chunks]
    args = ([l for l in chunks for _ in range(2)], [m for m in maps for _ in range(2)], T, DEV, torch.float16)      # chunk-major, as forward_chunks
    measure("lvis", make_bank(31 * 40, 5, 2), args, calls, warmup, dict(labels=31 * 40, rows_per_label=5, k=K, items=62, T=T, C=C))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="both", choices=("online", "lvis", "both"))
    ap.add_argument("--row-add", action="store_true", help="time the launch alone: mq_bank_select_fwd against mq_bank_select_add_fwd")
    a = ap.parse_args()
    global ROW_ADD
    ROW_ADD = a.row_add
    if a.shape in ("online", "both"):
        online(a.calls, a.warmup)
    if a.shape in ("lvis", "both"):
        lvis(a.calls, a.warmup)


if __name__ == "__main__":
    main()
