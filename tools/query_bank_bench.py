#!/usr/bin/env python3
"""Time `QueryBank.update` (one mq_bank_admit launch per call) against the Python loop of `pool_into_bank` on a dict, on the same device tensors.

  online : one image's worth of 512 kept detections over 40 labels, capacity 100, exclusion on, bank half full (50 rows per label)
  build  : 2000 batches of 64 boxes over 365 labels, capacity 5000, no exclusion, from an empty bank

Each measurement is taken after one excluded warm-up run, `--repeats` times (default 3), with device events around the timed region and wall time
around the same region plus a final synchronise.  One JSON line per shape: every repeat of both paths, their medians, the baseline's
run-to-run spread (max - min over the repeats) and the ratio of the medians.

    python tools/query_bank_bench.py [--repeats 3] [--shape online|build|both]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.modeling.detector import pool_into_bank  # noqa: E402
from mq_det_amd.query_bank import QueryBank  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

DEV = torch.device("cuda:0")
C = 256


def candidates(seed, n, n_labels, centres=8):
    """cluster centres plus small / large noise: both branches of the similarity test are taken"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_labels, n)
    cen = rng.standard_normal((n_labels, centres, C))
    cen /= np.linalg.norm(cen, axis=-1, keepdims=True)
    sigma = np.where(rng.random(n) < 0.6, 0.18, 1.3) / np.sqrt(C)
    x = (cen[labels, rng.integers(0, centres, n)] + rng.standard_normal((n, C)) * sigma[:, None]) * rng.uniform(0.5, 4.0, n)[:, None]
    return torch.from_numpy(x.astype(np.float32)[:, None]).to(DEV), torch.from_numpy(labels.astype(np.int64)).to(DEV)


def admit(bank, feats, labels, exclude, maxq, cfg):
    """one `pool_into_bank` call on prepared rows: the dict loop, or the device path when `bank` is a QueryBank"""
    t = BoxList(torch.zeros(len(labels), 4, device=DEV), (10, 10))
    t.add_field("labels", labels)
    return pool_into_bank(cfg, lambda vf, targets, reduce_mean: feats[:, 0], [None], [t], bank, exclude, maxq)


def timed(setup, run, repeats):
    """-> [(device ms, wall ms)] of `repeats` runs of run(setup()) after one warm-up"""
    out = []
    for r in range(repeats + 1):
        state = setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        run(state)
        b.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if r:
            out.append((a.elapsed_time(b), wall))
    return out


def report(shape, base, dev, extra):
    med = lambda xs: float(np.median(xs))      # noqa: E731
    bw, dw = [w for _, w in base], [w for _, w in dev]
    line = dict(shape=shape, **extra, dict_loop_ms=[round(w, 3) for w in bw], dict_loop_device_ms=[round(d, 3) for d, _ in base],
                query_bank_ms=[round(w, 3) for w in dw], query_bank_device_ms=[round(d, 3) for d, _ in dev],
                dict_loop_median_ms=round(med(bw), 3), query_bank_median_ms=round(med(dw), 3), dict_loop_spread_ms=round(max(bw) - min(bw), 3),
                speedup=round(med(bw) / med(dw), 2), faster_by_more_than_spread=bool(med(bw) - med(dw) > max(bw) - min(bw)))
    print(json.dumps(line), flush=True)


def online(repeats, cfg):
    pre_f, pre_l = candidates(1, 40 * 50, 40)
    pre_l = torch.arange(40, device=DEV).repeat_interleave(50)               # exactly 50 rows per label
    prefill = admit({}, pre_f, pre_l, False, 100, cfg)
    feats, labels = candidates(2, 512, 40)
    results = []

    def run(bank):
        results.append(admit(bank, feats, labels, True, 100, cfg))
    base = timed(lambda: {k: v.clone() for k, v in prefill.items()}, run, repeats)
    plain = results[-1]
    dev = timed(lambda: QueryBank.from_dict(prefill, DEV), run, repeats)
    got = results[-1].to_dict()
    assert sorted(got) == sorted(plain) and all(torch.equal(got[k], plain[k]) for k in plain)
    report("online", base, dev, dict(candidates=512, labels=40, capacity=100, exclude_similar=True, rows_before=2000,
                                     rows_after=sum(len(v) for v in plain.values())))


def build(repeats, cfg, batches=2000, per=64):
    feats, labels = candidates(3, batches * per, 365)
    results = []

    def run(bank):
        for lo in range(0, batches * per, per):
            bank = admit(bank, feats[lo:lo + per], labels[lo:lo + per], False, 5000, cfg)
        results.append(bank)
    base = timed(dict, run, repeats)
    plain = results[-1]
    dev = timed(lambda: QueryBank(DEV), run, repeats)
    got = results[-1].to_dict()
    assert sorted(got) == sorted(plain) and all(torch.equal(got[k], plain[k]) for k in plain)
    report("build", base, dev, dict(batches=batches, boxes_per_batch=per, labels=365, capacity=5000, exclude_similar=False,
                                    rows_after=sum(len(v) for v in plain.values())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shape", default="both", choices=("online", "build", "both"))
    args = ap.parse_args()
    cfg = get_cfg()
    if args.shape in ("online", "both"):
        online(args.repeats, cfg)
    if args.shape in ("build", "both"):
        build(args.repeats, cfg)


if __name__ == "__main__":
    main()
