#!/usr/bin/env python3
"""Time LVIS Fixed AP (mq_det_amd.evaluation.LvisFixedAPEvaluator) at the LVIS-minival shape on the device: 4 809 images, 1 203 categories
(LVIS's r / c / f split), 50 000 ground truths, topk 10 000 detections per category (12M accumulator rows; mq_det_amd.utils.synth.synthetic_lvis).

Reported separately (median of --reps runs after one warm-up, each on a fresh evaluator):
  ingest      the constructor: ground-truth json dict -> device tensors;
  match       mq_lvis_match (device events);
  accumulate  mq_lvis_accumulate (device events);
  total       summarize() wall time, ending in its one host sync (grouping sorts + both kernels + summary means).

    python tools/lvis_eval_bench.py [--reps 5]                        (needs an MI355X)
    python tools/lvis_eval_bench.py --reference-cpu 480 120 1000     (the reference's _summarize_fixed on the CPU, pure Python, at
                                                                      images / categories / detections per category; needs the reference checkout)
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

from mq_det_amd.utils.synth import synthetic_lvis  # noqa: E402


def device_bench(reps):
    from mq_det_amd import ops
    from mq_det_amd.evaluation import LvisFixedAPEvaluator
    dev = torch.device("cuda:0")
    gt, rows = synthetic_lvis()
    t_rows = [torch.from_numpy(rows[:, i]) for i in range(3)] + [torch.from_numpy(rows[:, 3:])]
    rec = {"ingest_s": [], "match_ms": [], "accumulate_ms": [], "total_s": []}
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.time()
        ev = LvisFixedAPEvaluator(gt, topk=10000, device=dev)
        torch.cuda.synchronize()
        t_ingest = time.time() - t0
        ev.acc.update(*t_rows)
        ev.synchronize_between_processes()
        torch.cuda.synchronize()
        ops.start_timing()
        t0 = time.time()
        ev.summarize()
        t_total = time.time() - t0
        k = ops.stop_timing()
        if r == 0:
            continue                               # warm-up: first launches, allocator
        rec["ingest_s"].append(t_ingest)
        rec["total_s"].append(t_total)
        rec["match_ms"].append(k["lvis_match"][1])
        rec["accumulate_ms"].append(k["lvis_accumulate"][1])
    e = ev.eval
    out = {k: float(np.median(v)) for k, v in rec.items()}
    out.update({"reps": reps, "rows": int(len(ev.acc.rows)), "pairs": int(len(e["pair_key"])),
                "detections_evaluated": int(e["pair_dt"][:, 1].sum()), "ground_truths": int(len(ev.gt_box)), "AP": ev.results["AP"]})
    return out


def reference_cpu(n_img, n_cat, det_per_cat):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_golden_lvis_eval import load_lvis_eval
    import contextlib
    import io
    lvis, le = load_lvis_eval()
    n_gt = round(50000 * n_img / 4809)
    gt, rows = synthetic_lvis(n_img=n_img, n_cat=n_cat, n_gt=n_gt, det_per_cat=det_per_cat)
    L = lvis.LVIS()
    L.dataset = gt
    with contextlib.redirect_stdout(io.StringIO()):
        L._create_index()
    ev = le.LvisEvaluatorFixedAP(L, topk=10000)
    ev.by_cat = {}
    for r in rows.tolist():                        # the accumulator's by_cat() view (rows are already per-category score order)
        ev.by_cat.setdefault(int(r[1]), []).append({"image_id": int(r[0]), "category_id": int(r[1]), "bbox": r[3:7], "score": r[2]})
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        ev._summarize_fixed()
    return {"reference_cpu_s": time.time() - t0, "images": n_img, "categories": n_cat, "ground_truths": n_gt, "rows": int(len(rows))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference-cpu", type=int, nargs=3, metavar=("IMAGES", "CATEGORIES", "DETS_PER_CAT"))
    a = ap.parse_args()
    res = reference_cpu(*a.reference_cpu) if a.reference_cpu else device_bench(a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
