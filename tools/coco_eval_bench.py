#!/usr/bin/env python3
"""Time CocoAPEvaluator.summarize() on the MI355X at a COCO val2017-like shape: 5 000 images, 80 categories, about 7 ground truths per
image, 100 detections per image (mq_det_amd.utils.synth.synthetic_coco, seeded).  Reported: update() of all images, summarize() (grouping
sorts + csrc/ap_eval.hip + the twelve means, ending in its one host sync) as the median and spread of `--runs` calls after one warm-up
call, the two kernels' share from the HIP events of ops.start_timing(), and -- for scale -- the numpy restatement tests/coco_eval_ref.py
on a tenth of the images (it is the test oracle, not a tuned evaluator).  One JSON line at the end.

    python tools/coco_eval_bench.py [--images 5000] [--runs 5] [--no-restatement]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(args):
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_bench needs a GPU: a time taken elsewhere says nothing")
    from mq_det_amd import ops
    from mq_det_amd.evaluation import CocoAPEvaluator
    from mq_det_amd.structures import BoxList
    from mq_det_amd.utils.synth import synthetic_coco
    dev = torch.device("cuda:0")
    gt, items = synthetic_coco(n_img=args.images, n_cat=args.categories)
    preds = []
    for i, size, boxes, scores, labels in items:
        bl = BoxList(torch.from_numpy(boxes).to(dev), size, "xyxy")
        bl.add_field("scores", torch.from_numpy(scores).to(dev))
        bl.add_field("labels", torch.from_numpy(labels).to(dev))
        preds.append((i, bl))
    ev = CocoAPEvaluator(gt, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.update(preds)
    ev.synchronize_between_processes()
    torch.cuda.synchronize()
    t_update = time.perf_counter() - t0
    strings = ev.summarize()                                # warm-up: code objects, the sorts' workspaces
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.summarize()                                      # ends in its host sync
        times.append((time.perf_counter() - t0) * 1e3)
    ops.start_timing()
    ev.summarize()
    kern = {k: round(v[1], 3) for k, v in ops.stop_timing().items()}
    out = {"images": args.images, "categories": args.categories, "ground_truths": len(gt["annotations"]), "detections": len(ev.acc.rows),
           "pairs": len(ev.eval["pair_key"]), "update_ms": round(t_update * 1e3, 1), "summarize_ms_median": round(statistics.median(times), 2),
           "summarize_ms_min": round(min(times), 2), "summarize_ms_max": round(max(times), 2), "kernel_ms": kern, "AP": ev.stats[0]}
    if not args.no_restatement:
        import coco_eval_ref as ref
        n = max(args.images // 10, 1)
        keep = {it[0] for it in items[:n]}
        sub = dict(gt, images=[im for im in gt["images"] if im["id"] in keep], annotations=[a for a in gt["annotations"] if a["image_id"] in keep])
        t0 = time.perf_counter()
        want = ref.evaluate(sub, ref.result_rows(items[:n], sub))
        out["restatement_images"], out["restatement_s"] = n, round(time.perf_counter() - t0, 2)
        es = CocoAPEvaluator(sub, device=dev)
        es.update(preds[:n])
        es.summarize()
        out["restatement_equal"] = bool(np.array_equal(es.eval["precision"].cpu().numpy(), want["precision"]))
    return strings, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--categories", type=int, default=80)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    with contextlib.redirect_stdout(io.StringIO()):          # summarize() prints its lines on every call; once is enough
        strings, out = measure(args)
    for s in strings:
        print(s)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
