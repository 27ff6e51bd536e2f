#!/usr/bin/env python3
"""Time FlickrRecallEvaluator on the MI355X at the Flickr30k Entities test shape: 1 000 images x 5 sentences, about 3 phrases per sentence,
up to 300 detections per sentence (mq_det_amd.utils.synth.synthetic_flickr, seeded; the exact counts are printed).  Reported:
`update_boxlist` over all sentences (resize + flickr_post_process as device rows, no host sync), `summarize()` (grouping sorts +
csrc/flickr_eval.hip, ending in its one host sync) as the median and spread of `--runs` calls after one warm-up call, the two kernels' share
from the HIP events of ops.start_timing(), and the numpy restatement tests/flickr_eval_ref.py (post-process + evaluate) on the host over
the same data -- it must give the same score dict.  One JSON line at the end.

    python tools/flickr_eval_bench.py [--images 1000] [--runs 5] [--no-restatement]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(args):
    if not torch.cuda.is_available():
        raise SystemExit("flickr_eval_bench needs a GPU: a time taken elsewhere says nothing")
    from mq_det_amd import ops
    from mq_det_amd.evaluation import FlickrRecallEvaluator
    from mq_det_amd.structures import BoxList
    from mq_det_amd.utils.synth import synthetic_flickr
    dev = torch.device("cuda:0")
    plus = 1
    gt, boxes, preds = synthetic_flickr(n_img=args.images, sent_per_img=args.sentences, det_per_sent=args.detections)
    lists = []
    for img, sid, size, orig, n_ph, b, sc, ph in preds:
        bl = BoxList(torch.from_numpy(b).to(dev), size, "xyxy")
        bl.add_field("scores", torch.from_numpy(sc).to(dev))
        bl.add_field("labels", torch.from_numpy(ph + plus).to(dev))
        lists.append(bl)
    ev = FlickrRecallEvaluator(gt, boxes, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for (img, sid, size, orig, n_ph, *_), bl in zip(preds, lists):
        ev.update_boxlist(img, sid, bl, n_ph, plus, orig)
    ev.synchronize_between_processes()
    torch.cuda.synchronize()
    t_update = time.perf_counter() - t0
    score = ev.summarize()                                  # warm-up: code objects, the sorts' workspaces
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.summarize()                                      # ends in its host sync
        times.append((time.perf_counter() - t0) * 1e3)
    ops.start_timing()
    ev.summarize()
    kern = {k: round(v[1], 3) for k, v in ops.stop_timing().items()}
    out = {"images": args.images, "sentences": len(preds), "phrases": ev.P, "ground_truth_boxes": len(ev.gt_box), "detections": len(ev.eval["dt_box"]),
           "update_ms": round(t_update * 1e3, 1), "summarize_ms_median": round(statistics.median(times), 2), "summarize_ms_min": round(min(times), 2),
           "summarize_ms_max": round(max(times), 2), "kernel_ms": kern, "Recall@1_all": score["Recall@1_all"],
           "Upper_bound_all": score["Upper_bound_all"]}
    if not args.no_restatement:
        import flickr_eval_ref as ref
        t0 = time.perf_counter()
        post = [ref.post_process(img, sid, b, sc, ph + plus, size, orig, n_ph, plus) for img, sid, size, orig, n_ph, b, sc, ph in preds]
        t1 = time.perf_counter()
        want = ref.evaluate(gt, boxes, post)
        t2 = time.perf_counter()
        out["restatement_post_process_s"], out["restatement_evaluate_s"] = round(t1 - t0, 2), round(t2 - t1, 2)
        out["restatement_equal"] = list(want.items()) == list(score.items())
    return score, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--sentences", type=int, default=5)
    ap.add_argument("--detections", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    score, out = measure(args)
    print({k: round(v, 4) for k, v in score.items() if k.endswith("_all")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
