#!/usr/bin/env python3
"""Images / s of `mq_det_amd.grounding.evaluate_grounding` on the MI355X: MQ-GLIP-T (bench.py's synthetic-weight model, 5-shot vision queries)
at 800 x 1333, `--items` (image, sentence) items with different synthetic captions of about 20 tokens and 4 to 6 phrases each, once at
B = `--batch` through `forward_grounding` and once as the reference runs it: B = 1 through `model(...)` (the forward this package had before
`forward_grounding`).  Both loops feed a FlickrRecallEvaluator through `update_boxlist` and end in `summarize()`; the first pass of each
(graph warm-up and capture) is not timed.  One JSON line at the end.

    python tools/grounding_bench.py [--items 32] [--batch 8] [--passes 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class PerItem:
    """the model without `forward_grounding`: evaluate_grounding then takes one `model(...)` call per item"""

    def __init__(self, model):
        self.model, self.cfg = model, model.cfg

    def __call__(self, *a, **k):
        return self.model(*a, **k)


def measure(args):
    if not torch.cuda.is_available():
        raise SystemExit("grounding_bench needs a GPU: a time taken elsewhere says nothing")
    import bench
    from mq_det_amd.evaluation import FlickrRecallEvaluator
    from mq_det_amd.grounding import evaluate_grounding
    from mq_det_amd.structures import BoxList, ImageList
    from mq_det_amd.utils.tokenizer import positive_map_from_spans, synthetic_caption
    dev = torch.device("cuda:0")
    cfg, model, _ = bench.build_model(dev, n_classes=6, n_categories=6)
    tk = model.tokenizer
    T = cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN
    g = torch.Generator().manual_seed(0)
    H, W = 800, 1333
    targets, gt, boxes, tokens = [], {}, {}, []
    for n in range(args.items):
        n_ph = 4 + n % 3
        caption, spans = synthetic_caption(n_ph, start=11 * n, sep=" and ", words=(2, 3, 3, 2, 3, 2))
        pm = positive_map_from_spans(tk, caption, spans, list(range(n_ph)))
        tokens.append(max(max(v) for v in pm.values()) + 2)
        pme = torch.zeros(n_ph, T)
        for k, v in pm.items():
            pme[k, v] = 1
        t = BoxList(torch.zeros(0, 4), (W, H), mode="xyxy")
        img = str(1000 + n // 5)
        for name, v in (("caption", caption), ("positive_map_eval", pme), ("original_img_id", img), ("sentence_id", n % 5),
                        ("orig_size", torch.tensor([500, 375]))):
            t.add_field(name, v)
        targets.append(t)
        gt.setdefault(img, []).append([{"phrase_id": str(100 * n + p), "phrase_type": ["other"]} for p in range(n_ph)])
        boxes.setdefault(img, {}).update({str(100 * n + p): [[10 + p, 20, 200 + p, 300]] for p in range(n_ph)})
    pixels = [torch.randn(args.batch, 3, H, W, generator=g).to(dev) for _ in range(2)]

    def loader(B):
        for b0 in range(0, args.items, B):
            ts = targets[b0:b0 + B]
            off = b0 % args.batch                            # item n has the same pixels at every batch size
            yield ImageList(pixels[(b0 // args.batch) % 2][off:off + len(ts)], [(H, W)] * len(ts)), ts, list(range(b0, b0 + len(ts)))

    def run(m, B):
        times = []
        for p in range(args.passes + 1):
            ev = FlickrRecallEvaluator(gt, boxes, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            score = evaluate_grounding(m, loader(B), ev, device=dev)
            torch.cuda.synchronize()
            if p:
                times.append(time.perf_counter() - t0)
        return args.items / min(times), args.items / max(times), score
    fast, fast_lo, score_b = run(model, args.batch)
    model.clear_caches()
    base, base_lo, score_1 = run(PerItem(model), 1)
    return {"items": args.items, "batch": args.batch, "canvas": [H, W], "caption_tokens_min_max": [min(tokens), max(tokens)],
            "phrases_per_item": [4, 5, 6], "forward_grounding_images_per_s": round(fast, 1), "forward_grounding_images_per_s_slowest_pass": round(fast_lo, 1),
            "per_item_forward_images_per_s": round(base, 1), "per_item_forward_images_per_s_slowest_pass": round(base_lo, 1),
            "speedup": round(fast / base, 2), "cache_stats": dict(model.cache_stats),
            "recall_at_1_all": [score_b["Recall@1_all"], score_1["Recall@1_all"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    print(json.dumps(measure(ap.parse_args())))


if __name__ == "__main__":
    main()
