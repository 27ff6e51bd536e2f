#!/usr/bin/env python3
"""Images / s of `mq_det_amd.detection.evaluate_detection` on the MI355X: MQ-GLIP-T (bench.py's synthetic-weight model, 5-shot vision
queries) at 800 x 1333 with the LVIS protocol's 31 chunk captions (1203 synthetic categories), `--images` new synthetic images per pass at
B = 1 and B = 4, once with `packed=True` (forward_chunks_packed -> update_packed: the rows are built by csrc/eval_rows.hip and the host
waits for nothing per image) and once with `packed=False` (forward_chunks -> BoxLists -> update: the code as it was, the baseline).  The
two run in the same process, alternating, `--passes` timed passes each after one untimed pass (graph capture); the medians are reported.
Every pass feeds a fresh LvisFixedAPEvaluator and ends in `summarize()`.  The host syncs are counted in one more pass of each kind under
torch's sync debug mode "warn": those inside the loop over the batches, per image, and those after it (fold, summarize(), overflow flag).
One JSON line at the end.

    python tools/detection_eval_bench.py [--images 8] [--passes 5] [--batches 1,4]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    if not torch.cuda.is_available():
        raise SystemExit("detection_eval_bench needs a GPU: a time taken elsewhere says nothing")
    import bench
    from mq_det_amd.detection import evaluate_detection
    from mq_det_amd.evaluation import LvisFixedAPEvaluator
    from mq_det_amd.structures import ImageList
    dev = torch.device("cuda:0")
    n_cat = 1203
    cfg, model, chunks = bench.build_model(dev, caches=True, n_categories=n_cat)
    queries_and_maps = ([c for c, _ in chunks], [pm for _, pm in chunks])
    H, W = bench.IMG_HW
    Hp, Wp = -(-H // 32) * 32, -(-W // 32) * 32
    g = torch.Generator().manual_seed(0)
    pixels = torch.zeros(4, 3, Hp, Wp)
    pixels[:, :, :H, :W] = torch.randn(4, 3, H, W, generator=g)
    pixels = pixels.to(dev)
    ids = list(range(1, args.images + 1))
    gt = {"images": [{"id": i, "neg_category_ids": [], "not_exhaustive_category_ids": []} for i in ids],
          "categories": [{"id": c, "frequency": "rcf"[c % 3]} for c in range(1, n_cat + 1)],
          "annotations": [{"id": n + 1, "image_id": i, "category_id": 1 + (37 * n) % n_cat, "bbox": [10.0 + n, 20.0, 100.0, 80.0], "area": 8000.0}
                          for n, i in enumerate(ids)]}

    def loader(B):
        for b0 in range(0, args.images, B):
            batch = ids[b0:b0 + B]
            # new pixels every batch (the clone is the "data loader", as in bench.py's lvis workload)
            yield (ImageList(pixels[:len(batch)].clone(), [(H, W)] * len(batch)),
                   [{"image_id": torch.tensor(i), "orig_size": torch.tensor([480, 640])} for i in batch], batch)

    def one_pass(B, packed, at_loop_end=None):
        ev = LvisFixedAPEvaluator(gt, device=dev)
        if at_loop_end is not None:                            # (the first call after the loop: the syncs counted so far are the loop's)
            gather = ev.synchronize_between_processes
            ev.synchronize_between_processes = lambda: (at_loop_end(), gather())[1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = evaluate_detection(model, loader(B), ev, queries_and_maps, device=dev, packed=packed)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, score, len(ev.acc.rows)

    def syncs(B, packed):
        """-> (host syncs inside the loop over the batches, host syncs after it: the fold, summarize(), the overflow flag)"""
        torch.cuda.set_sync_debug_mode("warn")
        in_loop = []
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                count = lambda: sum("synchroniz" in str(w.message) for w in caught)      # noqa: E731
                one_pass(B, packed, lambda: in_loop.append(count()))
                total = count()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return in_loop[0], total - in_loop[0]

    out = {"images_per_pass": args.images, "chunks": len(chunks), "canvas": [H, W], "passes": args.passes, "batches": {}}
    for B in args.batches:
        times = {True: [], False: []}
        scores, rows = {}, {}
        for p in range(args.passes + 1):
            for packed in ((True, False) if p % 2 == 0 else (False, True)):         # alternating, the order swapped every pass
                t, scores[packed], rows[packed] = one_pass(B, packed)
                if p:
                    times[packed].append(t)
        if scores[True] != scores[False] or rows[True] != rows[False]:
            raise SystemExit(f"B = {B}: the two paths disagree ({rows[True]} / {rows[False]} rows)")
        n_sync = {packed: syncs(B, packed) for packed in (True, False)}
        med = {k: statistics.median(v) for k, v in times.items()}
        out["batches"][str(B)] = {
            "packed_images_per_s": round(args.images / med[True], 2), "boxlist_images_per_s": round(args.images / med[False], 2),
            "packed_images_per_s_min_max": [round(args.images / max(times[True]), 2), round(args.images / min(times[True]), 2)],
            "boxlist_images_per_s_min_max": [round(args.images / max(times[False]), 2), round(args.images / min(times[False]), 2)],
            "ratio": round(med[False] / med[True], 3), "rows_kept": rows[True],
            "host_syncs_per_image_in_the_loop": {"packed": round(n_sync[True][0] / args.images, 2), "boxlist": round(n_sync[False][0] / args.images, 2)},
            "host_syncs_after_the_loop": {"packed": n_sync[True][1], "boxlist": n_sync[False][1]}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1, 4])
    print(json.dumps(measure(ap.parse_args())))


if __name__ == "__main__":
    main()
