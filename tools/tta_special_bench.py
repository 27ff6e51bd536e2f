#!/usr/bin/env python3
"""Time the device TTA merge per TEST.SPECIAL_NMS mode against the restated CPU reference on the same rows.

B = 8 images, the default 24 transforms x (100 + 16) rows, 80 classes, TEST.TH and TEST.PRE_NMS_TOP_N at their defaults.  Per mode:
  device_ms   tta.merge end to end (packing on the host, the launches, the one read-back of the counts), device idle before and after
  kernels_ms  ops.tta_merge alone between two device events
  cpu_ms      tests/tta_special_ref.py merge_special over the B images (numpy on this host; 'none': tests/test_tta_cpu.py merge_restated)
Medians of --repeat runs after one warm-up.  One JSON line.

    python tools/tta_special_bench.py [--repeat 5] [--batch 8]
"""
import argparse
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


def make_dets(B, T, K, n_cls, wh, seed=3):
    """Seeded rows: objects in the original frame seen by every transform with jitter (so classes hold real clusters), distinct scores."""
    g = np.random.default_rng(seed)
    pool = g.permutation(np.arange(1, T * B * K + 1)).astype(np.float32) / np.float32(T * B * K + 1)     # distinct, spread over (0, 1)
    objs = []
    for (w, h) in wh:
        n = 60
        x1, y1 = g.uniform(0, 0.7 * w, n), g.uniform(0, 0.7 * h, n)
        objs.append((np.stack([x1, y1, x1 + g.uniform(8, 0.3 * w, n), y1 + g.uniform(8, 0.3 * h, n)], 1), g.integers(1, n_cls + 1, n)))
    dets = []
    for t in range(T):
        s = 0.5 + 0.25 * (t // 2)
        packed = np.zeros((B, K, 6), np.float32)
        whs = []
        for b, (w, h) in enumerate(wh):
            ws, hs = int(w * s), int(h * s)
            pick = g.integers(0, len(objs[b][0]), K)
            bx = (objs[b][0][pick] + g.normal(0, 2.0, (K, 4))) * s
            lab = np.where(g.random(K) < 0.8, objs[b][1][pick], g.integers(1, n_cls + 1, K))
            if t % 2:
                bx = np.stack([ws - bx[:, 2] - 1, bx[:, 1], ws - bx[:, 0] - 1, bx[:, 3]], 1)
            sc = pool[(t * B + b) * K:(t * B + b + 1) * K]
            o = np.argsort(-sc, kind="stable")
            packed[b] = np.concatenate([bx[o], sc[o, None], lab[o, None]], 1)
            whs.append((ws, hs))
        dets.append((torch.from_numpy(packed), [K] * B, whs, t % 2 == 1, (0, 10000)))
    return dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    import tta_special_cases as sc
    import tta_special_ref as ref
    import test_tta_cpu as tc
    from mq_det_amd import get_cfg, ops, tta
    dev = torch.device("cuda:0")
    cfg = get_cfg()
    T, K, n_cls = 2 * len(cfg.TEST.SCALES), cfg.MODEL.ATSS.DETECTIONS_PER_IMG + 16, cfg.TEST.NUM_CLASSES - 1
    wh = [(640, 480), (480, 640), (500, 375), (640, 427), (427, 640), (640, 480), (375, 500), (500, 333)][:args.batch]
    dets = make_dets(len(wh), T, K, n_cls, wh)
    dets_d = sc.to_device(dets, dev)
    rows = sc.prep_restated(dets, wh)
    out = {"B": len(wh), "T": T, "K": K, "classes": n_cls, "TH": cfg.TEST.TH, "PRE_NMS_TOP_N": cfg.TEST.PRE_NMS_TOP_N, "repeat": args.repeat, "modes": {}}
    spans = []
    real = ops.tta_merge

    def timed(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **k)
        e1.record()
        spans.append((e0, e1))
        return r
    ops.tta_merge = timed
    for mode in ("none",) + ref.MODES:
        cfg.TEST.SPECIAL_NMS = mode
        wall, kern, cpu, n_dev = [], [], [], None
        for it in range(args.repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tta.merge(dets_d, wh, cfg, dev)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(spans[-1][0].elapsed_time(spans[-1][1]))
            n_dev = [len(r) for r in res]
        for it in range(args.repeat):
            t0 = time.perf_counter()
            if mode == "none":
                want = [len(r[1]) for r in tc.merge_restated(dets, wh, cfg)]
            else:
                want = [len(ref.merge_special(bx, s, lb, tta.class_list(cfg), mode, cfg.TEST.TH, cfg.MODEL.RETINANET.INFERENCE_TH,
                                              cfg.TEST.PRE_NMS_TOP_N)["scores"]) for bx, s, lb in rows]
            cpu.append((time.perf_counter() - t0) * 1e3)
        out["modes"][mode] = {"device_ms": round(statistics.median(wall[1:]), 3), "kernels_ms": round(statistics.median(kern[1:]), 3),
                              "cpu_ms": round(statistics.median(cpu), 1), "rows_out": n_dev, "rows_out_cpu": want}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
