#!/usr/bin/env python3
"""Write tests/golden/lvis_eval_{small,medium}.npz + .json: what the reference's LVIS Fixed AP path returns, executed in place.

maskrcnn_benchmark/data/datasets/evaluation/lvis/lvis.py and lvis_eval.py run from where they lie (oracle/_refload.py shells), with:
  * pycocotools.mask stubbed: `iou` restated as pycocotools' bbIou with iscrowd = 0 (maskApi.c; pycocotools is not installed here), in
    double, returning [] when either side is empty as _mask.pyx does -- the only function the bbox path calls;
  * torchvision stubbed (lvis.py imports it, the evaluation does not use it);
  * maskrcnn_benchmark.utils.mdetr_dist stubbed to one process (all_gather(x) = [x], main process).
LvisEvaluatorFixedAP.update is fed mdetr-style predictions (image_id, {"scores", "labels", "boxes" xyxy fp32}); _summarize_fixed runs the
reference's LVISResults / LVISEval.  Stored: the ground truth and the predictions, topk, per (image, category, area) dt_matches != 0 /
dt_ignore / gt_ignore, precision, recall, results and the printed strings.

    python tools/gen_golden_lvis_eval.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "lvis_eval_")


def iou_restated(dt, gt, iscrowd):
    """pycocotools.mask.iou for two lists of xywh boxes: bbIou (maskApi.c) with iscrowd = 0, [len(dt), len(gt)] double."""
    if len(dt) == 0 or len(gt) == 0:
        return []
    assert not any(iscrowd)
    out = np.zeros((len(dt), len(gt)))
    for j, G in enumerate(gt):
        ga = G[2] * G[3]
        for i, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i_ = w * h
            out[i, j] = i_ / (da + ga - i_)
    return out


def load_lvis_eval():
    from oracle import _refload
    pc = types.ModuleType("pycocotools")
    pc.__path__ = []
    mask = types.ModuleType("pycocotools.mask")
    mask.iou = iou_restated
    pc.mask = mask
    dist = types.ModuleType("maskrcnn_benchmark.utils.mdetr_dist")
    dist.all_gather = lambda x: [x]
    dist.is_main_process = lambda: True
    dist.get_world_size = lambda: 1
    sys.modules.update({"pycocotools": pc, "pycocotools.mask": mask, "torchvision": types.ModuleType("torchvision"),
                        "maskrcnn_benchmark.utils.mdetr_dist": dist})
    R = _refload.REF + "/maskrcnn_benchmark"
    _refload._shell("maskrcnn_benchmark", R)
    _refload._shell("maskrcnn_benchmark.utils", R + "/utils")
    sys.modules["maskrcnn_benchmark.utils"].mdetr_dist = dist
    for sub in ("data", "data/datasets", "data/datasets/evaluation", "data/datasets/evaluation/lvis"):
        _refload._shell("maskrcnn_benchmark." + sub.replace("/", "."), R + "/" + sub)
    lvis = importlib.import_module("maskrcnn_benchmark.data.datasets.evaluation.lvis.lvis")
    le = importlib.import_module("maskrcnn_benchmark.data.datasets.evaluation.lvis.lvis_eval")
    return lvis, le


def small_case():
    """Hand-made: every rule of LvisEvaluatorFixedAP._summarize_fixed (see tests/test_lvis_eval_cpu.py)."""
    cats = [(1, "r"), (2, "c"), (3, "f"), (5, "r"), (7, "c"), (9, "f"), (11, "f"), (13, "c")]
    images = [{"id": 10, "neg_category_ids": [2, 5], "not_exhaustive_category_ids": [3]},
              {"id": 20, "neg_category_ids": [1], "not_exhaustive_category_ids": []},
              {"id": 30, "neg_category_ids": [9, 13], "not_exhaustive_category_ids": [1, 9]},
              {"id": 40, "neg_category_ids": [], "not_exhaustive_category_ids": [7]},
              {"id": 50, "neg_category_ids": [3], "not_exhaustive_category_ids": []}]          # no detections
    A = []

    def ann(i, c, box, area=None, **kw):
        A.append(dict({"id": len(A) + 1, "image_id": i, "category_id": c, "bbox": box,
                       "area": box[2] * box[3] if area is None else area}, **kw))
    ann(10, 1, [0, 0, 10, 10])                    # IoU 0.5 / 0.75 exactly with the detections below
    ann(10, 1, [20, 20, 40, 40])
    ann(10, 1, [100, 100, 120, 90])
    ann(10, 1, [0, 0, 10, 10], ignore=1)          # ignored duplicate
    ann(10, 3, [5, 5, 50, 50])
    ann(10, 3, [5, 5, 30, 30], area=0)            # zero area: dropped
    ann(20, 1, [10, 10, 31, 33])                  # area 1023: small / medium boundary
    ann(20, 1, [50, 50, 32, 32])                  # area 1024 exactly
    ann(20, 7, [0, 0, 200, 200], ignore=1)        # only an ignored gt: category 7 stays -1 where nothing else counts
    ann(20, 9, [1, 2, 3, 4])
    ann(30, 3, [30, 30, 100, 96])
    ann(30, 3, [35, 28, 100, 96])
    ann(30, 3, [300, 300, 9, 9])
    ann(30, 3, [0, 0, 1, 1])
    ann(40, 11, [10, 10, 20, 20])                 # category with ground truths and no detections
    ann(40, 1, [60, 60, 80, 80])
    ann(40, 1, [61, 61, 79, 79])
    ann(40, 1, [62, 60, 80, 80])
    ann(40, 2, [5, 5, 5, 5], ignore=1)
    ann(50, 3, [0, 0, 50, 50])
    ann(99, 1, [0, 0, 10, 10])                    # image not in the file
    ann(10, 4, [0, 0, 10, 10])                    # category not in the file
    A[2]["id"] = 0                                # a ground-truth id of 0
    gt = {"images": images, "annotations": A, "categories": [{"id": c, "name": f"c{c}", "frequency": f} for c, f in cats]}
    P = []

    def det(i, c, box, s):
        P.append((i, c, s, box[0], box[1], box[0] + box[2], box[1] + box[3]))
    det(10, 1, [0, 0, 5, 10], 0.9)                # IoU 0.5 with gt 1
    det(10, 1, [0, 0, 7.5, 10], 0.9)              # IoU 0.75, tied score
    det(10, 1, [20, 20, 40, 40], 0.8)
    det(10, 1, [20, 22, 40, 40], 0.8)
    det(10, 1, [101, 99, 118, 92], 0.7)           # matches the id-0 gt
    det(10, 1, [0, 0, 10, 10], 0.6)               # matches the ignored gt
    det(10, 1, [500, 500, 5, 5], 0.5)
    det(10, 2, [0, 0, 10, 10], 0.5)               # negative category, no gt
    det(10, 3, [5, 5, 50, 50], 0.4)
    det(10, 3, [200, 200, 50, 50], 0.4)           # not exhaustive: unmatched is ignored
    det(10, 5, [0, 0, 0, 10], 0.95)               # zero area: dropped
    det(10, 5, [3, 3, 40, 40], 0.3)
    det(10, 7, [0, 0, 10, 10], 0.99)              # neither gt nor negative: dropped
    det(20, 1, [10, 10, 31, 33], 0.9)
    det(20, 1, [50, 50, 32, 32], 0.9)
    det(20, 1, [11, 11, 30, 32], 0.2)
    det(20, 7, [0, 0, 200, 200], 0.6)
    det(20, 7, [5, 5, 20, 20], 0.6)
    det(20, 9, [1, 2, 3, 4], 0.1)
    det(20, 9, [-5, -5, -3, -3], 0.7)             # negative w and h: area > 0, kept
    det(30, 3, [30, 30, 100, 96], 0.9)
    det(30, 3, [32, 29, 100, 96], 0.9)
    det(30, 3, [31, 31, 99, 95], 0.9)
    det(30, 3, [300, 300, 9, 9], 0.3)
    det(30, 9, [0, 0, 40, 40], 0.8)
    det(30, 13, [0, 0, 40, 40], 0.8)
    det(30, 1, [0, 0, 40, 40], 0.8)               # not in the negative list of 30, no gt: dropped
    for k in range(9):                            # category 1 on image 40: more detections than topk keeps
        det(40, 1, [60 + k, 60 - k, 80, 80 + k], 0.5 + 0.01 * (k % 4))
    det(40, 2, [5, 5, 5, 5], 0.4)
    det(99, 1, [0, 0, 10, 10], 0.99)              # image not in the file
    det(10, 4, [0, 0, 10, 10], 0.99)              # category not in the file
    return gt, P, 12


def medium_case(seed=7):
    from mq_det_amd.utils.synth import synthetic_lvis
    gt, rows = synthetic_lvis(n_img=300, n_cat=120, n_gt=1500, det_per_cat=250, seed=seed, neg_per_img=8, nel_per_img=2, hit_frac=0.6)
    for n, a in enumerate(gt["annotations"]):
        if n % 37 == 0:
            a["ignore"] = 1
    P = [(int(r[0]), int(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[3] + r[5]), float(r[4] + r[6])) for r in rows]
    return gt, P, 200


def predictions(P):
    """rows (image, category, score, x1, y1, x2, y2) -> mdetr-style predictions, one item per image in first-appearance order, fp32 tensors"""
    by_img = {}
    for p in P:
        by_img.setdefault(p[0], []).append(p)
    out = []
    for i, lst in by_img.items():
        a = np.asarray([p[2:] for p in lst], np.float32)
        out.append((i, {"scores": torch.from_numpy(a[:, 0].copy()), "labels": torch.tensor([p[1] for p in lst], dtype=torch.int64),
                        "boxes": torch.from_numpy(a[:, 1:].copy())}))
    return out


def run(lvis, le, gt, P, topk):
    L = lvis.LVIS()
    L.dataset = json.loads(json.dumps(gt))
    L._create_index()
    ev = le.LvisEvaluatorFixedAP(L, topk=topk)
    preds = predictions(P)
    for n in range(0, len(preds), 3):             # three images per engine step
        ev.update(preds[n:n + 3])
    ev.synchronize_between_processes()
    seen = []
    run0 = le.LVISEval.run

    def run_and_keep(self):
        run0(self)
        seen.append(self)
    le.LVISEval.run = run_and_keep
    strings = ev.summarize()
    le.LVISEval.run = run0
    e = seen[0]
    flags = []
    for r in e.eval_imgs:
        if r is None:
            continue
        flags.append({"image_id": int(r["image_id"]), "category_id": int(r["category_id"]), "area": e.params.area_rng.index(r["area_rng"]),
                      "dt_m": (np.asarray(r["dt_matches"]) != 0).astype(int).tolist(), "dt_ig": np.asarray(r["dt_ignore"]).astype(int).tolist(),
                      "gt_ig": np.asarray(r["gt_ignore"]).astype(int).tolist()})
    return preds, strings, {k: float(v) for k, v in e.results.items()}, e.eval["precision"], e.eval["recall"], flags


def save(name, gt, preds, topk, strings, results, precision, recall, flags):
    ids = np.concatenate([np.full(len(p["scores"]), i, np.int64) for i, p in preds])
    np.savez_compressed(OUT + name + ".npz", image_id=ids, scores=np.concatenate([p["scores"].numpy() for _, p in preds]),
                        labels=np.concatenate([p["labels"].numpy() for _, p in preds]),
                        boxes=np.concatenate([p["boxes"].numpy() for _, p in preds]), precision=precision, recall=recall)
    js = {"gt": gt, "topk": topk, "image_order": [int(i) for i, _ in preds], "strings": strings, "results": results}
    if flags is not None:
        js["flags"] = flags
    with open(OUT + name + ".json", "w") as f:
        json.dump(js, f, separators=(",", ":"))
    for ext in (".npz", ".json"):
        size = os.path.getsize(OUT + name + ext)
        print(name + ext, size, "bytes")
        assert size < 1 << 20


def main():
    lvis, le = load_lvis_eval()
    gt, P, topk = small_case()
    out = run(lvis, le, gt, P, topk)
    save("small", gt, out[0], topk, *out[1:])
    gt, P, topk = medium_case()
    out = run(lvis, le, gt, P, topk)
    save("medium", gt, out[0], topk, *out[1:5], None)


if __name__ == "__main__":
    main()
