#!/usr/bin/env python3
"""Write the fixtures of tests/test_coco_eval_cpu.py / tests/test_gpu_coco_eval.py under tests/golden/:

  coco_eval_prepare   the reference's own `prepare_for_coco_detection` (coco_eval.py:129-157) and `BoxList` (structures/bounding_box.py),
                      executed in place through oracle/_refload.py on a stub dataset: an unknown label, an empty prediction, square and
                      non-square resize ratios; and its `summarize_per_category` / `COCOResults.update` on a stub `coco_eval` object.
  coco_eval_bridge    the reference's own LVISEval (loaded as tools/gen_golden_lvis_eval.py does) on a ground truth where LVIS and COCO
                      rules coincide -- asserted below: no crowd, no `ignore`, every image lists every category it has no annotation of in
                      neg_category_ids, no not_exhaustive_category_ids, at most 100 detections per pair, max_dets = -1 -- next to what
                      tests/coco_eval_ref.py gives on the same rows.
  coco_eval_small     hand-made, every rule (the list in tests/test_coco_eval_cpu.py); expected outputs of tests/coco_eval_ref.py.
  coco_eval_medium    seeded random with crowds; expected outputs of tests/coco_eval_ref.py.

pycocotools is not installed here: `pycocotools.cocoeval.COCOeval` is an empty stand-in class (COCOResults.update only asks isinstance),
and the per-category lines of every case are the reference's `summarize_per_category` on a stub holding the case's precision array.

    python tools/gen_golden_coco_eval.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import importlib
import json
import os
import sys
import tempfile
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "coco_eval_")
COCO_EVAL_PY = "maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py"

import coco_eval_ref as ref  # noqa: E402


def check_size(path):
    size = os.path.getsize(path)
    print(os.path.basename(path), size, "bytes")
    assert size < 1 << 20


class Stub:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def reference_code():
    """-> (BoxList, prepare_for_coco_detection, summarize_per_category, COCOResults, COCOeval stand-in) of the reference, run in place"""
    from oracle import _refload
    R = _refload.REF + "/maskrcnn_benchmark"
    if "maskrcnn_benchmark" not in sys.modules:
        _refload._shell("maskrcnn_benchmark", R)
    if "maskrcnn_benchmark.structures" not in sys.modules:
        _refload._shell("maskrcnn_benchmark.structures", R + "/structures")
    BoxList = importlib.import_module("maskrcnn_benchmark.structures.bounding_box").BoxList
    fn = _refload.reference_functions(COCO_EVAL_PY, ["prepare_for_coco_detection", "summarize_per_category"], {"np": np})
    cocoeval = types.ModuleType("pycocotools.cocoeval")
    cocoeval.COCOeval = type("COCOeval", (), {})
    if "pycocotools" not in sys.modules:
        pc = types.ModuleType("pycocotools")
        pc.__path__ = []
        sys.modules["pycocotools"] = pc
    sys.modules["pycocotools.cocoeval"] = cocoeval
    cls = _refload.reference_classes(COCO_EVAL_PY, ["COCOResults"], extra_globals={"OrderedDict": OrderedDict})
    return BoxList, fn["prepare_for_coco_detection"], fn["summarize_per_category"], cls["COCOResults"], cocoeval.COCOeval


def per_category_lines(summarize_per_category, COCOeval, gt, precision, stats=None):
    """the reference's summarize_per_category on a stub coco_eval -> the lines it writes"""
    cats = {c["id"]: c for c in gt["categories"]}
    ce = COCOeval()
    ce.params = Stub(iouThrs=ref.IOU_THRS, areaRngLbl=ref.AREA_LBL, maxDets=ref.MAX_DETS, catIds=sorted(cats), iouType="bbox")
    ce.eval = {"precision": precision}
    ce.cocoGt = Stub(cats=cats)
    ce.stats = np.asarray(stats) if stats is not None else None
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bbox.csv")
        summarize_per_category(ce, path)
        with open(path) as f:
            text = f.read()
    return ce, text


# ---------------------------------------------------------------------------------------------------------------- prepare
def prepare_case(BoxList, prepare_for_coco_detection, summarize_per_category, COCOResults, COCOeval):
    g = np.random.default_rng(11)
    imgs = {7: (640, 480), 3: (500, 375), 12: (333, 500), 5: (640, 427), 9: (400, 400)}        # id -> (width, height)
    sizes = {7: (800, 600), 3: (1066, 800), 12: (800, 1201), 5: (1199, 800), 9: (400, 400)}    # the network's input: 7 has equal ratios
    label_map = {1: 18, 2: 44, 3: 3, 5: 90}                                                    # label 4 is unknown
    order = [7, 3, 12, 5, 9]
    items, preds = [], []
    for i in order:
        n = 0 if i == 5 else int(g.integers(6, 12))                                             # image 5: an empty prediction
        w, h = sizes[i]
        x1, y1 = g.random(n) * w * 0.7, g.random(n) * h * 0.7
        b = np.stack([x1, y1, x1 + g.random(n) * w * 0.3, y1 + g.random(n) * h * 0.3], 1).astype(np.float32).reshape(-1, 4)
        labels = g.integers(1, 6, n).astype(np.int64)
        if n:
            labels[0] = 4
        scores = g.random(n).astype(np.float32)
        bl = BoxList(torch.from_numpy(b.copy()), (w, h), mode="xyxy")
        bl.add_field("scores", torch.from_numpy(scores.copy()))
        bl.add_field("labels", torch.from_numpy(labels.copy()))
        preds.append(bl)
        items.append((i, (w, h), b, scores, labels))
    dataset = Stub(id_to_img_map={n: i for n, i in enumerate(order)}, coco=Stub(imgs={i: {"width": s[0], "height": s[1]} for i, s in imgs.items()}),
                   contiguous_category_id_to_json_id=label_map)
    res = prepare_for_coco_detection(preds, dataset)
    rows = np.asarray([[r["image_id"], r["category_id"], r["score"]] + r["bbox"] for r in res], np.float64).reshape(-1, 7)
    assert len(rows) and not (rows[:, 0] == 5).any() and set(rows[:, 1].astype(int)) <= set(label_map.values())
    assert sum(int((it[4] == 4).sum()) for it in items) > 0 and len(rows) == sum(int((it[4] != 4).sum()) for it in items)
    gt = {"images": [{"id": i, "width": s[0], "height": s[1]} for i, s in imgs.items()], "annotations": [],
          "categories": [{"id": c, "name": f"name {c}"} for c in sorted(label_map.values())]}
    again = ref.result_rows(items, gt, label_map)                                              # the restatement's own prepare, against the reference
    assert np.array_equal(again[np.argsort(again[:, 0], kind="stable")], rows[np.argsort(rows[:, 0], kind="stable")])
    # summarize_per_category / COCOResults on a stub coco_eval
    K = len(gt["categories"])
    precision = g.random((10, 101, K, 4, 3))
    precision[:, 60:, 1] = -1
    precision[:, :, 2, 1] = -1                                                                 # no small object of category 2: that line ends early
    precision[:, :, :, 2] = -1                                                                 # no medium object at all
    stats = g.random(12)
    ce, text = per_category_lines(summarize_per_category, COCOeval, gt, precision, stats)
    results = COCOResults("bbox")
    results.update(ce)
    np.savez_compressed(OUT + "prepare.npz", image_id=np.concatenate([np.full(len(it[2]), it[0], np.int64) for it in items]),
                        boxes=np.concatenate([it[2] for it in items]), scores=np.concatenate([it[3] for it in items]),
                        labels=np.concatenate([it[4] for it in items]), rows=rows, precision=precision, stats=stats)
    with open(OUT + "prepare.json", "w") as f:
        json.dump({"gt": gt, "label_to_cat_id": sorted(label_map.items()), "image_order": order, "sizes": {str(i): list(s) for i, s in sizes.items()},
                   "per_category": text, "results": {k: dict(v) for k, v in results.results.items()}}, f, separators=(",", ":"))
    check_size(OUT + "prepare.npz"), check_size(OUT + "prepare.json")


# ---------------------------------------------------------------------------------------------------------------- the evaluation cases
def small_case():
    """Hand-made: every rule of the COCO evaluation (the coverage assertions of tests/test_coco_eval_cpu.py)."""
    cats = [1, 2, 3, 5, 7]
    images = [{"id": 10, "width": 200, "height": 200}, {"id": 20, "width": 200, "height": 160}, {"id": 30, "width": 320, "height": 240},
              {"id": 40, "width": 100, "height": 100},                                          # neither ground truth nor detection
              {"id": 50, "width": 100, "height": 60}]
    sizes = {10: (200, 200), 20: (200, 160), 30: (640, 480), 40: (333, 333), 50: (200, 150)}     # 50: ratios 1/2 and 2/5
    label_map = {1: 1, 2: 2, 3: 3, 4: 5, 5: 7, 6: 99}                                           # 99: a category the file lacks; 9: unknown
    A = []

    def ann(i, c, box, area=None, **kw):
        A.append(dict({"id": len(A) + 1, "image_id": i, "category_id": c, "bbox": box, "area": box[2] * box[3] if area is None else area,
                       "iscrowd": 0}, **kw))
    ann(10, 1, [0, 0, 50, 50], iscrowd=1)              # a crowd: three detections take it
    ann(10, 1, [10, 10, 20, 20])                       # a non-crowd inside the crowd
    ann(10, 2, [0, 0, 10, 10])                         # IoU exactly 0.5 with its detection
    ann(10, 2, [20, 0, 10, 10])                        # IoU exactly 0.75
    ann(20, 2, [0, 0, 100, 100])                       # large: out of range for small / medium, matched once only there
    ann(20, 1, [10, 10, 30, 30])                       # gets id 0 below
    ann(20, 1, [60, 60, 31, 33])                       # area 1023
    ann(20, 1, [100, 100, 32, 32], area=1024.0)        # the small / medium boundary
    for n in range(12):                                # image 30, category 3: twelve ground truths, more than 100 detections
        ann(30, 3, [10 + 25 * n, 10, 20, 20 + n])
    ann(30, 3, [0, 100, 300, 100], iscrowd=1)
    ann(50, 5, [10, 10, 40, 30])                       # category 5: ground truths and no detection
    ann(50, 3, [5, 5, 20, 20])
    ann(99, 1, [0, 0, 10, 10])                         # image not in the file
    ann(10, 4, [0, 0, 10, 10])                         # category not in the file
    A[5]["id"] = 0
    del A[6]["iscrowd"]                                # iscrowd defaults to 0
    gt = {"images": images, "annotations": A, "categories": [{"id": c, "name": f"thing {c}"} for c in cats]}
    P = {i["id"]: [] for i in images}

    def det(i, label, box, s):                         # box xywh in the ground truth's frame -> xyxy (legacy: x2 = x + w - 1) at the network's size
        sx, sy = sizes[i][0] / [m for m in images if m["id"] == i][0]["width"], sizes[i][1] / [m for m in images if m["id"] == i][0]["height"]
        P[i].append((label, s, box[0] * sx, box[1] * sy, (box[0] + box[2] - 1) * sx, (box[1] + box[3] - 1) * sy))
    det(10, 1, [5, 5, 10, 10], 0.95)                   # inside the crowd, off the non-crowd: crowd IoU exactly 1
    det(10, 1, [30, 30, 15, 15], 0.9)                  # inside the crowd too
    det(10, 1, [10, 10, 20, 16], 0.85)                 # crowd IoU 1 > non-crowd IoU 0.8: takes the non-crowd up to 0.8
    det(10, 1, [12, 12, 20, 20], 0.5)                  # the non-crowd is taken: falls to the crowd
    det(10, 1, [150, 150, 20, 20], 0.4)                # unmatched
    det(10, 2, [0, 0, 5, 10], 0.9)                     # IoU 0.5
    det(10, 2, [20, 0, 7.5, 10], 0.9)                  # IoU 0.75, tied score inside the pair
    det(10, 6, [0, 0, 10, 10], 0.99)                   # category 99
    det(10, 9, [0, 0, 10, 10], 0.99)                   # unknown label
    det(20, 2, [0, 0, 100, 100], 0.9)                  # tied with image 10's across images
    det(20, 2, [0, 0, 100, 90], 0.8)                   # IoU 0.9 with the same ground truth: unmatched, and out of range where the gt is
    det(20, 1, [10, 10, 30, 30], 0.7)                  # matches the id-0 ground truth
    det(20, 1, [60, 60, 31, 33], 0.6)
    det(20, 1, [100, 100, 32, 32], 0.6)
    det(20, 5, [0, 0, 50, 50], 0.3)                    # category 7: detections and no ground truth
    det(20, 5, [120, 20, 50, 50], 0.2)
    for n in range(12):
        det(30, 3, [10 + 25 * n, 10, 20, 20 + n], 0.30 - 0.01 * n if n < 2 else 0.05 - 0.001 * n)
    for n in range(95):                                # 107 detections on the pair: the last ones fall to the cut
        det(30, 3, [(7 * n) % 280, 100 + (11 * n) % 90, 12, 12], 0.29 - 0.002 * n if n < 20 else 0.04 - 0.0001 * n)
    det(50, 3, [5, 5, 20, 20], 0.9)
    det(50, 3, [40, 20, 30, 30], 0.1)
    order = [10, 20, 30, 40, 50]                       # 40 with an empty prediction
    items = []
    for i in order:
        a = np.asarray(P[i], np.float64).reshape(-1, 6)
        items.append((i, sizes[i], a[:, 2:].astype(np.float32), a[:, 1].astype(np.float32), a[:, 0].astype(np.int64)))
    return gt, items, label_map


def medium_case():
    from mq_det_amd.utils.synth import synthetic_coco
    gt, items = synthetic_coco(n_img=60, n_cat=10, gt_per_img=6.0, det_per_img=40, seed=3, crowd_frac=0.08)
    return gt, items, None


def bridge_case():
    from mq_det_amd.utils.synth import synthetic_coco
    gt, items = synthetic_coco(n_img=50, n_cat=8, gt_per_img=5.0, det_per_img=30, seed=5, crowd_frac=0.0, grid=4)
    cats = [c["id"] for c in gt["categories"]]
    have = {}
    for a in gt["annotations"]:
        del a["iscrowd"]
        have.setdefault(a["image_id"], set()).add(a["category_id"])
    for im in gt["images"]:
        im["neg_category_ids"] = [c for c in cats if c not in have.get(im["id"], set())]
        im["not_exhaustive_category_ids"] = []
    for n, c in enumerate(gt["categories"]):
        c["frequency"] = "rcf"[n % 3]
    return gt, items, None


def run_bridge(gt, items, rows):
    """the reference's LVISEval on the COCO rows -> (precision [10, 101, K, 4], recall [10, K, 4], packed flags)"""
    from gen_golden_lvis_eval import load_lvis_eval
    lvis, le = load_lvis_eval()
    # the conditions under which the two rule sets coincide
    assert not any(a.get("iscrowd") or a.get("ignore") for a in gt["annotations"])
    cats = {c["id"] for c in gt["categories"]}
    have = {}
    for a in gt["annotations"]:
        have.setdefault(a["image_id"], set()).add(a["category_id"])
        assert a["area"] > 0
    for im in gt["images"]:
        assert set(im["neg_category_ids"]) == cats - have.get(im["id"], set()) and im["not_exhaustive_category_ids"] == []
    per_pair = {}
    for r in rows:
        per_pair[(r[0], r[1])] = per_pair.get((r[0], r[1]), 0) + 1
    assert max(per_pair.values()) <= 100 and (rows[:, 5] * rows[:, 6] > 0).all()
    L = lvis.LVIS()
    L.dataset = json.loads(json.dumps(gt))
    L._create_index()
    ev = le.LvisEvaluatorFixedAP(L, topk=10000)
    r32 = rows.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), rows)
    x2, y2 = r32[:, 3] + r32[:, 5], r32[:, 4] + r32[:, 6]
    assert np.array_equal(x2 - r32[:, 3], r32[:, 5]) and np.array_equal(y2 - r32[:, 4], r32[:, 6])        # LVIS's x2 - x1 gives the COCO row's w back
    preds = []
    for i in sorted(set(rows[:, 0].astype(int))):
        m = rows[:, 0] == i
        preds.append((int(i), {"scores": torch.from_numpy(r32[m, 2].copy()), "labels": torch.from_numpy(rows[m, 1].astype(np.int64)),
                               "boxes": torch.from_numpy(np.stack([r32[m, 3], r32[m, 4], x2[m], y2[m]], 1))}))
    for n in range(0, len(preds), 3):
        ev.update(preds[n:n + 3])
    ev.synchronize_between_processes()
    seen = []
    run0 = le.LVISEval.run

    def run_and_keep(self):
        run0(self)
        seen.append(self)
    le.LVISEval.run = run_and_keep
    ev.summarize()
    le.LVISEval.run = run0
    e = seen[0]
    assert e.params.max_dets == -1
    flags = {}
    for r in e.eval_imgs:
        if r is not None:
            flags[(int(r["image_id"]), int(r["category_id"]), e.params.area_rng.index(r["area_rng"]))] = (
                np.asarray(r["dt_matches"]) != 0, np.asarray(r["dt_ignore"]).astype(bool), np.asarray(r["gt_ignore"]))
    return e.eval["precision"], e.eval["recall"], flags


def save_case(name, gt, items, label_map, code, extra=None):
    _, _, summarize_per_category, COCOResults, COCOeval = code
    rows = ref.result_rows(items, gt, label_map)
    out = ref.evaluate(gt, rows)
    pi, pc, pd, bits, cnt = ref.pack_bits(out["flags"], out["img_ids"], out["cat_ids"])
    ce, text = per_category_lines(summarize_per_category, COCOeval, gt, out["precision"], out["stats"])
    res = COCOResults("bbox")
    res.update(ce)
    assert {k: float(v) for k, v in res.results["bbox"].items()} == dict(out["results"]["bbox"])
    arrays = dict(image_id=np.concatenate([np.full(len(it[2]), it[0], np.int64) for it in items]),
                  boxes=np.concatenate([it[2].reshape(-1, 4) for it in items]), scores=np.concatenate([it[3] for it in items]),
                  labels=np.concatenate([it[4] for it in items]), rows=rows, precision=out["precision"], recall=out["recall"],
                  pair_img=pi, pair_cat=pc, pair_D=pd, dt_bits=bits, gt_count=cnt)
    if extra:
        extra(rows, out, arrays)
    np.savez_compressed(OUT + name + ".npz", **arrays)
    with open(OUT + name + ".json", "w") as f:
        json.dump({"gt": gt, "label_to_cat_id": sorted(label_map.items()) if label_map else None, "image_order": [it[0] for it in items],
                   "sizes": {str(it[0]): list(it[1]) for it in items}, "strings": out["strings"], "stats": out["stats"],
                   "results": {"bbox": dict(out["results"]["bbox"])}, "per_category": text}, f, separators=(",", ":"))
    check_size(OUT + name + ".npz"), check_size(OUT + name + ".json")
    print(name, len(rows), "rows;", out["strings"][0])


def main():
    code = reference_code()
    prepare_case(*code)
    gt, items, label_map = small_case()
    save_case("small", gt, items, label_map, code)
    gt, items, label_map = medium_case()
    save_case("medium", gt, items, label_map, code)
    gt, items, label_map = bridge_case()

    def bridge(rows, out, arrays):
        p, r, flags = run_bridge(gt, items, rows)
        arrays["lvis_precision"], arrays["lvis_recall"] = p, r
        ids = ref.pack_bits(flags, out["img_ids"], out["cat_ids"])
        for k, v in zip(("lvis_pair_img", "lvis_pair_cat", "lvis_pair_D", "lvis_dt_bits", "lvis_gt_count"), ids):
            arrays[k] = v
        print("bridge: restatement == LVISEval:", np.array_equal(out["precision"][..., 2], p), np.array_equal(out["recall"][..., 2], r),
              all(np.array_equal(arrays["lvis_" + k], arrays[k]) for k in ("pair_img", "pair_cat", "pair_D", "dt_bits", "gt_count")))
    save_case("bridge", gt, items, label_map, code, bridge)


if __name__ == "__main__":
    main()
