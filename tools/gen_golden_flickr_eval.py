#!/usr/bin/env python3
"""Write the fixtures of tests/test_flickr_eval_cpu.py / tests/test_gpu_flickr_eval.py under tests/golden/:

  flickr_eval_small    the hand-made Entities directory tests/golden/flickr_entities (subset test, separate boxes, plus = 1)
  flickr_eval_merged   the same directory with merge_boxes (DATASETS.FLICKR_GT_TYPE = "merged"), plus = 0

Everything recorded is the output of the reference's own code, executed from where it lies through oracle/_refload.py:
`Flickr30kEntitiesRecallEvaluator` (the parsed and filtered ground truth, `evaluate`), `FlickrEvaluator.summarize` (the score dict) and
`resize_box` + `flickr_post_process` on the reference's `BoxList` (the post-processed dicts).  `prettytable` and `mdetr_dist` are stubs.
The synthetic detections have no equal scores within a sentence (asserted: `torch.topk` leaves tie order open), phrases with 0, 1, 5, 10
and 11 detections, a hit only at rank 2, 6 and 11, one IoU of exactly 0.5, and a phrase with a zero-area ground truth next to a normal
one, where the dummy box turns every prefix that reaches it into NaN.  tests/flickr_eval_ref.py must agree (asserted).

    python tools/gen_golden_flickr_eval.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import importlib
import json
import os
import sys
import types
import typing
import xml.etree.ElementTree as ET
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ENT = os.path.join(ROOT, "tests", "golden", "flickr_entities")
OUT = os.path.join(ROOT, "tests", "golden", "flickr_eval_")
FLICKR_EVAL_PY = "maskrcnn_benchmark/data/datasets/evaluation/flickr/flickr_eval.py"
INFERENCE_PY = "maskrcnn_benchmark/engine/inference.py"

import flickr_eval_ref as ref  # noqa: E402

# network input (width, height) per image; 1002 keeps its own size: the ratios are 1 and the IoU of exactly 0.5 survives the resize
NET_SIZE = {"1001": (800, 600), "1002": (640, 480), "1003": (533, 800), "1004": (600, 600)}
# (detections, rank of the only hit or None) dealt to the evaluated phrases in reading order
PLANS = [(5, 2), (1, 1), (0, None), (10, 6), (11, 11), (1, None), (5, None), (10, 1), (11, None), (3, 3), (10, 10), (5, 5), (11, 6)]


class _Table:
    """prettytable.PrettyTable stand-in"""
    field_names = None

    def add_row(self, row):
        pass

    def __str__(self):
        return ""


def reference_code():
    from oracle import _refload
    R = _refload.REF + "/maskrcnn_benchmark"
    if "maskrcnn_benchmark" not in sys.modules:
        _refload._shell("maskrcnn_benchmark", R)
    if "maskrcnn_benchmark.structures" not in sys.modules:
        _refload._shell("maskrcnn_benchmark.structures", R + "/structures")
    BoxList = importlib.import_module("maskrcnn_benchmark.structures.bounding_box").BoxList
    glb = {"np": np, "ET": ET, "defaultdict": defaultdict, "Path": Path, "PrettyTable": _Table,
           "dist": types.SimpleNamespace(is_main_process=lambda: True, all_gather=lambda x: [x])}
    glb.update({n: getattr(typing, n) for n in ("Any", "Dict", "List", "Optional", "Sequence", "Tuple", "Union")})
    code = _refload.reference_classes(FLICKR_EVAL_PY, ["RecallTracker", "Flickr30kEntitiesRecallEvaluator", "FlickrEvaluator"],
                                      ["get_sentence_data", "get_annotations", "box_area", "_box_inter_union", "box_iou", "_merge_boxes"], glb)
    fn = _refload.reference_functions(INFERENCE_PY, ["resize_box", "flickr_post_process"])
    return BoxList, code["FlickrEvaluator"], fn["flickr_post_process"]


def detections(evaluator, plus, seed):
    """-> per evaluated-or-not sentence (image, sentence id, size, orig (h, w), n_phrases, boxes, scores, labels); sentences that are not
    evaluated get a stray prediction too (the evaluator must ignore it)"""
    g = np.random.default_rng(seed)
    sizes = {}
    for img in evaluator.img_ids:
        root = ET.parse(os.path.join(ENT, "Annotations", f"{img}.xml")).getroot()
        sizes[img] = (int(root.find("size/height").text), int(root.find("size/width").text))
    out, plan_no = [], 0
    for img in evaluator.img_ids:
        h, w = sizes[img]
        nw, nh = NET_SIZE[img]
        ratio = np.array([nw / w, nh / h, nw / w, nh / h])
        for sid, phrases in enumerate(evaluator.imgid2sentences[img]):
            rows = []
            for j, ph in enumerate(phrases or []):
                gts = np.asarray(evaluator.imgid2boxes[img][ph["phrase_id"]], dtype=np.float64)
                if img == "1002" and ph["phrase_id"] == "11" and sid == 2:
                    n, hit, hit_box = 1, 1, np.array([0.0, 0.0, 100.0, 50.0])                 # IoU 5000 / 10000 with [0, 0, 100, 100]
                elif ph["phrase_id"] == "22":
                    n, hit, hit_box = 5, 1, gts[-1]                                            # zero-area box first, the normal one last
                else:
                    n, hit = PLANS[plan_no % len(PLANS)]
                    plan_no += 1
                    hit_box = gts[int(g.integers(len(gts)))]
                for rank in range(1, n + 1):
                    if rank == hit:
                        box = hit_box
                    else:                                                                      # IoU 0.25 with its ground truth, or far away
                        gt0 = gts[0]
                        shift = 0.6 * (gt0[2] - gt0[0]) if rank % 2 else 3.0 * w
                        box = gt0 + np.array([shift, 0, shift, 0])
                    rows.append((j + plus, 0.95 - 0.05 * rank - 0.003 * j, box * ratio))
            if phrases is None:
                rows.append((plus, 0.5, np.array([1.0, 2.0, 30.0, 40.0])))
            perm = g.permutation(len(rows))
            labels = np.array([rows[i][0] for i in perm], dtype=np.int64)
            scores = np.array([rows[i][1] for i in perm], dtype=np.float32)
            boxes = np.array([rows[i][2] for i in perm], dtype=np.float32).reshape(-1, 4)
            assert len(np.unique(scores)) == len(scores), "equal scores within a sentence"
            out.append((img, sid, (nw, nh), (h, w), len(phrases or [0]), boxes, scores, labels))
    return out


def case(name, merge, plus, BoxList, FlickrEvaluator, flickr_post_process):
    fe = FlickrEvaluator(ENT, "test", merge_boxes=merge)
    ev = fe.evaluator
    dets = detections(ev, plus, seed=3 + merge)
    post = []
    for img, sid, size, orig, n_ph, boxes, scores, labels in dets:
        bl = BoxList(torch.from_numpy(boxes.copy()), size, mode="xyxy")
        bl.add_field("scores", torch.from_numpy(scores.copy()))
        bl.add_field("labels", torch.from_numpy(labels.copy()))
        tgt = BoxList(torch.zeros(0, 4), size, mode="xyxy")
        tgt.add_field("orig_size", torch.tensor(orig))
        tgt.add_field("original_img_id", img)
        tgt.add_field("sentence_id", sid)
        p = flickr_post_process(bl, [tgt], {k + plus: [k] for k in range(n_ph)}, plus)
        post.append({"image_id": p["image_id"], "sentence_id": p["sentence_id"], "boxes": p["boxes"], "scores": [[float(s) for s in ss] for ss in p["scores"]]})
    fe.update(post)
    fe.synchronize_between_processes()
    score = fe.summarize()
    gt_sent = {i: [None if s is None else [{"phrase_id": p["phrase_id"], "phrase_type": p["phrase_type"]} for p in s] for s in ss]
               for i, ss in ev.imgid2sentences.items()}
    gt_box = {i: {p: [[int(v) for v in b] for b in bl] for p, bl in d.items()} for i, d in ev.imgid2boxes.items()}
    mine = ref.evaluate(gt_sent, gt_box, post, merge_boxes=False)        # (the recorded boxes are merged already)
    assert list(mine.items()) == list(score.items()), (mine, score)
    for (img, sid, size, orig, n_ph, boxes, scores, labels), p in zip(dets, post):
        q = ref.post_process(img, sid, boxes, scores, labels, size, orig, n_ph, plus)
        assert q["boxes"] == p["boxes"], (img, sid)
    meta = {"merge_boxes": bool(merge), "plus": plus, "subset": "test", "topk": [1, 5, 10, -1], "iou_thresh": 0.5,
            "gt_sentences": gt_sent, "gt_boxes": gt_box, "all_ids": ev.all_ids,
            "sentences": [{"image_id": d[0], "sentence_id": d[1], "size": list(d[2]), "orig_size": list(d[3]), "n_phrases": d[4]} for d in dets],
            "post": post, "score": [[k, v] for k, v in score.items()]}
    with open(OUT + name + ".json", "w") as f:
        json.dump(meta, f)
    off = np.cumsum([0] + [len(d[5]) for d in dets])
    np.savez_compressed(OUT + name + ".npz", off=off, boxes=np.concatenate([d[5] for d in dets]), scores=np.concatenate([d[6] for d in dets]),
                        labels=np.concatenate([d[7] for d in dets]))
    for ext in (".json", ".npz"):
        size = os.path.getsize(OUT + name + ext)
        print(os.path.basename(OUT + name + ext), size, "bytes")
        assert size < 100 << 10
    print(name, score)


if __name__ == "__main__":
    code = reference_code()
    case("small", False, 1, *code)
    case("merged", True, 0, *code)
