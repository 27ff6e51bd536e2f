"""TEST INFRASTRUCTURE ONLY: numpy restatement of the reference's phrase-grounding evaluation -- `resize_box` + `flickr_post_process`
(engine/inference.py:314-338) and `Flickr30kEntitiesRecallEvaluator.evaluate` + `FlickrEvaluator.summarize`'s score dict
(data/datasets/evaluation/flickr/flickr_eval.py:152-202,220-255,323-390,420-438) -- on the plain ground-truth dicts
`FlickrRecallEvaluator` takes.  tools/gen_golden_flickr_eval.py pins it against the reference's own code; the tests use it where the
reference leaves a behaviour open (ties in `torch.topk`: here detection order) or where its fixtures do not reach (over 64 boxes)."""
from collections import defaultdict

import numpy as np


def filter_gt(gt, boxes, merge_boxes=False):
    """-> (sentences {image: [kept phrases or None]}, boxes {image: {phrase: [[x1, y1, x2, y2]]}}) as flickr_eval.py:288-318 builds them"""
    out_b, out_s = {}, {}
    for img, sents in gt.items():
        img = str(img)
        bx = {}
        for pid, bl in boxes.get(img, {}).items():
            b = [list(x) for x in bl]
            if merge_boxes and len(b) > 1:
                a = np.asarray(b)
                b = [[a[:, 0].min(), a[:, 1].min(), a[:, 2].max(), a[:, 3].max()]]
            bx[str(pid)] = b
        out_b[img] = bx
        out_s[img] = []
        for s in sents:
            kept = [p for p in (s or []) if str(p["phrase_id"]) in bx]
            out_s[img].append(kept if kept else None)
    return out_s, out_b


def box_iou(b1, b2):
    b1, b2 = np.asarray(b1, dtype=np.float64).reshape(-1, 4), np.asarray(b2, dtype=np.float64).reshape(-1, 4)
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt = np.maximum(b1[:, None, :2], b2[:, :2])
    rb = np.minimum(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clip(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (a1[:, None] + a2 - inter)


def post_process(image_id, sentence_id, boxes, scores, labels, size, orig_size, n_phrases, plus):
    """boxes [n, 4] float32 xyxy at `size` = (width, height), orig_size = (height, width) -> the reference's dict; score descending, ties
    in detection order; the resize in fp32 like BoxList.resize."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    h, w = orig_size
    ratio = np.array([w / size[0], h / size[1], w / size[0], h / size[1]]).astype(np.float32)
    boxes = boxes * ratio
    order = np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")
    out_b, out_s = [[] for _ in range(n_phrases)], [[] for _ in range(n_phrases)]
    for i in order:
        out_b[int(labels[i]) - plus].append([float(v) for v in boxes[i]])
        out_s[int(labels[i]) - plus].append(float(scores[i]))
    for b in out_b:
        b.append([0.0, 0.0, 0.0, 0.0])
    return {"image_id": image_id, "sentence_id": sentence_id, "boxes": out_b, "scores": out_s}


def evaluate(gt, boxes, predictions, topk=(1, 5, 10, -1), iou_thresh=0.5, merge_boxes=False):
    """-> score dict, keys in FlickrEvaluator.summarize's order"""
    sents, bx = filter_gt(gt, boxes, merge_boxes)
    all_ids = {(img, k) for img, ss in sents.items() for k, s in enumerate(ss) if s is not None}
    total = {k: defaultdict(int) for k in topk}
    pos = {k: defaultdict(int) for k in topk}
    seen = set()
    for pred in predictions:
        cur = (str(pred["image_id"]), int(pred["sentence_id"]))
        if cur in seen or cur not in all_ids:
            continue
        seen.add(cur)
        phrases = sents[cur[0]][cur[1]]
        if len(pred["boxes"]) != len(phrases):
            raise RuntimeError("wrong number of phrase lists")
        for cur_boxes, phrase in zip(pred["boxes"], phrases):
            ious = box_iou(cur_boxes, bx[cur[0]][str(phrase["phrase_id"])])
            for k in topk:
                maxi = ious.max() if k == -1 else ious[:k].max()
                for cat in ["all"] + list(phrase["phrase_type"]):
                    total[k][cat] += 1
                    pos[k][cat] += bool(maxi >= iou_thresh)
    if len(seen) != len(all_ids):
        raise RuntimeError("Missing predictions")
    score = {}
    for k in topk:
        header = "Upper_bound" if k == -1 else f"Recall@{k}"
        for cat in sorted(total[topk[0]]):
            score[f"{header}_{cat}"] = pos[k][cat] / total[k][cat]
    return score
