"""TEST INFRASTRUCTURE ONLY: a plain-Python / numpy restatement of the COCO branch of the reference's evaluation -- `results_dict.update`
and `prepare_for_coco_detection` (engine/inference.py:649-650, coco_eval.py:129-157), then pycocotools' `COCO.loadRes`, `COCOeval._prepare`,
`computeIoU` (with maskApi.c's `bbIou`, crowd included), `evaluateImg`, `accumulate` and `summarize` for iouType bbox, and the reference's
`summarize_per_category` -- for the tests of mq_det_amd.evaluation.CocoAPEvaluator.  Written step by step after pycocotools' published
sources.

What it rests on: pycocotools is NOT installed where the fixtures are made, so no line of it ever ran against this file.  The one slice
that code of the reference pins is the crowd-free maxDets = 100 one: tests/golden/coco_eval_bridge holds the precision / recall arrays and
the per-detection flags of the reference's own LVISEval on a ground truth where LVIS and COCO rules coincide, and
tests/test_coco_eval_cpu.py asserts that this file reproduces them.  Crowd handling and maxDets 1 / 10 rest on this restatement alone;
`prepare_for_coco_detection`, `summarize_per_category` and `COCOResults` are pinned by tests/golden/coco_eval_prepare (the reference's own
functions, executed in place)."""
from collections import OrderedDict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]


def result_rows(items, gt, label_to_cat_id=None):
    """items: [(image id, size (w, h), boxes xyxy fp32 [n, 4], scores fp32 [n], labels [n])] in arrival order -> the rows
    (image id, category id, score, x, y, w, h) of `coco_results`, float64 holding fp32 values: the dict update (the last prediction of an
    image wins, an empty one too), images in ascending id order, BoxList.resize to the ground truth's (width, height) and
    convert("xywh") in fp32, labels through the map."""
    imgs = {im["id"]: im for im in gt["images"]}
    if label_to_cat_id is None:
        label_to_cat_id = {i + 1: c for i, c in enumerate(sorted({c["id"] for c in gt["categories"]}))}
    last = {}
    for it in items:
        last[it[0]] = it
    rows = []
    for i in sorted(last):
        _, size, boxes, scores, labels = last[i]
        if len(boxes) == 0:
            continue
        b = np.asarray(boxes, np.float32).reshape(-1, 4)
        if i in imgs:
            tw, th = imgs[i]["width"], imgs[i]["height"]
            rw, rh = float(tw) / float(size[0]), float(th) / float(size[1])
            b = b * np.array([rw, rh, rw, rh]).astype(np.float32)           # BoxList.resize: fp32 boxes times the ratio as fp32
        one = np.float32(1)
        xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + one, b[:, 3] - b[:, 1] + one], 1)
        for k in range(len(b)):
            if int(labels[k]) in label_to_cat_id:
                rows.append([float(i), float(label_to_cat_id[int(labels[k])]), float(np.float32(scores[k]))] + [float(v) for v in xywh[k]])
    return np.asarray(rows, np.float64).reshape(-1, 7)


def bbiou(d, g, crowd):
    """maskApi.c bbIou, one pair, in double"""
    ga, da = g[2] * g[3], d[2] * d[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def prepare(gt, rows):
    """COCO.createIndex / loadRes / COCOeval._prepare -> (img_ids, cat_ids, gts {(img, cat): [(id, bbox, area, iscrowd)]} in
    annotation-file order, dts {(img, cat): [(score, bbox, area)]} in results order)"""
    imgs = {im["id"]: im for im in gt["images"]}
    cats = {c["id"]: c for c in gt["categories"]}
    img_ids, cat_ids = sorted(imgs), sorted(cats)
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    if not set(int(r[0]) for r in rows) <= set(img_ids):
        raise ValueError("Results do not correspond to current coco set")
    per_img = {}
    for a in gt.get("annotations", []):
        per_img.setdefault(a["image_id"], []).append(a)
    gts = {}
    for i in img_ids:
        for a in per_img.get(i, []):
            if a["category_id"] in cats:
                gts.setdefault((i, a["category_id"]), []).append((a["id"], [float(v) for v in a["bbox"]], float(a["area"]), int(a.get("iscrowd", 0))))
    dts = {}
    by_img = {}
    for r in rows.tolist():
        by_img.setdefault(int(r[0]), []).append(r)
    for i in img_ids:
        for r in by_img.get(i, []):
            if int(r[1]) in cats:
                dts.setdefault((i, int(r[1])), []).append((r[2], r[3:7], r[5] * r[6]))
    return img_ids, cat_ids, gts, dts


def evaluate_img(dts, gts, area_rng, max_det=MAX_DETS[-1], ids=False):
    """-> (dtm != 0 [10, D] bool, dtIg [10, D] bool, gtIg [G] int in the sorted order, scores [D]); D = min(len(dts), max_det).
    ids: dtm itself (the matched annotation ids) instead of dtm != 0, and the detections in their sorted order as a fifth item."""
    ig_all = [1 if (g[3] or g[2] < area_rng[0] or g[2] > area_rng[1]) else 0 for g in gts]
    gi = np.argsort(ig_all, kind="mergesort")
    gts = [gts[i] for i in gi]
    gt_ig = np.array([ig_all[i] for i in gi], dtype=np.int64)
    di = np.argsort([-d[0] for d in dts], kind="mergesort")
    dts = [dts[i] for i in di[0:max_det]]
    crowd = [int(g[3]) for g in gts]
    T, G, D = len(IOU_THRS), len(gts), len(dts)
    ious = [[bbiou(d[1], g[1], g[3]) for g in gts] for d in dts] if G and D else []
    gtm, dtm, dt_ig = np.zeros((T, G)), np.zeros((T, D)), np.zeros((T, D))
    if len(ious):
        for t, thr in enumerate(IOU_THRS):
            for d in range(D):
                iou = min([thr, 1 - 1e-10])
                m = -1
                for g in range(G):
                    if gtm[t, g] > 0 and not crowd[g]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[g] == 1:
                        break
                    if ious[d][g] < iou:
                        continue
                    iou = ious[d][g]
                    m = g
                if m == -1:
                    continue
                dt_ig[t, d] = gt_ig[m]
                dtm[t, d] = gts[m][0]
                gtm[t, m] = d + 1                      # the detection's id: loadRes numbers them from 1
    out = np.array([d[2] < area_rng[0] or d[2] > area_rng[1] for d in dts], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out, T, 0)))
    if ids:
        return dtm, dt_ig, gt_ig, [d[0] for d in dts], dts
    return dtm != 0, dt_ig, gt_ig, [d[0] for d in dts]


def pack_bits(flags, img_ids, cat_ids):
    """flags {(img, cat, area): (dtm [10, D], dtIg [10, D], gtIg)} -> (pair image ids, pair category ids, detections per pair, dt_bits
    [sum D, 2] uint64 with bit = area * 10 + threshold, gt_count [P, 4]) with the pairs in (image, category) order"""
    pairs = sorted({(img_ids.index(i), cat_ids.index(c)) for i, c, _ in flags})
    pi, pc, pd, bits, cnt = [], [], [], [], []
    for ii, ci in pairs:
        i, c = img_ids[ii], cat_ids[ci]
        D = flags[(i, c, 0)][0].shape[1]
        w = np.zeros((D, 2), np.uint64)
        for a in range(4):
            m, ig, gig = flags[(i, c, a)]
            for t in range(10):
                w[:, 0] |= m[t].astype(np.uint64) << np.uint64(a * 10 + t)
                w[:, 1] |= ig[t].astype(np.uint64) << np.uint64(a * 10 + t)
        pi.append(i), pc.append(c), pd.append(D), bits.append(w)
        cnt.append([int(np.count_nonzero(np.asarray(flags[(i, c, a)][2]) == 0)) for a in range(4)])
    return (np.asarray(pi, np.int64), np.asarray(pc, np.int64), np.asarray(pd, np.int64),
            np.concatenate(bits).reshape(-1, 2) if bits else np.zeros((0, 2), np.uint64), np.asarray(cnt, np.int64).reshape(-1, 4))


def summarize_lines(precision, recall):
    """COCOeval.summarize -> (stats [12], the printed lines)"""
    template = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"

    def one(ap, thr=None, area="all", max_dets=100):
        aind = [n for n, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [n for n, m in enumerate(MAX_DETS) if m == max_dets]
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap else s[:, :, aind, mind]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if thr is None else "{:0.2f}".format(thr)
        return mean, template.format("Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, max_dets, mean)
    out = [one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"), one(0, max_dets=1),
           one(0, max_dets=10), one(0), one(0, area="small"), one(0, area="medium"), one(0, area="large")]
    return [float(v) for v, _ in out], [s for _, s in out]


def evaluate(gt, rows):
    """COCOeval.evaluate + accumulate + summarize -> dict(precision [10, 101, K, 4, 3], recall [10, K, 4, 3], stats, strings, results,
    flags {(img, cat, area): (dtm != 0, dtIg, gtIg)})"""
    img_ids, cat_ids, gts, dts = prepare(gt, rows)
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    flags = {}
    for k, c in enumerate(cat_ids):
        for a, rng in enumerate(AREA_RNG):
            E = []
            for i in img_ids:
                g, d = gts.get((i, c), []), dts.get((i, c), [])
                if not g and not d:
                    continue
                m, ig, gig, sc = evaluate_img(d, g, rng)
                flags[(i, c, a)] = (m, ig, gig)
                E.append((m, ig, gig, np.asarray(sc, np.float64)))
            if not E:
                continue
            for mi, max_det in enumerate(MAX_DETS):
                sc = np.concatenate([e[3][0:max_det] for e in E])
                o = np.argsort(-sc, kind="mergesort")
                dm = np.concatenate([e[0][:, 0:max_det] for e in E], 1)[:, o]
                di = np.concatenate([e[1][:, 0:max_det] for e in E], 1)[:, o]
                npig = np.count_nonzero(np.concatenate([e[2] for e in E]) == 0)
                if npig == 0:
                    continue
                tps, fps = np.logical_and(dm, np.logical_not(di)), np.logical_and(np.logical_not(dm), np.logical_not(di))
                for t, (tp, fp) in enumerate(zip(np.cumsum(tps, 1).astype(float), np.cumsum(fps, 1).astype(float))):
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    try:
                        for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, mi] = np.array(q)
    stats, strings = summarize_lines(precision, recall)
    results = OrderedDict([("bbox", OrderedDict(zip(["AP", "AP50", "AP75", "APs", "APm", "APl"], stats)))])
    return {"precision": precision, "recall": recall, "stats": stats, "strings": strings, "results": results, "flags": flags,
            "img_ids": img_ids, "cat_ids": cat_ids}
