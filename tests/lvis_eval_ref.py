"""TEST INFRASTRUCTURE ONLY: a plain-Python / numpy restatement of the reference's LVIS Fixed AP path -- `LvisEvaluatorFixedAP._summarize_fixed`
(lvis_eval.py:849-875) through LVISResults(max_dets=-1) and LVISEval(iou_type="bbox") -- for the tests of mq_det_amd.evaluation
LvisFixedAPEvaluator.  `bbiou` restates pycocotools' bbIou (maskApi.c) with iscrowd = 0; `evaluate_img` restates lvis_eval.py:318-410 line by
line.  The fixtures under tests/golden/lvis_eval* pin the same path by running the reference's own code (tools/gen_golden_lvis_eval.py)."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def bbiou(d, g):
    """pycocotools bbIou, one pair, iscrowd = 0, in double"""
    ga, da = g[2] * g[3], d[2] * d[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    return i / (da + ga - i)


def evaluate_img(dts, gts, area_rng, nel):
    """dts: [(score, bbox, area)] in the pair's results order; gts: [(id, bbox, area, ignore)] in annotation-file order; nel: the category
    is not exhaustively annotated in the image -> (dt_m != 0 [10, D] bool, dt_ig [10, D] bool, gt_ig [G] int) in the reference's orders."""
    gt_ig_all = [1 if (g[3] or g[2] < area_rng[0] or g[2] > area_rng[1]) else 0 for g in gts]
    gi = np.argsort(gt_ig_all, kind="mergesort")
    gts = [gts[i] for i in gi]
    gt_ig = np.array([gt_ig_all[i] for i in gi], dtype=np.int64)
    di = np.argsort([-d[0] for d in dts], kind="mergesort")
    dts = [dts[i] for i in di]
    T, G, D = len(IOU_THRS), len(gts), len(dts)
    ious = [[bbiou(d[1], g[1]) for g in gts] for d in dts] if G and D else []
    gt_m = np.zeros((T, G))
    dt_m = np.zeros((T, D))
    dt_ig = np.zeros((T, D))
    for t, thr in enumerate(IOU_THRS):
        if len(ious) == 0:
            break
        for d in range(D):
            iou = min([thr, 1 - 1e-10])
            m = -1
            for g in range(G):
                if gt_m[t, g] > 0:
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
            dt_m[t, d] = gts[m][0]
            gt_m[t, m] = d + 1
    mask = np.array([d[2] < area_rng[0] or d[2] > area_rng[1] or nel for d in dts], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(dt_m == 0, np.repeat(mask, T, 0)))
    return dt_m != 0, dt_ig, gt_ig, [dts[i][0] for i in range(D)]


def prepare(gt, rows, topk):
    """_summarize_fixed's results (per category: score descending, ties in row order, cut to topk) + LVISResults / LVISEval._prepare ->
    (img_ids, cat_ids, gts {(img, cat): [...]}, dts {(img, cat): [...]}, nel {img: set}, freq groups)."""
    imgs = {im["id"]: im for im in gt["images"]}
    cats = {c["id"]: c for c in gt["categories"]}
    img_ids, cat_ids = sorted(imgs), sorted(cats)
    by_cat = {}
    for r in rows.tolist():
        by_cat.setdefault(int(r[1]), []).append(r)
    results = []
    for c, lst in by_cat.items():
        results.extend(sorted(lst, key=lambda r: r[2], reverse=True)[:topk])
    gts = {}
    per_img = {}
    for a in gt["annotations"]:
        per_img.setdefault(a["image_id"], []).append(a)
    for i in img_ids:
        for a in per_img.get(i, []):
            if a["category_id"] in cats and 0 < a["area"] < float("inf"):
                gts.setdefault((i, a["category_id"]), []).append((a["id"], list(map(float, a["bbox"])), float(a["area"]), bool(a.get("ignore", 0))))
    pl = {}
    for (i, c) in gts:
        pl.setdefault(i, set()).add(c)
    dts = {}
    for r in results:
        i, c = int(r[0]), int(r[1])
        if float(r[0]) != i or float(r[1]) != c:
            continue
        area = r[5] * r[6]
        if i not in imgs or c not in cats or not (0 < area < float("inf")):
            continue
        if c not in imgs[i]["neg_category_ids"] and c not in pl.get(i, set()):
            continue
        dts.setdefault((i, c), []).append((r[2], r[3:7], area))
    nel = {i: set(imgs[i]["not_exhaustive_category_ids"]) for i in img_ids}
    groups = [[n for n, c in enumerate(cat_ids) if cats[c]["frequency"] == f] for f in "rcf"]
    return img_ids, cat_ids, gts, dts, nel, groups


def summarize_fixed(gt, rows, topk):
    """-> (precision, recall, results OrderedDict, strings, per-pair flags {(img, cat, area_idx): (dt_m, dt_ig, gt_ig)})"""
    from collections import OrderedDict
    img_ids, cat_ids, gts, dts, nel, groups = prepare(gt, rows, topk)
    T, R, K, A = len(IOU_THRS), len(REC_THRS), len(cat_ids), 4
    precision, recall = -np.ones((T, R, K, A)), -np.ones((T, K, A))
    flags = {}
    for k, c in enumerate(cat_ids):
        for a, rng in enumerate(AREA_RNG):
            E = []
            for i in img_ids:
                g, d = gts.get((i, c), []), dts.get((i, c), [])
                if not g and not d:
                    continue
                m, ig, gig, sc = evaluate_img(d, g, rng, c in nel[i])
                flags[(i, c, a)] = (m, ig, gig)
                E.append((m, ig, gig, sc))
            if not E:
                continue
            sc = np.concatenate([np.asarray(e[3], np.float64) for e in E])
            o = np.argsort(-sc, kind="mergesort")
            dm = np.concatenate([e[0] for e in E], 1)[:, o]
            di = np.concatenate([e[1] for e in E], 1)[:, o]
            ng = np.count_nonzero(np.concatenate([e[2] for e in E]) == 0)
            if ng == 0:
                continue
            tps, fps = np.logical_and(dm, np.logical_not(di)), np.logical_and(np.logical_not(dm), np.logical_not(di))
            for t, (tp, fp) in enumerate(zip(np.cumsum(tps, 1).astype(float), np.cumsum(fps, 1).astype(float))):
                rc = tp / ng
                recall[t, k, a] = rc[-1] if len(tp) else 0
                pr = (tp / (fp + tp + np.spacing(1))).tolist()
                for i in range(len(tp) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                q = [0.0] * R
                try:
                    for j, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        q[j] = pr[pi]
                except Exception:
                    pass
                precision[t, :, k, a] = np.array(q)

    def mean(kind, thr=None, area="all", grp=None):
        aidx = [n for n, lbl in enumerate(["all", "small", "medium", "large"]) if lbl == area]
        s = precision if kind == "ap" else recall
        if thr is not None:
            s = s[np.where(thr == IOU_THRS)[0]]
        s = (s[:, :, groups[grp], aidx] if grp is not None else s[:, :, :, aidx]) if kind == "ap" else s[:, :, aidx]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    res = OrderedDict()
    res["AP"], res["AP50"], res["AP75"] = mean("ap"), mean("ap", 0.50), mean("ap", 0.75)
    res["APs"], res["APm"], res["APl"] = mean("ap", area="small"), mean("ap", area="medium"), mean("ap", area="large")
    res["APr"], res["APc"], res["APf"] = mean("ap", grp=0), mean("ap", grp=1), mean("ap", grp=2)
    res["AR@-1"] = mean("ar")
    for lbl in ("small", "medium", "large"):
        res[f"AR{lbl[0]}@-1"] = mean("ar", area=lbl)
    template = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} catIds={:>3s}] = {:0.3f}"
    strings = []
    for key, v in res.items():
        title, ty = ("Average Precision", "(AP)") if "AP" in key else ("Average Recall", "(AR)")
        iou = "{:0.2f}".format(float(key[2:]) / 100) if len(key) > 2 and key[2].isdigit() else "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1])
        grp = key[2] if len(key) > 2 and key[2] in "rcf" else "all"
        ar = key[2] if len(key) > 2 and key[2] in "sml" else "all"
        strings.append(template.format(title, ty, iou, ar, -1, grp, v))
    return precision, recall, res, strings, flags
