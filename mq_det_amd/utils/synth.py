"""Seeded synthetic weights / inputs for benchmarking (no checkpoints or datasets exist offline).

`randomize_(model)` re-draws every parameter so that all branches of the network are numerically live
(the reference zero-initialises the GCP gates, the layer-scale and the DCN offset conv): fan-in scaled normals
for weights, ~N(1, 0.1) norm scales, small biases, O(1 px) deformable offsets, alignment bias chosen so that a
few percent of the (location, class) scores clear the 0.05 threshold and the post-processing sees real work.
"""
import math

import torch


@torch.no_grad()
def randomize_(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        shape = tuple(p.shape)
        if name.endswith("ff_gate"):
            p.fill_(0.3)
        elif name.endswith("log_scale"):
            p.fill_(0.0)
        elif name.endswith("bias0"):
            p.fill_(-6.0)
        elif name.endswith(".scale"):
            p.fill_(1.0)
        elif "gamma_" in name:
            p.copy_(torch.randn(shape, generator=g) * 0.05 + 0.5)
        elif name.endswith("relative_position_bias_table"):
            p.copy_(torch.randn(shape, generator=g) * 0.5)
        elif "embeddings" in name and name.endswith("weight") and p.dim() == 2:
            p.copy_(torch.randn(shape, generator=g) * 0.3)
        elif p.dim() == 1:
            if name.endswith("weight") and ("norm" in name.lower() or ".bn." in name):
                p.copy_(torch.randn(shape, generator=g) * 0.1 + 1.0)
            else:
                p.copy_(torch.randn(shape, generator=g) * 0.05)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            gain = 40.0 if "dot_product_projection_text" in name else (1.5 if ("qkv" in name or "query" in name or "key" in name or "to_q" in name or "to_kv" in name or "v_proj" in name or "l_proj" in name) else 1.0)
            p.copy_(torch.randn(shape, generator=g) * (gain / math.sqrt(fan_in)))
    model._invalidate()
    return model


def synthetic_bank(labels, channels=256, k=5, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {int(l): torch.randn(k, 1, channels, generator=g) for l in labels}


# LVIS v1 frequency split of its 1203 categories (rare / common / frequent)
LVIS_FREQ_SPLIT = (337, 461, 405)


def synthetic_lvis(n_img=4809, n_cat=1203, n_gt=50000, det_per_cat=10000, seed=0, neg_per_img=15, nel_per_img=2, hit_frac=0.3):
    """Seeded LVIS-shaped ground truth (a dict in LVIS json format) and detections (numpy: image id, category id, score, x, y, w, h as
    float32 rows, per category `det_per_cat` rows).  A `hit_frac` share of each category's detections are jittered copies of its ground
    truths, the rest lie on random images (most of them fall outside the image's positive / negative categories, as in LVIS).  Scores
    are quantised to 1/4096 so that ties occur."""
    import numpy as np
    g = np.random.default_rng(seed)
    img_ids = np.sort(g.choice(np.arange(1, 600000), n_img, replace=False))
    cat_ids = np.arange(1, n_cat + 1)
    split = np.cumsum([round(n_cat * f / sum(LVIS_FREQ_SPLIT)) for f in LVIS_FREQ_SPLIT])
    freq = ["r" if c < split[0] else "c" if c < split[1] else "f" for c in range(n_cat)]
    wh = g.integers(320, 641, (n_img, 2))
    gi = g.integers(0, n_img, n_gt)
    gc = g.integers(0, n_cat, n_gt)
    gw = np.maximum(g.random(n_gt) ** 2 * wh[gi, 0] * 0.8, 1.0)
    gh = np.maximum(g.random(n_gt) ** 2 * wh[gi, 1] * 0.8, 1.0)
    gx, gy = g.random(n_gt) * (wh[gi, 0] - gw), g.random(n_gt) * (wh[gi, 1] - gh)
    anns = [{"id": int(n + 1), "image_id": int(img_ids[gi[n]]), "category_id": int(cat_ids[gc[n]]),
             "bbox": [float(gx[n]), float(gy[n]), float(gw[n]), float(gh[n])], "area": float(gw[n] * gh[n])} for n in range(n_gt)]
    images = []
    for i in range(n_img):
        neg = g.choice(n_cat, neg_per_img, replace=False)
        nel = g.choice(n_cat, nel_per_img, replace=False)
        images.append({"id": int(img_ids[i]), "width": int(wh[i, 0]), "height": int(wh[i, 1]),
                       "neg_category_ids": [int(cat_ids[c]) for c in neg], "not_exhaustive_category_ids": [int(cat_ids[c]) for c in nel]})
    gt = {"images": images, "annotations": anns,
          "categories": [{"id": int(c), "name": f"c{c}", "frequency": f} for c, f in zip(cat_ids, freq)]}
    by_cat = [[] for _ in range(n_cat)]
    for n in range(n_gt):
        by_cat[gc[n]].append(n)
    rows = np.zeros((n_cat * det_per_cat, 7), np.float32)
    for c in range(n_cat):
        r = rows[c * det_per_cat:(c + 1) * det_per_cat]
        nh = int(det_per_cat * hit_frac) if by_cat[c] else 0
        src = np.asarray(by_cat[c], np.int64)[g.integers(0, max(len(by_cat[c]), 1), nh)] if nh else np.zeros(0, np.int64)
        ri = g.integers(0, n_img, det_per_cat - nh)
        r[:, 1] = cat_ids[c]
        r[:nh, 0] = img_ids[gi[src]]
        r[nh:, 0] = img_ids[ri]
        j = lambda v, s: v * (1 + s * g.standard_normal(len(v)))                          # noqa: E731
        r[:nh, 3], r[:nh, 4] = j(gx[src] + 1, 0.05), j(gy[src] + 1, 0.05)
        r[:nh, 5], r[:nh, 6] = j(gw[src], 0.1), j(gh[src], 0.1)
        rw, rh = g.random(len(ri)) * wh[ri, 0] * 0.5 + 1, g.random(len(ri)) * wh[ri, 1] * 0.5 + 1
        r[nh:, 3], r[nh:, 4], r[nh:, 5], r[nh:, 6] = g.random(len(ri)) * (wh[ri, 0] - rw), g.random(len(ri)) * (wh[ri, 1] - rh), rw, rh
        r[:, 2] = np.floor(g.random(det_per_cat) * 4096) / 4096
    return gt, rows


def synthetic_coco(n_img=5000, n_cat=80, gt_per_img=7.0, det_per_img=100, seed=0, crowd_frac=0.02, hit_frac=0.5, grid=0):
    """Seeded COCO-shaped ground truth (a dict in COCO json format, `crowd_frac` of the annotations iscrowd) and predictions as the
    engine holds them: [(image id, (width, height) of the network input, boxes xyxy float32 [n, 4] at that size, scores float32 [n],
    labels int64 [n] = 1 + the category's position)], `det_per_img` per image.  A `hit_frac` share of an image's detections are jittered
    copies of its ground truths (with their category most of the time), the rest are random.  Scores are quantised to 1/1024 so that ties
    occur.  grid > 0: the network input has the image's size and every coordinate is a multiple of 1 / grid (exact in fp32 sums)."""
    import numpy as np
    g = np.random.default_rng(seed)
    img_ids = np.sort(g.choice(np.arange(1, 600000), n_img, replace=False))
    cat_ids = np.sort(g.choice(np.arange(1, 4 * n_cat + 1), n_cat, replace=False))
    wh = g.integers(320, 641, (n_img, 2))
    pwh = wh if grid else g.integers(400, 801, (n_img, 2))
    ng = g.poisson(gt_per_img, n_img)
    gi = np.repeat(np.arange(n_img), ng)
    n_gt = len(gi)
    gc = g.integers(0, n_cat, n_gt)
    gw = np.maximum(g.random(n_gt) ** 2 * wh[gi, 0] * 0.8, 2.0)
    gh = np.maximum(g.random(n_gt) ** 2 * wh[gi, 1] * 0.8, 2.0)
    gx, gy = g.random(n_gt) * (wh[gi, 0] - gw), g.random(n_gt) * (wh[gi, 1] - gh)
    if grid:
        gx, gy, gw, gh = (np.round(v * grid) / grid for v in (gx, gy, np.maximum(gw, 2.0), np.maximum(gh, 2.0)))
    crowd = g.random(n_gt) < crowd_frac
    anns = [{"id": int(n + 1), "image_id": int(img_ids[gi[n]]), "category_id": int(cat_ids[gc[n]]), "iscrowd": int(crowd[n]),
             "bbox": [float(gx[n]), float(gy[n]), float(gw[n]), float(gh[n])], "area": float(gw[n] * gh[n])} for n in range(n_gt)]
    gt = {"images": [{"id": int(img_ids[i]), "width": int(wh[i, 0]), "height": int(wh[i, 1])} for i in range(n_img)], "annotations": anns,
          "categories": [{"id": int(c), "name": f"c{c}"} for c in cat_ids]}
    first = np.concatenate([[0], np.cumsum(ng)])
    N = n_img * det_per_img
    di = np.repeat(np.arange(n_img), det_per_img)
    hit = (g.random(N) < hit_frac) & (ng[di] > 0)
    src = np.minimum(first[di] + (g.random(N) * ng[di]).astype(np.int64), max(n_gt - 1, 0))
    j = lambda v, s: v * (1 + s * g.standard_normal(N))                                   # noqa: E731
    rw, rh = g.random(N) * wh[di, 0] * 0.5 + 2, g.random(N) * wh[di, 1] * 0.5 + 2
    rx, ry = g.random(N) * (wh[di, 0] - rw), g.random(N) * (wh[di, 1] - rh)
    if n_gt:
        x, y = np.where(hit, j(gx[src] + 1, 0.05), rx), np.where(hit, j(gy[src] + 1, 0.05), ry)
        w, h = np.where(hit, np.maximum(j(gw[src], 0.1), 1.0), rw), np.where(hit, np.maximum(j(gh[src], 0.1), 1.0), rh)
        lab = np.where(hit & (g.random(N) < 0.8), gc[src], g.integers(0, n_cat, N)) + 1
    else:
        x, y, w, h, lab = rx, ry, rw, rh, g.integers(0, n_cat, N) + 1
    if grid:
        x, y, w, h = (np.round(v * grid) / grid for v in (x, y, np.maximum(w, 1.0), np.maximum(h, 1.0)))
    sx, sy = pwh[di, 0] / wh[di, 0], pwh[di, 1] / wh[di, 1]
    # xyxy with the legacy convention: convert("xywh") adds 1 to x2 - x1
    boxes = np.stack([x * sx, y * sy, (x + w - 1) * sx, (y + h - 1) * sy], 1).astype(np.float32)
    scores = (np.floor(g.random(N) * 1024) / 1024).astype(np.float32)
    preds = []
    for i in range(n_img):
        s = slice(i * det_per_img, (i + 1) * det_per_img)
        preds.append((int(img_ids[i]), (int(pwh[i, 0]), int(pwh[i, 1])), boxes[s], scores[s], lab[s].astype(np.int64)))
    return gt, preds


FLICKR_TYPES = ("people", "clothing", "bodyparts", "animals", "vehicles", "instruments", "scene", "other")


def synthetic_flickr(n_img=1000, sent_per_img=5, phrases_per_sent=3.0, det_per_sent=300, seed=0, hit_frac=0.5, max_gt=3, score_levels=0,
                     same_size=False):
    """Seeded Flickr30k-Entities-shaped ground truth, as `FlickrRecallEvaluator` takes it, and detections as the model returns them:
    -> (gt {image id: [sentence = list of {"phrase_id", "phrase_type"}]}, boxes {image id: {phrase id: [[x1, y1, x2, y2] ints]}},
    preds [(image id, sentence id, (width, height) of the network input, (height, width) of the image, number of phrases, boxes xyxy float32
    [n, 4] at the input size, scores float32 [n], phrase index int64 [n])]).  A sentence has 1 + Poisson(phrases_per_sent - 1) phrases (at most
    10) of 1 .. max_gt boxes and one or two types, and up to `det_per_sent` detections; a `hit_frac` share of them are jittered copies of a
    ground truth of their phrase, the rest are random.  score_levels > 0 quantises the scores so that ties occur; same_size: the network
    input has the image's size (ratio 1)."""
    import numpy as np
    g = np.random.default_rng(seed)
    gt, boxes, preds = {}, {}, []
    for i in range(n_img):
        img = str(100000 + 7 * i)
        w, h = int(g.integers(320, 641)), int(g.integers(320, 641))
        nw, nh = (w, h) if same_size else (int(g.integers(400, 1334)), int(g.integers(400, 801)))
        gt[img], boxes[img] = [], {}
        for s in range(sent_per_img):
            n_ph = int(min(10, 1 + g.poisson(max(phrases_per_sent - 1, 0))))
            sent, gts = [], []
            for p in range(n_ph):
                pid = str(1000 * s + p)
                k = int(g.integers(1, max_gt + 1))
                bw, bh = g.integers(8, w // 2, k), g.integers(8, h // 2, k)
                x, y = (g.random(k) * (w - bw)).astype(np.int64), (g.random(k) * (h - bh)).astype(np.int64)
                b = np.stack([x, y, x + bw, y + bh], 1)
                boxes[img][pid] = b.tolist()
                gts.append(b.astype(np.float64))
                types = list(g.choice(FLICKR_TYPES, 1 + int(g.random() < 0.15), replace=False))
                sent.append({"phrase_id": pid, "phrase_type": [str(t) for t in types]})
            gt[img].append(sent)
            n = int(g.integers(det_per_sent // 2, det_per_sent + 1)) if det_per_sent > 1 else det_per_sent
            ph = g.integers(0, n_ph, n)
            hit = g.random(n) < hit_frac
            b = np.empty((n, 4))
            rw, rh = g.random(n) * w * 0.5 + 2, g.random(n) * h * 0.5 + 2
            rx, ry = g.random(n) * (w - rw), g.random(n) * (h - rh)
            b[:] = np.stack([rx, ry, rx + rw, ry + rh], 1)
            for d in np.nonzero(hit)[0]:
                src = gts[ph[d]]
                b[d] = src[int(g.integers(len(src)))] + g.normal(0, 6, 4)
            sc = g.random(n)
            if score_levels:
                sc = np.floor(sc * score_levels) / score_levels
            ratio = np.array([nw / w, nh / h, nw / w, nh / h])
            preds.append((img, s, (nw, nh), (h, w), n_ph, (b * ratio).astype(np.float32), sc.astype(np.float32), ph.astype(np.int64)))
    return gt, boxes, preds
