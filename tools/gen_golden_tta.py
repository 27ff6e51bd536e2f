#!/usr/bin/env python3
"""Write tests/golden/tta_merge.npz + tta_merge.json: what the reference's own test-time augmentation code returns, executed in place.

maskrcnn_benchmark/data/datasets/evaluation/box_aug.py im_detect_bbox_aug runs from where it lies (oracle/_refload.py shells), with:
  * a stand-in model that returns seeded synthetic detections for every transform (its calls are counted; boxes are drawn in the scaled
    frame of the ImageList it receives) -- the fixture stores them as the packed [T, B, K, 6] rows the device merge reads;
  * torchvision.transforms.functional stubbed by the PIL / torch calls torchvision makes for PIL images (resize, hflip, to_tensor,
    normalize) -- the pixels only reach the stand-in model, the ingest is pinned against Pillow by the tests directly;
  * maskrcnn_benchmark.layers.nms (_C.nms, csrc/cuda/nms.cu) patched with a restatement: greedy +1-IoU NMS in score order, kept indices
    returned ascending (nms.cu:138-142), as oracle/gen_golden.py does for ml_nms; cv2 stubbed (numpy branch, unused).
Resize.get_size, BoxList.transpose / resize, remove_boxes and merge_result_from_multi_scales are the reference's code.

    python tools/gen_golden_tta.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tta_merge")


def nms_restated(boxes, scores, thresh):
    """_C.nms: sort by score (descending), greedy IoU > thresh with the legacy +1, kept indices ascending."""
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order]
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    lt = torch.max(b[:, None, :2], b[None, :, :2])
    rb = torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = (inter / (area[:, None] + area[None, :] - inter) > thresh).numpy()
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= over[i, i + 1:]
    return torch.sort(order[torch.tensor(keep, dtype=torch.long)])[0]


def load_box_aug():
    from oracle import _refload
    ns = _refload.load()
    from PIL import Image

    def resize(img, size, interpolation=None):
        return img.resize((size[1], size[0]), Image.BILINEAR) if isinstance(size, (tuple, list)) else None

    def to_tensor(pic):
        t = torch.from_numpy(np.array(pic, np.uint8, copy=True)).view(pic.size[1], pic.size[0], len(pic.getbands()))
        return t.permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def normalize(t, mean, std):
        m, s = torch.as_tensor(mean, dtype=t.dtype), torch.as_tensor(std, dtype=t.dtype)
        return t.sub(m[:, None, None]).div(s[:, None, None])
    F = types.ModuleType("torchvision.transforms.functional")
    F.resize, F.hflip, F.to_tensor, F.normalize = resize, lambda im: im.transpose(Image.FLIP_LEFT_RIGHT), to_tensor, normalize
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.functional = F
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.transforms.functional": F,
                        "cv2": types.ModuleType("cv2")})
    R = _refload.REF + "/maskrcnn_benchmark"
    for sub in ("data", "data/transforms", "data/datasets", "data/datasets/evaluation"):
        _refload._shell("maskrcnn_benchmark." + sub.replace("/", "."), R + "/" + sub)
    import importlib
    T = importlib.import_module("maskrcnn_benchmark.data.transforms.transforms")
    pkg = sys.modules["maskrcnn_benchmark.data.transforms"]
    for n in ("Compose", "Resize", "RandomHorizontalFlip", "ToTensor", "Normalize"):
        setattr(pkg, n, getattr(T, n))
    sys.modules["maskrcnn_benchmark.data"].transforms = pkg
    conf = sys.modules["maskrcnn_benchmark.config"]
    conf.cfg = ns.defaults._C.clone() if hasattr(ns.defaults._C, "clone") else ns.defaults._C
    L = sys.modules["maskrcnn_benchmark.layers"]
    L.soft_nms = L.nms
    box_aug = importlib.import_module("maskrcnn_benchmark.data.datasets.evaluation.box_aug")
    box_aug.nms = nms_restated
    return box_aug, T, ns.bounding_box, conf.cfg


def main():
    from PIL import Image
    box_aug, T, bb, cfg = load_box_aug()
    d = cfg.TEST
    defaults = {k: (list(map(list, d[k])) if k == "RANGES" else list(d[k]) if isinstance(d[k], (tuple, list)) else d[k])
                for k in ("SCALES", "RANGES", "MAX_SIZE", "FLIP", "SPECIAL_NMS", "TH", "PRE_NMS_TOP_N", "NUM_CLASSES", "SELECT_CLASSES")}
    defaults.update({"INPUT.TO_BGR255": cfg.INPUT.TO_BGR255, "INPUT.FORMAT": cfg.INPUT.FORMAT})

    # Resize.get_size over LVIS-like and odd sizes at the default scales, MAX_SIZE 2500 and 1333 (banker's rounding, truncation)
    sizes = [(640, 480), (480, 640), (500, 375), (375, 500), (640, 427), (427, 640), (333, 500), (1, 7), (7, 1), (2501, 3), (1000, 1000),
             (1801, 1800), (799, 533), (612, 612), (3000, 1200), (1333, 800), (800, 1333)]
    get_size = []
    for (w, h) in sizes:
        for s in list(d.SCALES) + [800, 33]:
            for m in (d.MAX_SIZE, 1333, None):
                get_size.append([w, h, s, -1 if m is None else m] + list(T.Resize(s, m).get_size((w, h))))

    # BoxList.transpose / resize of the reference
    g = torch.Generator().manual_seed(5)
    xy = torch.rand(16, 2, generator=g) * 90
    bx = torch.cat([xy, xy + torch.rand(16, 2, generator=g) * 40], 1)
    bl = bb.BoxList(bx, (131, 97))
    tr = {"box": bx.numpy(), "size": [131, 97], "flip_lr": bl.transpose(0).bbox.numpy(), "flip_tb": bl.transpose(1).bbox.numpy(),
          "resize_eq": bl.resize((262, 194)).bbox.numpy(), "resize_ne": bl.resize((200, 50)).bbox.numpy()}

    cases = {}
    for name, over in (("band", dict(SCALES=(32, 48, 80), RANGES=((24, 10000), (0, 10000), (0, 40)), MAX_SIZE=100, TH=0.5, NUM_CLASSES=7,
                                     SELECT_CLASSES=())),
                       ("noband", dict(SCALES=(40, 72), RANGES=((0, 10000),), MAX_SIZE=2500, TH=0.6, NUM_CLASSES=81, SELECT_CLASSES=(2, 5, 9))),
                       # SELECT_CLASSES out of order: the reference's output follows the list
                       ("unsorted", dict(SCALES=(40, 72), RANGES=((0, 10000),), MAX_SIZE=2500, TH=0.6, NUM_CLASSES=81, SELECT_CLASSES=(9, 2, 5, 3)))):
        for k, v in over.items():
            d[k] = v
        d.FLIP, d.SPECIAL_NMS = True, "none"
        imgs = [Image.new("RGB", (64, 48)), Image.new("RGB", (40, 72))]
        K, B = 40, len(imgs)
        rng = np.random.default_rng({"band": 11, "noband": 12, "unsorted": 13}[name])
        score_pool = rng.permutation(np.arange(1, 4000)).astype(np.float32) / np.float32(4096.0)    # distinct, exact
        dets, calls = [], []
        tie = np.float32(0.1875)

        def model(images, captions=None, positive_map=None):
            t = len(calls)
            calls.append([list(s) for s in images.image_sizes])
            packed = np.zeros((B, K, 6), np.float32)
            counts = []
            out = []
            for b, (h, w) in enumerate(images.image_sizes):
                n = int(rng.integers(K // 2, K - 4))
                x1 = rng.uniform(0, 0.6 * w, n)
                y1 = rng.uniform(0, 0.6 * h, n)
                bw = rng.uniform(1, 0.5 * w, n)
                bh = rng.uniform(1, 0.5 * h, n)
                rows = np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)
                sc = score_pool[(t * B + b) * K:(t * B + b) * K + n].copy()
                sc[sc == tie] = tie + np.float32(1 / 8192)
                lab = rng.integers(0, 12, n).astype(np.float32)
                # rows tied at one score: different classes, small disjoint boxes in the empty bottom-right corner (NMS keeps them all)
                for q in range(4):
                    rows = np.concatenate([rows, np.array([[0.62 * w + 3.5 * q, 0.8 * h, 0.62 * w + 3.5 * q + 2.5, 0.8 * h + 2.5]], np.float32)])
                    sc = np.append(sc, tie)
                    lab = np.append(lab, np.float32([2, 5, 3, 1][q] if t % 2 == 0 else [4, 6, 2, 5][q]))
                order = np.argsort(-sc, kind="stable")           # the model returns its rows score-sorted
                rows, sc, lab = rows[order], sc[order], lab[order]
                m = len(sc)
                packed[b, :m] = np.concatenate([rows, sc[:, None], lab[:, None]], 1)
                counts.append(m)
                r = bb.BoxList(torch.from_numpy(rows.copy()), (w, h), mode="xyxy")
                r.add_field("scores", torch.from_numpy(sc.copy()))
                r.add_field("labels", torch.from_numpy(lab.astype(np.int64)))
                out.append(r)
            dets.append((packed, counts))
            return out

        # first run without the cut: the survivors' scores place PRE_NMS_TOP_N inside the group of tied rows
        d.PRE_NMS_TOP_N = 0
        calls.clear()
        dets.clear()
        rng_state = rng.bit_generator.state
        res0 = box_aug.im_detect_bbox_aug(model, imgs, "cpu", captions=["x"] * B, positive_map_label_to_token={})
        above = [int((r.get_field("scores") > torch.tensor(tie)).sum()) for r in res0]
        ties = [int((r.get_field("scores") == torch.tensor(tie)).sum()) for r in res0]
        top_n = above[0] + 2
        assert ties[0] >= 4 and 2 <= top_n - above[0] < ties[0], (above, ties)
        d.PRE_NMS_TOP_N = top_n
        rng.bit_generator.state = rng_state
        calls.clear()
        dets.clear()
        res = box_aug.im_detect_bbox_aug(model, imgs, "cpu", captions=["x"] * B, positive_map_label_to_token={})
        assert len(res[0]) < len(res0[0]) and len(res[0]) >= top_n
        cases[name] = {
            "cfg": {"SCALES": list(d.SCALES), "RANGES": [list(r) for r in d.RANGES], "MAX_SIZE": d.MAX_SIZE, "FLIP": True, "TH": d.TH,
                    "PRE_NMS_TOP_N": top_n, "NUM_CLASSES": d.NUM_CLASSES, "SELECT_CLASSES": list(d.SELECT_CLASSES)},
            "image_wh": [list(im.size) for im in imgs], "calls": calls, "counts": [c for _, c in dets],
            "out_counts": [len(r) for r in res], "out_counts_nocut": [len(r) for r in res0]}
        np_out = {f"{name}_packed": np.stack([p for p, _ in dets])}
        for b, r in enumerate(res):
            np_out[f"{name}_boxes{b}"] = r.bbox.numpy()
            np_out[f"{name}_scores{b}"] = r.get_field("scores").numpy()
            np_out[f"{name}_labels{b}"] = r.get_field("labels").numpy()
        cases[name]["arrays"] = sorted(np_out)
        tr.update(np_out)
    with open(OUT + ".json", "w") as f:
        json.dump({"defaults": defaults, "get_size": get_size, "cases": cases}, f, indent=None, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **tr)
    print("wrote", OUT + ".json", OUT + ".npz", {k: v["out_counts"] for k, v in cases.items()})


if __name__ == "__main__":
    main()
