"""Evaluator-side accumulation and gather of detections as TENSORS.

Reference: `LvisEvaluatorFixedAP` (data/datasets/evaluation/lvis/lvis_eval.py:766-808) keeps, per category, the `topk`
(10 000) best detections seen so far as Python lists of dicts (`update`: per-category sort + `_merge_lists`, :752-763) and
exchanges them between ranks by pickling the whole dict through two all_gathers of uint8 tensors
(`synchronize_between_processes` :801-808 -> utils/mdetr_dist.py:32-89) -- the only large message of the eval pipeline
(10^2 - 10^3 MB of pickle).  Here the same state is one [n, 7] fp32 tensor per rank
(image id, category id, score, x, y, w, h) that stays on the device:
  * `update`      appends rows; when the buffer outgrows `prune_at` rows it is cut back to the per-category top-k with two
                  stable sorts (score descending, then category) and a rank-within-category mask -- ties keep the earlier
                  detection, like `_merge_lists`;
  * `synchronize_between_processes`  one all_gather of the row counts and one fixed-shape `all_gather_into_tensor` of the
                  padded rows over RCCL (28 bytes per detection instead of a pickled dict) -- like the reference the
                  per-rank lists are CONCATENATED, not re-trimmed (lvis_eval.py:803-806);
  * `by_cat`      the reference's `{category: [ {"image_id", "category_id", "bbox", "score"} ]}` view for the LVIS API.
Image ids must be exactly representable in fp32 (< 2^24; LVIS / COCO ids are < 600 000).

`LvisFixedAPEvaluator` computes the LVIS Fixed AP from that state on the device (csrc/lvis_eval.hip; DESIGN.md "LVIS Fixed AP")."""
import json
import math
import os
from collections import OrderedDict, defaultdict

import numpy as np
import torch
import torch.distributed as dist


class FixedAPAccumulator:
    def __init__(self, topk=10000, device="cpu", prune_at=None):
        self.topk = int(topk)
        self.device = torch.device(device)
        self.prune_at = prune_at
        self.rows = torch.zeros(0, 7, dtype=torch.float32, device=self.device)
        self._pending = []
        self._npending = 0

    # ------------------------------------------------------------------ accumulate
    def update(self, image_ids, labels, scores, boxes_xywh):
        """Detections of one or more images: image_ids [n] / labels [n] / scores [n] / boxes [n, 4] (x, y, w, h)."""
        n = len(scores)
        if n == 0:
            return
        r = torch.empty(n, 7, dtype=torch.float32, device=self.device)
        r[:, 0] = torch.as_tensor(image_ids, device=self.device).float()
        r[:, 1] = torch.as_tensor(labels, device=self.device).float()
        r[:, 2] = torch.as_tensor(scores, device=self.device).float()
        r[:, 3:] = torch.as_tensor(boxes_xywh, device=self.device).float()
        self._pending.append(r)
        self._npending += n
        limit = self.prune_at if self.prune_at is not None else 4 * max(len(self.rows), 1 << 16)
        if self._npending >= limit:
            self._fold()

    def update_boxlist(self, image_id, boxlist):
        """One reference-style prediction (engine/inference.py:643-648: `output.bbox` in xyxy after `resize_box` to the original
        image size) -> rows with the bbox exactly as `LvisEvaluatorFixedAP.prepare` builds it (lvis_eval.py:810-835 through
        `convert_to_xywh` :998-1000): (xmin, ymin, xmax - xmin, ymax - ymin) -- NO legacy +1 (that is BoxList.convert("xywh"),
        which the LVIS path never calls)."""
        if boxlist.mode != "xyxy":
            boxlist = boxlist.convert("xyxy")
        b = boxlist.bbox
        n = len(b)
        xywh = torch.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1) if n else b.reshape(0, 4)
        self.update(torch.full((n,), float(image_id)), boxlist.get_field("labels"), boxlist.get_field("scores"), xywh)

    def _fold(self):
        if self._pending:
            self.rows = self._prune(torch.cat([self.rows] + self._pending))
            self._pending, self._npending = [], 0

    def _prune(self, rows):
        """Per-category top-k, each category's rows in descending score order, ties in arrival order."""
        if len(rows) == 0:
            return rows
        o = torch.sort(rows[:, 2], descending=True, stable=True)[1]
        rows = rows[o]
        o = torch.sort(rows[:, 1], stable=True)[1]
        rows = rows[o]
        cat = rows[:, 1]
        first = torch.ones(len(rows), dtype=torch.bool, device=rows.device)
        first[1:] = cat[1:] != cat[:-1]
        start = torch.cummax(torch.where(first, torch.arange(len(rows), device=rows.device), torch.zeros((), dtype=torch.long, device=rows.device)), 0)[0]
        rank = torch.arange(len(rows), device=rows.device) - start
        return rows[rank < self.topk]

    # ------------------------------------------------------------------ exchange
    def synchronize_between_processes(self, group=None, force=False):
        """`force`: run the two collectives even in a one-rank group (the one-GPU RCCL test; a one-rank job otherwise has nothing to exchange)."""
        self._fold()
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
            return
        world = dist.get_world_size(group)
        n = torch.tensor([len(self.rows)], dtype=torch.long, device=self.device)
        sizes = torch.empty(world, dtype=torch.long, device=self.device)
        dist.all_gather_into_tensor(sizes, n, group=group)
        sizes = sizes.tolist()
        m = max(max(sizes), 1)
        pad = torch.zeros(m, 7, dtype=torch.float32, device=self.device)
        pad[:len(self.rows)] = self.rows
        out = torch.empty(world * m, 7, dtype=torch.float32, device=self.device)
        dist.all_gather_into_tensor(out, pad, group=group)
        self.rows = torch.cat([out[r * m:r * m + sizes[r]] for r in range(world)])     # concatenated, like the reference

    # ------------------------------------------------------------------ reference view
    def by_cat(self):
        self._fold()
        rows = self.rows.cpu()
        out = defaultdict(list)
        for img, cat, sc, x, y, w, h in rows.tolist():
            out[int(cat)].append({"image_id": int(img), "category_id": int(cat), "bbox": [x, y, w, h], "score": sc})
        return out


# ====================================================================================================== LVIS Fixed AP on the device
_ID_LIMIT = 1 << 24          # ids above are not exact in the accumulator's fp32 rows
_AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
_AREA_LBL = ["all", "small", "medium", "large"]
_FREQ_LBL = ["r", "c", "f"]


def _ids(values, field):
    a = np.asarray(values, dtype=np.float64).reshape(-1)
    if a.size and (not np.all(np.isfinite(a)) or np.any(a != np.round(a))):
        raise ValueError(f"{field}: ids must be integers")
    if a.size and np.any(np.abs(a) >= _ID_LIMIT):
        raise ValueError(f"{field}: ids must lie within +-2^24 (the accumulator keeps them as fp32), got {a[np.abs(a) >= _ID_LIMIT][0]:.0f}")
    return a.astype(np.int64)


class LvisFixedAPEvaluator:
    """Drop-in for the reference's `LvisEvaluatorFixedAP` (data/datasets/evaluation/lvis/lvis_eval.py:766-875) on the default
    `DATASETS.LVIS_USE_NORMAL_AP = False` path of engine/inference.py `build_lvis_evaluator`: the per-category top-k rows stay in a
    `FixedAPAccumulator`, and `summarize()` runs `_summarize_fixed` (LVISResults(max_dets=-1) + LVISEval(iou_type="bbox"), params.max_dets = -1)
    on the device: grouping with torch sorts, matching and accumulation in csrc/lvis_eval.hip, the summary means in torch; one host sync.

    gt: the reference's LVIS object (only `.dataset` is read), a dict in LVIS json format, or a path to such a json."""

    def __init__(self, gt, topk=10000, device="cuda"):
        if isinstance(gt, (str, os.PathLike)):
            with open(gt) as f:
                gt = json.load(f)
        ds = gt if isinstance(gt, dict) else gt.dataset
        self.device = torch.device(device)
        self.topk = int(topk)
        self.acc = FixedAPAccumulator(self.topk, self.device)
        self.results = OrderedDict()
        self.eval = {}
        self.iou_thrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        self._ingest(ds)

    # ------------------------------------------------------------------ ground truth, once
    def _ingest(self, ds):
        dev = self.device
        imgs = {}
        for img in ds["images"]:                       # LVIS._create_index: the last image of an id wins
            imgs[img["id"]] = img
        cats = {}
        for c in ds["categories"]:
            cats[c["id"]] = c
        img_ids = _ids(sorted(imgs), "images.id")
        cat_ids = _ids(sorted(cats), "categories.id")
        K = len(cat_ids)
        self.K = K
        img_pos = {int(i): n for n, i in enumerate(img_ids)}
        cat_pos = {int(c): n for n, c in enumerate(cat_ids)}
        self.freq_groups = [[] for _ in _FREQ_LBL]
        for n, c in enumerate(cat_ids):
            self.freq_groups[_FREQ_LBL.index(cats[int(c)]["frequency"])].append(n)

        def pair_keys(field):
            keys = []
            for i in img_ids:
                lst = imgs[int(i)].get(field, [])
                cs = _ids(lst, f"images.{field}")
                keys.extend(img_pos[int(i)] * K + cat_pos[int(c)] for c in cs if int(c) in cat_pos)
            return torch.tensor(sorted(set(keys)), dtype=torch.int64).to(dev)
        self.neg_keys, self.nel_keys = pair_keys("neg_category_ids"), pair_keys("not_exhaustive_category_ids")

        anns = ds["annotations"]
        a_img = _ids([a["image_id"] for a in anns], "annotations.image_id")
        a_cat = _ids([a["category_id"] for a in anns], "annotations.category_id")
        a_id = np.asarray([a["id"] for a in anns], dtype=np.int64).reshape(-1)
        if len(np.unique(a_id)) != len(a_id):
            raise ValueError("annotations.id: ids must be unique")
        a_area = np.asarray([a["area"] for a in anns], dtype=np.float64).reshape(-1)
        a_box = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        a_ign = np.asarray([bool(a.get("ignore", 0)) for a in anns], dtype=np.uint8).reshape(-1)
        # get_ann_ids(img_ids, cat_ids): images of the file, categories of the file, 0 < area < inf
        keep = np.array([int(i) in img_pos and int(c) in cat_pos for i, c in zip(a_img, a_cat)], dtype=bool).reshape(-1)
        keep &= (a_area > 0) & (a_area < np.inf)
        idx = np.nonzero(keep)[0]
        key = np.array([img_pos[int(a_img[j])] * K + cat_pos[int(a_cat[j])] for j in idx], dtype=np.int64)
        o = np.argsort(key, kind="stable")                  # per pair in annotation-file order
        idx, key = idx[o], key[o]
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)       # noqa: E731
        self.gt_key = t(key, torch.int64)
        self.gt_box = t(a_box[idx].reshape(-1, 4), torch.float64)
        self.gt_area = t(a_area[idx], torch.float64)
        self.gt_ign = t(a_ign[idx], torch.uint8)
        self.gt_nz = t(a_id[idx] != 0, torch.uint8)
        self.img_ids_f = t(img_ids.astype(np.float64), torch.float64)
        self.cat_ids_f = t(cat_ids.astype(np.float64), torch.float64)
        self.area_rng_t = t(np.asarray(_AREA_RNG, np.float64), torch.float64)
        self.iou_thr_t = t(self.iou_thrs, torch.float64)
        self.rec_thr_t = t(self.rec_thrs, torch.float64)
        self.freq_t = [t(np.asarray(g, np.int64), torch.int64) for g in self.freq_groups]

    # ------------------------------------------------------------------ the engine's calls
    def update(self, predictions):
        """predictions: the engine's `mdetr_style_output`, [(image_id, {"scores", "labels", "boxes" xyxy})] -- converted as
        LvisEvaluatorFixedAP.prepare + convert_to_xywh (no legacy +1)."""
        for image_id, pred in predictions:
            if len(pred) == 0:
                continue
            b = pred["boxes"]
            n = len(b)
            if n == 0:
                continue
            xmin, ymin, xmax, ymax = b.unbind(1)
            xywh = torch.stack((xmin, ymin, xmax - xmin, ymax - ymin), dim=1)
            self.acc.update(torch.full((n,), float(image_id)), pred["labels"], pred["scores"], xywh)

    def synchronize_between_processes(self):
        self.acc.synchronize_between_processes()

    def summarize(self):
        """Main process: the strings of LVISEval.print_results (max_dets = -1) and self.results; other ranks: None."""
        if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
            return None
        precision, recall = self.evaluate()
        vals = []
        for kind, thr, area, grp in self._summary_specs():
            vals.append(self._mean(precision if kind == "ap" else recall, kind, thr, area, grp))
        vals = torch.stack(vals).cpu().tolist()            # the one host sync
        self.results = OrderedDict((name, float(v)) for (name, *_), v in zip(self._summary_names(), vals))
        return self.print_results()

    # ------------------------------------------------------------------ evaluate + accumulate
    def _rows(self):
        """_summarize_fixed's results: per category score descending (ties in by_cat() order), cut to topk, then LVISResults / _prepare's
        filters -> (rows, pair key) of the kept detections, sorted by pair (within a pair by score, ties in results order)."""
        acc = self.acc
        acc._fold()
        rows = acc._prune(acc.rows)                        # after a gather the ranks' lists are concatenated: sort and cut again
        dev, K = self.device, self.K
        img, cat = rows[:, 0].double(), rows[:, 1].double()
        ii = torch.searchsorted(self.img_ids_f, img).clamp(max=max(len(self.img_ids_f) - 1, 0))
        ci = torch.searchsorted(self.cat_ids_f, cat).clamp(max=max(K - 1, 0))
        ok = torch.zeros(len(rows), dtype=torch.bool, device=dev)
        if len(self.img_ids_f) and K:
            ok = (self.img_ids_f[ii] == img) & (self.cat_ids_f[ci] == cat)
        area = rows[:, 5].double() * rows[:, 6].double()
        ok &= (area > 0) & (area < math.inf)
        key = ii * K + ci
        ok &= self._member(self.gt_key, key) | self._member(self.neg_keys, key)
        rows, key = rows[ok], key[ok]
        o = torch.sort(key, stable=True)[1]
        return rows[o], key[o]

    @staticmethod
    def _member(sorted_keys, key):
        if len(sorted_keys) == 0:
            return torch.zeros(key.shape, dtype=torch.bool, device=key.device)
        j = torch.searchsorted(sorted_keys, key).clamp(max=len(sorted_keys) - 1)
        return sorted_keys[j] == key

    def evaluate(self):
        """-> (precision [10, 101, K, 4], recall [10, K, 4]) fp64 on the device, as LVISEval.accumulate lays them out; also kept in self.eval
        with the per-detection match bits (test hooks)."""
        from . import ops
        K, dev = self.K, self.device
        rows, dkey = self._rows()
        pkey = torch.unique(torch.cat([self.gt_key, dkey]))                       # every (image, category) pair with a gt or a detection
        i32 = lambda x: x.to(torch.int32)                                          # noqa: E731
        ds, de = torch.searchsorted(dkey, pkey), torch.searchsorted(dkey, pkey, right=True)
        gs, ge = torch.searchsorted(self.gt_key, pkey), torch.searchsorted(self.gt_key, pkey, right=True)
        pair_dt = i32(torch.stack([ds, de - ds], 1)).contiguous()
        pair_gt = i32(torch.stack([gs, ge - gs], 1)).contiguous()
        pair_nel = self._member(self.nel_keys, pkey).to(torch.uint8)
        dt_box = rows[:, 3:7].contiguous()
        dt_bits, gt_count = ops.lvis_match(pair_dt, pair_gt, pair_nel, dt_box, self.gt_box, self.gt_area, self.gt_ign, self.gt_nz,
                                           self.area_rng_t, self.iou_thr_t)
        num_gt = torch.zeros(K, 4, dtype=torch.int64, device=dev)
        num_gt.index_add_(0, pkey % K, gt_count.long())
        # accumulate's order per category: score descending, ties by image id, then by the position in the pair
        o = torch.sort(rows[:, 2], descending=True, stable=True)[1]
        o = o[torch.sort((dkey % K)[o], stable=True)[1]]
        cat_off = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        cat_off[1:] = torch.cumsum(torch.bincount(dkey % K, minlength=K), 0)
        precision, recall = ops.lvis_accumulate(i32(cat_off), i32(o), dt_bits, i32(num_gt).contiguous(), self.rec_thr_t)
        self.eval = {"precision": precision, "recall": recall, "pair_key": pkey, "pair_dt": pair_dt, "pair_gt": pair_gt,
                     "dt_bits": dt_bits, "gt_count": gt_count, "num_gt": num_gt}
        return precision, recall

    # ------------------------------------------------------------------ summary (LVISEval._summarize / summarize / print_results)
    @staticmethod
    def _summary_names():
        return [("AP",), ("AP50",), ("AP75",), ("APs",), ("APm",), ("APl",), ("APr",), ("APc",), ("APf",), ("AR@-1",), ("ARs@-1",), ("ARm@-1",),
                ("ARl@-1",)]

    @staticmethod
    def _summary_specs():
        return [("ap", None, "all", None), ("ap", 0.50, "all", None), ("ap", 0.75, "all", None), ("ap", None, "small", None),
                ("ap", None, "medium", None), ("ap", None, "large", None), ("ap", None, "all", 0), ("ap", None, "all", 1),
                ("ap", None, "all", 2), ("ar", None, "all", None), ("ar", None, "small", None), ("ar", None, "medium", None),
                ("ar", None, "large", None)]

    def _mean(self, s, kind, iou_thr, area, grp):
        aidx = [i for i, lbl in enumerate(_AREA_LBL) if lbl == area]
        if iou_thr is not None:
            s = s[torch.as_tensor(np.where(iou_thr == self.iou_thrs)[0], device=s.device)]
        if kind == "ap":
            s = s[:, :, self.freq_t[grp]] if grp is not None else s
            s = s[..., aidx]
        else:
            s = s[:, :, aidx]
        v = s > -1
        n = v.sum()
        return torch.where(n > 0, torch.where(v, s, torch.zeros((), dtype=s.dtype, device=s.device)).sum() / n.clamp(min=1),
                           torch.full((), -1.0, dtype=torch.float64, device=s.device))

    def print_results(self):
        template = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} catIds={:>3s}] = {:0.3f}"
        out = []
        for key, value in self.results.items():
            title, _type = ("Average Precision", "(AP)") if "AP" in key else ("Average Recall", "(AR)")
            if len(key) > 2 and key[2].isdigit():
                iou = "{:0.2f}".format(float(key[2:]) / 100)
            else:
                iou = "{:0.2f}:{:0.2f}".format(self.iou_thrs[0], self.iou_thrs[-1])
            grp = key[2] if len(key) > 2 and key[2] in ["r", "c", "f"] else "all"
            area = key[2] if len(key) > 2 and key[2] in ["s", "m", "l"] else "all"
            line = template.format(title, _type, iou, area, -1, grp, value)
            print(line)
            out.append(line)
        return out
