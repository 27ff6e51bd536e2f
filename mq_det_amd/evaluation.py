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

`LvisFixedAPEvaluator` computes the LVIS Fixed AP from that state on the device (csrc/ap_eval.hip; DESIGN.md "LVIS Fixed AP").
`CocoAPEvaluator` computes pycocotools' COCO AP (COCO / ODinW) from rows of the same kind (csrc/ap_eval.hip, the same kernels under COCO's rules; DESIGN.md "COCO AP").
`FlickrRecallEvaluator` computes Flickr30k Entities Recall@k (phrase grounding) from such rows (csrc/flickr_eval.hip; DESIGN.md "Phrase grounding").
`update_packed` of the first two takes a forward's packed detections as they lie on the device: csrc/eval_rows.hip builds the rows in one launch and
`append_block` keeps them with their device count until the next fold (mq_det_amd/detection.py; DESIGN.md "Detection evaluation loop")."""
import json
import math
import os
import re
import warnings
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

    def append_block(self, rows_buffer, n_rows_dev):
        """Rows that were built on the device (ops.eval_rows): the buffer [capacity, columns] is kept whole together with the device int that
        says how many of its rows are live; `_fold()` reads the pending counts at once.  Towards the prune trigger a block weighs its capacity,
        the number the host knows."""
        if rows_buffer.dim() != 2 or rows_buffer.shape[1] != self.rows.shape[1] or rows_buffer.dtype != torch.float32:
            raise ValueError(f"append_block: rows of shape [n, {self.rows.shape[1]}] fp32 expected, got {tuple(rows_buffer.shape)} {rows_buffer.dtype}")
        self._pending.append((rows_buffer, n_rows_dev.reshape(())))
        self._npending += len(rows_buffer)
        limit = self.prune_at if self.prune_at is not None else 4 * max(len(self.rows), 1 << 16)
        if self._npending >= limit:
            self._fold()

    def _fold(self):
        if self._pending:
            blocks = [p for p in self._pending if isinstance(p, tuple)]
            if blocks:                                         # every pending block's row count in ONE device->host read
                live = iter(torch.stack([n for _, n in blocks]).tolist())
                self._pending = [p[0][:max(0, min(int(next(live)), len(p[0])))] if isinstance(p, tuple) else p for p in self._pending]
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
        cols = self.rows.shape[1]
        pad = torch.zeros(m, cols, dtype=torch.float32, device=self.device)
        pad[:len(self.rows)] = self.rows
        out = torch.empty(world * m, cols, dtype=torch.float32, device=self.device)
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


def _packed_rows(ev, packed, counts, image_ids, n_chunks, candidate, cols, ratios, **mode):
    """The launch both evaluators' `update_packed` share: entry table in image-major order out of the forward's chunk-major items (the B x g
    permutation), a fresh row buffer of the full capacity, one ops.eval_rows; -> (rows buffer, state [2] int32 on the device: rows written,
    overflow bit).  The overflow bit is folded into ev._tie_overflow on the device."""
    from . import ops
    ids = _ids(image_ids, "predictions.image_id")
    B, g = len(ids), int(n_chunks)
    if packed.dim() != 3 or packed.shape[0] != g * B or len(ratios) != B:
        raise ValueError(f"update_packed: {B} images x {g} chunks, packed detections of shape {tuple(packed.shape)}, {len(ratios)} image sizes")
    K2 = packed.shape[1]
    table = ops.eval_rows_table([c * B + b for b in range(B) for c in range(g)], [float(i) for i in ids for _ in range(g)],
                                [r[0] for r in ratios for _ in range(g)], [r[1] for r in ratios for _ in range(g)],
                                [c == 0 for _ in range(B) for c in range(g)], g * B, ev.device)
    rows = torch.empty(g * B * K2 + (B if mode.get("placeholder") else 0), cols, dtype=torch.float32, device=ev.device)
    state = torch.empty(2, dtype=torch.int32, device=ev.device)
    ops.eval_rows(packed.contiguous(), counts.contiguous(), table, rows, state, cols=cols, candidate=candidate, **mode)
    ev._tie_overflow = state[1] if ev._tie_overflow is None else torch.maximum(ev._tie_overflow, state[1])
    return rows, state


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


def _not_main_process():
    return dist.is_available() and dist.is_initialized() and dist.get_rank() != 0


def _masked_mean(s):
    """Mean of the entries above -1 (the kernels' mark for "no ground truth"), -1 where there is none; on the device."""
    v = s > -1
    n = v.sum()
    return torch.where(n > 0, torch.where(v, s, torch.zeros((), dtype=s.dtype, device=s.device)).sum() / n.clamp(min=1),
                       torch.full((), -1.0, dtype=torch.float64, device=s.device))


class _APEvaluator:
    """What LvisFixedAPEvaluator and CocoAPEvaluator share: the ground truth as device tensors, the (image, category) pairs the match
    kernel of csrc/ap_eval.hip works on and the per-category order its accumulate kernel reads."""

    def __init__(self, gt, device, acc):
        """gt: path / dict / object with `.dataset`.  Indexes the images and categories; the class goes on with its own ingestion and ends
        with `_ingest_annotations`."""
        if isinstance(gt, (str, os.PathLike)):
            with open(gt) as f:
                gt = json.load(f)
        self._ds = gt if isinstance(gt, dict) else gt.dataset
        self.device = torch.device(device)
        self.acc = acc
        self._tie_overflow = None
        self.results = OrderedDict()
        self.eval = {}
        self.iou_thrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        self._imgs, self._cats = {}, {}
        for img in self._ds["images"]:                 # LVIS._create_index / COCO.createIndex: the last image of an id wins
            self._imgs[img["id"]] = img
        for c in self._ds["categories"]:
            self._cats[c["id"]] = c
        self._img_ids = _ids(sorted(self._imgs), "images.id")
        self._cat_ids = _ids(sorted(self._cats), "categories.id")
        self.K = len(self._cat_ids)
        self._img_pos = {int(i): n for n, i in enumerate(self._img_ids)}
        self._cat_pos = {int(c): n for n, c in enumerate(self._cat_ids)}

    def _ingest_annotations(self, anns, ign_field, keep=None):
        """anns: the file's annotation list; ign_field: the annotation field behind the kernel's per-ground-truth byte; keep(area): a further
        filter.  Sets the ground-truth tensors and the kernels' tables; -> the byte on the device."""
        dev, K, img_pos, cat_pos = self.device, self.K, self._img_pos, self._cat_pos
        a_img = _ids([a["image_id"] for a in anns], "annotations.image_id")
        a_cat = _ids([a["category_id"] for a in anns], "annotations.category_id")
        a_id = np.asarray([a["id"] for a in anns], dtype=np.int64).reshape(-1)
        if len(np.unique(a_id)) != len(a_id):
            raise ValueError("annotations.id: ids must be unique")
        a_area = np.asarray([a["area"] for a in anns], dtype=np.float64).reshape(-1)
        a_box = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        a_ign = np.asarray([bool(a.get(ign_field, 0)) for a in anns], dtype=np.uint8).reshape(-1)
        # get_ann_ids / getAnnIds(img_ids, cat_ids): images of the file, categories of the file
        ok = np.array([int(i) in img_pos and int(c) in cat_pos for i, c in zip(a_img, a_cat)], dtype=bool).reshape(-1)
        if keep is not None:
            ok &= keep(a_area)
        idx = np.nonzero(ok)[0]
        key = np.array([img_pos[int(a_img[j])] * K + cat_pos[int(a_cat[j])] for j in idx], dtype=np.int64)
        o = np.argsort(key, kind="stable")                  # per pair in annotation-file order
        idx, key = idx[o], key[o]
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)       # noqa: E731
        self.gt_key = t(key, torch.int64)
        self.gt_box = t(a_box[idx].reshape(-1, 4), torch.float64)
        self.gt_area = t(a_area[idx], torch.float64)
        self.gt_nz = t(a_id[idx] != 0, torch.uint8)
        self.img_ids_f = t(self._img_ids.astype(np.float64), torch.float64)
        self.cat_ids_f = t(self._cat_ids.astype(np.float64), torch.float64)
        self.area_rng_t = t(np.asarray(_AREA_RNG, np.float64), torch.float64)
        self.iou_thr_t = t(self.iou_thrs, torch.float64)
        self.rec_thr_t = t(self.rec_thrs, torch.float64)
        del self._ds                                        # only held between the two steps of the constructor
        return t(a_ign[idx], torch.uint8)

    def tie_overflow(self):
        """Whether a forward that came through `update_packed` had more detections tied with the DETECTIONS_PER_IMG-th score than tie slots
        (`last_tie_overflow` of the BoxList path).  One host sync."""
        return self._tie_overflow is not None and bool(self._tie_overflow.item())

    def _pairs(self, dkey):
        """Sorted pair keys of the kept detections -> (pkey: every (image, category) pair with a gt or a detection, pair_dt, pair_gt
        [P, 2] int32 = (first, count) of the pair's detections / ground truths)."""
        pkey = torch.unique(torch.cat([self.gt_key, dkey]))
        ds, de = torch.searchsorted(dkey, pkey), torch.searchsorted(dkey, pkey, right=True)
        gs, ge = torch.searchsorted(self.gt_key, pkey), torch.searchsorted(self.gt_key, pkey, right=True)
        return pkey, torch.stack([ds, de - ds], 1).to(torch.int32).contiguous(), torch.stack([gs, ge - gs], 1).to(torch.int32).contiguous()

    def _by_category(self, rows, dkey, pkey, gt_count):
        """After the match -> (num_gt [K, 4] int64, accumulate's order per category: score descending, ties by image id, then by the
        position in the pair, int32; cat_off [K + 1] int32)."""
        K, dev = self.K, self.device
        num_gt = torch.zeros(K, 4, dtype=torch.int64, device=dev)
        if K:
            num_gt.index_add_(0, pkey % K, gt_count.long())
        dcat = dkey % K if K else dkey
        o = torch.sort(rows[:, 2], descending=True, stable=True)[1]
        o = o[torch.sort(dcat[o], stable=True)[1]]
        cat_off = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        cat_off[1:] = torch.cumsum(torch.bincount(dcat, minlength=K)[:K], 0)
        return num_gt, o.to(torch.int32), cat_off.to(torch.int32)


class LvisFixedAPEvaluator(_APEvaluator):
    """Drop-in for the reference's `LvisEvaluatorFixedAP` (data/datasets/evaluation/lvis/lvis_eval.py:766-875) on the default
    `DATASETS.LVIS_USE_NORMAL_AP = False` path of engine/inference.py `build_lvis_evaluator`: the per-category top-k rows stay in a
    `FixedAPAccumulator`, and `summarize()` runs `_summarize_fixed` (LVISResults(max_dets=-1) + LVISEval(iou_type="bbox"), params.max_dets = -1)
    on the device: grouping with torch sorts, matching and accumulation in csrc/ap_eval.hip, the summary means in torch; one host sync.

    gt: the reference's LVIS object (only `.dataset` is read), a dict in LVIS json format, or a path to such a json."""

    def __init__(self, gt, topk=10000, device="cuda"):
        self.topk = int(topk)
        super().__init__(gt, device, FixedAPAccumulator(self.topk, device))
        dev, K = self.device, self.K
        self.freq_groups = [[] for _ in _FREQ_LBL]
        for n, c in enumerate(self._cat_ids):
            self.freq_groups[_FREQ_LBL.index(self._cats[int(c)]["frequency"])].append(n)
        self.freq_t = [torch.tensor(g, dtype=torch.int64).to(dev) for g in self.freq_groups]

        def pair_keys(field):
            keys = []
            for i in self._img_ids:
                lst = self._imgs[int(i)].get(field, [])
                cs = _ids(lst, f"images.{field}")
                keys.extend(self._img_pos[int(i)] * K + self._cat_pos[int(c)] for c in cs if int(c) in self._cat_pos)
            return torch.tensor(sorted(set(keys)), dtype=torch.int64).to(dev)
        self.neg_keys, self.nel_keys = pair_keys("neg_category_ids"), pair_keys("not_exhaustive_category_ids")
        # get_ann_ids: 0 < area < inf
        self.gt_ign = self._ingest_annotations(self._ds["annotations"], "ignore", keep=lambda area: (area > 0) & (area < np.inf))

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

    def update_packed(self, packed, counts, image_ids, input_sizes, orig_sizes, n_chunks, candidate=False):
        """One launch group of `forward_chunks_packed` -- packed [g * B, K2, 6], the RAW counts [g * B] int32 on the device, items chunk-major
        -- for the B images `image_ids` (original ids) and g = `n_chunks` chunks; input_sizes / orig_sizes: per image (height, width) of the
        network input (`images.image_sizes`) and of the original image (the target's `orig_size`), host numbers.  The rows are those of
        `update([(id, {...}) for every chunk])` after the engine's `resize_box` (engine/inference.py:643-648) run per image, image by image,
        bit for bit and in the same order -- built by one launch of csrc/eval_rows.hip, without a host sync; the counts stay on the device
        until the accumulator folds.  candidate: the counts are plain numbers (TEST.USE_MULTISCALE's candidate mode)."""
        rows, state = _packed_rows(self, packed, counts, image_ids, n_chunks, candidate, cols=7,
                                   ratios=[(float(ow) / float(iw), float(oh) / float(ih)) for (ih, iw), (oh, ow) in zip(input_sizes, orig_sizes)])
        self.acc.append_block(rows, state[0])

    def synchronize_between_processes(self):
        self.acc.synchronize_between_processes()

    @staticmethod
    def write_results(lines, path):
        """`write_lvis_results` (engine/inference.py:354-366): bbox.csv from the strings of `summarize()`."""
        out = ["metric, avg "]
        for line in lines:
            out.append(" ".join(line.split(" ")[:-2]) + ", " + line.split(" ")[-1] + " ")
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")

    def save_instances_results(self, path):
        """`LvisEvaluatorFixedAP.save_instances_results` (lvis_eval.py:877-884): the kept detections as one json list, sorted by image id
        with Python's stable sort (within an image: the order of `acc.by_cat()`, categories ascending, scores descending)."""
        instances = []
        for _, inst in self.acc.by_cat().items():
            instances = instances + inst
        instances = sorted(instances, key=lambda x: x["image_id"], reverse=False)
        with open(path, "w") as f:
            json.dump(instances, f)

    def summarize(self):
        """Main process: the strings of LVISEval.print_results (max_dets = -1) and self.results; other ranks: None."""
        if _not_main_process():
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
        rows, dkey = self._rows()
        pkey, pair_dt, pair_gt = self._pairs(dkey)
        pair_nel = self._member(self.nel_keys, pkey).to(torch.uint8)
        dt_box = rows[:, 3:7].contiguous()
        dt_bits, gt_count = ops.lvis_match(pair_dt, pair_gt, pair_nel, dt_box, self.gt_box, self.gt_area, self.gt_ign, self.gt_nz,
                                           self.area_rng_t, self.iou_thr_t)
        num_gt, order, cat_off = self._by_category(rows, dkey, pkey, gt_count)
        precision, recall = ops.lvis_accumulate(cat_off, order, dt_bits, num_gt.to(torch.int32).contiguous(), self.rec_thr_t)
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
        return _masked_mean(s)

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


# ====================================================================================================== COCO AP on the device
_COCO_MAX_DETS = (1, 10, 100)
# COCOeval.summarize's twelve lines: (ap, iouThr, areaRng, maxDets)
_COCO_SPECS = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
               (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
               (0, None, "medium", 100), (0, None, "large", 100)]
_COCO_METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]          # COCOResults.METRICS["bbox"]


class _ResultRows(FixedAPAccumulator):
    """The accumulator's buffer and exchange for `results_dict`: rows [n, 8] = the seven columns + a mark that is 1 on the first row of one
    image's prediction and 0 on the others, so that the running sum of the marks numbers the predictions in arrival order -- also after the
    gather, which concatenates the ranks' rows in rank order.  Nothing is pruned: COCO keeps every detection until the per-pair cut."""

    def __init__(self, device):
        super().__init__(topk=0, device=device)
        self.rows = torch.zeros(0, 8, dtype=torch.float32, device=self.device)

    def append(self, rows):
        self._pending.append(rows)
        self._npending += len(rows)

    def _prune(self, rows):
        return rows


class CocoAPEvaluator(_APEvaluator):
    """The COCO / ODinW branch of the reference's engine/inference.py (:649-650 `results_dict.update`, :703-708 the gather, :749-763 `evaluate` ->
    data/datasets/evaluation/coco/coco_eval.py `do_coco_evaluation`: `prepare_for_coco_detection`, pycocotools `COCOeval` for iou_type bbox,
    `summarize_per_category`, `COCOResults`) with the detections kept as device rows: `update` resizes, converts and maps labels on the device,
    `synchronize_between_processes` is `FixedAPAccumulator`'s fixed-shape exchange, `summarize()` groups with torch sorts, matches and
    accumulates in csrc/ap_eval.hip and takes the twelve means in torch; one host sync.

    gt: the reference's `dataset.coco` (only `.dataset` is read), a dict in COCO json format, or a path to such a json.
    label_to_cat_id: the dataset's `contiguous_category_id_to_json_id`; default {i + 1: id} over the sorted category ids."""

    def __init__(self, gt, device="cuda", label_to_cat_id=None):
        super().__init__(gt, device, _ResultRows(device))
        self.stats = []
        self.cat_ids = [int(c) for c in self._cat_ids]           # params.catIds
        self.cat_names = [self._cats[c].get("name", str(c)) for c in sorted(self._cats)]
        self.img_size = {int(i): (img["width"], img["height"]) for i, img in sorted(self._imgs.items()) if "width" in img and "height" in img}
        self.gt_crowd = self._ingest_annotations(self._ds.get("annotations", []), "iscrowd")
        if label_to_cat_id is None:
            label_to_cat_id = {i + 1: c for i, c in enumerate(self.cat_ids)}
        labels = sorted(label_to_cat_id)
        self.lbl_keys = torch.from_numpy(_ids(labels, "label_to_cat_id")).to(self.device)
        self.lbl_vals = torch.from_numpy(_ids([label_to_cat_id[k] for k in labels], "label_to_cat_id")).float().to(self.device)
        self.lbl_keys32 = self.lbl_keys.to(torch.int32)          # (ids lie within +-2^24) the kernel's table

    # ------------------------------------------------------------------ the engine's calls
    def update(self, predictions):
        """predictions: {image id: BoxList} or an iterable of such pairs (original image ids; boxes at any size) -- `results_dict.update` and
        `prepare_for_coco_detection` in one: resize to the ground-truth image's (width, height), convert("xywh") with the legacy +1, labels
        through label_to_cat_id.  An image that arrives again replaces what it had, an empty list included (it then has no detections); a row
        of an unknown label keeps its place with a NaN category and falls out with the categories the file lacks."""
        dev = self.device
        items = predictions.items() if isinstance(predictions, dict) else predictions
        for image_id, bl in items:
            iid = float(_ids([image_id], "predictions.image_id")[0])
            n = len(bl)
            r = torch.zeros(max(n, 1), 8, dtype=torch.float32, device=dev)
            r[:, 0] = iid
            r[0, 7] = 1.0
            if n == 0:
                r[0, 1] = math.nan
                self.acc.append(r)
                continue
            size = self.img_size.get(int(iid))
            bl = bl.to(dev)
            if size is not None:                           # an image the ground truth lacks: summarize() refuses it
                bl = bl.resize(size)
            labels = bl.get_field("labels").to(dev).long()
            if len(self.lbl_keys):
                j = torch.searchsorted(self.lbl_keys, labels).clamp(max=len(self.lbl_keys) - 1)
                r[:, 1] = torch.where(self.lbl_keys[j] == labels, self.lbl_vals[j], torch.full((), math.nan, device=dev))
            else:
                r[:, 1] = math.nan
            r[:, 2] = bl.get_field("scores").to(dev).float()
            r[:, 3:7] = bl.convert("xywh").bbox
            self.acc.append(r)

    def update_packed(self, packed, counts, image_ids, input_sizes, orig_sizes=None, n_chunks=1, candidate=False):
        """One launch group of `forward_chunks_packed` -- packed [g * B, K2, 6], the RAW counts [g * B] int32 on the device, items chunk-major
        -- for the B images `image_ids` (original ids) and g = `n_chunks` chunks; input_sizes: per image (height, width) of the network input
        (`images.image_sizes`); orig_sizes is not read (the target size is the ground-truth image's, ratio 1 for an image the file lacks).
        Per image one block holding its chunks in chunk order: the rows of `update({id: cat_boxlist([chunk outputs])})`, bit for bit and in
        the same order, an image without a detection included -- built by one launch of csrc/eval_rows.hip, without a host sync."""
        ids = _ids(image_ids, "predictions.image_id")
        ratios = []
        for i, (ih, iw) in zip(ids, input_sizes):
            size = self.img_size.get(int(i))
            ratios.append((1.0, 1.0) if size is None else (size[0] / float(iw), size[1] / float(ih)))
        rows, state = _packed_rows(self, packed, counts, image_ids, n_chunks, candidate, cols=8, ratios=ratios, plus_one=True, placeholder=True,
                                   lbl_keys=self.lbl_keys32, lbl_vals=self.lbl_vals)
        self.acc.append_block(rows, state[0])

    def synchronize_between_processes(self, group=None, force=False):
        self.acc.synchronize_between_processes(group, force)

    # ------------------------------------------------------------------ evaluate + accumulate
    def _rows(self):
        """-> (rows, pair key, rank in the pair, unknown-image flag): per image the prediction that arrived last, the detections COCOeval._prepare
        keeps (categories of the file), sorted by pair and within a pair by score (ties in results order), cut to maxDets[-1] per pair."""
        acc, dev, K = self.acc, self.device, self.K
        acc._fold()
        rows = acc.rows
        NI = len(self.img_ids_f)
        img, cat = rows[:, 0].double(), rows[:, 1].double()
        real = ~torch.isnan(cat)
        known = torch.zeros(len(rows), dtype=torch.bool, device=dev)
        ii = torch.zeros(len(rows), dtype=torch.int64, device=dev)
        if NI:
            ii = torch.searchsorted(self.img_ids_f, img).clamp(max=NI - 1)
            known = self.img_ids_f[ii] == img
        unknown = (real & ~known).any()                    # loadRes: results' image ids must be a subset of the ground truth's
        block = torch.cumsum((rows[:, 7] > 0).long(), 0)
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        last = torch.zeros(max(NI, 1), dtype=torch.int64, device=dev)
        last.scatter_reduce_(0, torch.where(known, ii, zero), torch.where(known, block, zero), "amax", include_self=True)
        ok = known & real & (block == last[ii])
        ci = torch.zeros(len(rows), dtype=torch.int64, device=dev)
        if K:
            ci = torch.searchsorted(self.cat_ids_f, torch.where(real, cat, torch.zeros((), dtype=torch.float64, device=dev))).clamp(max=K - 1)
            ok &= self.cat_ids_f[ci] == cat
        else:
            ok &= False
        key = ii * K + ci
        rows, key = rows[ok], key[ok]
        o = torch.sort(rows[:, 2], descending=True, stable=True)[1]
        o = o[torch.sort(key[o], stable=True)[1]]
        rows, key = rows[o], key[o]
        ar = torch.arange(len(rows), device=dev)
        first = torch.ones(len(rows), dtype=torch.bool, device=dev)
        first[1:] = key[1:] != key[:-1]
        rank = ar - torch.cummax(torch.where(first, ar, torch.zeros((), dtype=torch.int64, device=dev)), 0)[0] if len(rows) else ar
        keep = rank < _COCO_MAX_DETS[-1]
        return rows[keep], key[keep], rank[keep], unknown

    def evaluate(self):
        """-> (precision [10, 101, K, 4, 3], recall [10, K, 4, 3]) fp64 on the device, as COCOeval.accumulate lays them out; also kept in
        self.eval with the per-detection match bits (test hooks)."""
        from . import ops
        rows, dkey, rank, unknown = self._rows()
        pkey, pair_dt, pair_gt = self._pairs(dkey)
        dt_box = rows[:, 3:7].contiguous()
        dt_bits, gt_count = ops.coco_match(pair_dt, pair_gt, dt_box, self.gt_box, self.gt_area, self.gt_crowd, self.gt_nz, self.area_rng_t,
                                           self.iou_thr_t)
        num_gt, order, cat_off = self._by_category(rows, dkey, pkey, gt_count)
        precision, recall = ops.coco_accumulate(cat_off, order, rank.to(torch.int32).contiguous(), dt_bits, num_gt.to(torch.int32).contiguous(),
                                                self.rec_thr_t)
        self.eval = {"precision": precision, "recall": recall, "pair_key": pkey, "pair_dt": pair_dt, "pair_gt": pair_gt, "dt_bits": dt_bits,
                     "gt_count": gt_count, "num_gt": num_gt, "rows": rows, "rank": rank, "unknown_images": unknown}
        return precision, recall

    # ------------------------------------------------------------------ summary (COCOeval.summarize, COCOResults.update)
    def _mean(self, s, iou_thr, area, max_det):
        if iou_thr is not None:
            s = s[torch.as_tensor(np.where(iou_thr == self.iou_thrs)[0], device=s.device)]
        s = s[..., _AREA_LBL.index(area), _COCO_MAX_DETS.index(max_det)]
        return _masked_mean(s)

    def summarize(self):
        """Main process: the twelve lines COCOeval.summarize prints, self.stats and self.results["bbox"]; other ranks: None."""
        if _not_main_process():
            return None
        precision, recall = self.evaluate()
        vals = [self._mean(precision if ap else recall, thr, area, md) for ap, thr, area, md in _COCO_SPECS]
        vals = torch.stack(vals + [self.eval["unknown_images"].double()]).cpu().tolist()          # the one host sync
        if vals[-1]:
            raise ValueError("Results do not correspond to current coco set: predictions of image ids the ground truth does not hold")
        self.stats = [float(v) for v in vals[:-1]]
        self.results = OrderedDict([("bbox", OrderedDict(zip(_COCO_METRICS, self.stats)))])
        template = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
        out = []
        for (ap, thr, area, md), v in zip(_COCO_SPECS, self.stats):
            iou = "{:0.2f}:{:0.2f}".format(self.iou_thrs[0], self.iou_thrs[-1]) if thr is None else "{:0.2f}".format(thr)
            line = template.format("Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, md, v)
            print(line)
            out.append(line)
        return out

    def per_category(self, csv_output=None):
        """Main process: the lines of the reference's `summarize_per_category` (title, then AP / AP50 / APs / APm / APl at maxDets 100: the
        per-category `np.mean` over thresholds and recall points, -1 entries included), also written to `csv_output` when given; other
        ranks: None.  Not a hot path: the precision array comes to the host and numpy takes the means, so that the digits are numpy's."""
        if _not_main_process():
            return None
        if "precision" not in self.eval:
            self.evaluate()
        precision = self.eval["precision"].cpu().numpy()
        mind = [len(_COCO_MAX_DETS) - 1]

        def line(iou_thr=None, area="all"):
            iou = "{:0.2f}:{:0.2f}".format(self.iou_thrs[0], self.iou_thrs[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
            text = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ], ".format("Average Precision", "(AP)", iou, area, _COCO_MAX_DETS[-1])
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == self.iou_thrs)[0]]
            s = s[:, :, :, [_AREA_LBL.index(area)], mind]
            if len(s[s > -1]) == 0:
                return text
            avg = 0.0
            for k in range(self.K):
                text += "{}, ".format(np.mean(s[:, :, k, :]))
                avg += np.mean(s[:, :, k, :])
            return text + "{} \n".format(avg / self.K)
        out = ["metric, " + "".join("{}, ".format(n) for n in self.cat_names) + "avg \n", line(), line(iou_thr=.5), line(area="small"),
               line(area="medium"), line(area="large")]
        if csv_output is not None:
            with open(csv_output, "w") as f:
                for text in out:
                    f.writelines(text)
        return out


# ====================================================================================================== Flickr30k Entities Recall@k on the device
_FLICKR_PHRASE = re.compile(r"\[/EN#([^/\s\]]+)((?:/[^/\s\]]*)*)\s")


def read_entities_sentences(path):
    """One `Sentences/<image>.txt` of Flickr30k Entities: a caption per non-empty line, an annotated phrase written `[/EN#<id>/<type>/<type> words]`
    (zero or more types) -> per caption the list of {"phrase_id", "phrase_type": [...]} in reading order."""
    with open(path) as f:
        lines = [ln for ln in f.read().split("\n") if ln.strip()]
    return [[{"phrase_id": m.group(1), "phrase_type": [t for t in m.group(2).split("/")[1:]]} for m in _FLICKR_PHRASE.finditer(ln + " ")]
            for ln in lines]


def read_entities_boxes(path):
    """One `Annotations/<image>.xml` of Flickr30k Entities: every <object> names one or more phrase ids (<name>) and either carries a <bndbox>
    (xmin, ymin, xmax, ymax) or a <nobndbox> / <scene> mark -> {phrase id: [[x1, y1, x2, y2], ...]} of the ids with boxes, in file order."""
    import xml.etree.ElementTree as ET
    boxes = {}
    for obj in ET.parse(path).getroot().iter("object"):
        bb = obj.find("bndbox")
        if bb is None:
            continue
        box = [int(bb.findtext(tag)) for tag in ("xmin", "ymin", "xmax", "ymax")]
        for name in obj.findall("name"):
            boxes.setdefault(name.text, []).append(list(box))
    return boxes


class FlickrRecallEvaluator:
    """The phrase-grounding branch of the reference's engine/inference.py (`TEST.EVAL_TASK = "grounding"`: `flickr_post_process` :322-338, the
    evaluator calls :701-724) and data/datasets/evaluation/flickr/flickr_eval.py (`FlickrEvaluator`, `Flickr30kEntitiesRecallEvaluator`,
    `RecallTracker`) with the detections kept as fp32 device rows.  `update_boxlist` is resize_box + flickr_post_process without a host sync,
    `update` takes the reference's post-processed dicts, `synchronize_between_processes` is `FixedAPAccumulator`'s fixed-shape exchange,
    `summarize()` groups with torch sorts, runs csrc/flickr_eval.hip and returns the reference's `score` dict after one host sync.

    gt: {image id: [sentence, ...]}, a sentence being a list of phrases {"phrase_id", "phrase_type": [...]} or None (not evaluated);
    boxes: {image id: {phrase id: [[x1, y1, x2, y2], ...]}}.  Phrases without boxes are dropped and a sentence that keeps none is not
    evaluated, as in flickr_eval.py:305-318.  Rows [n, 8] fp32: a prediction is one header row (sentence slot, number of phrase lists, -1,
    0.., mark 1) followed by its detections (sentence slot, phrase, score, x1, y1, x2, y2, mark 0); the running sum of the marks is the
    arrival number, also after the gather.

    Rules (flickr_eval.py:323-390): the first prediction of a sentence wins, later ones are dropped with a warning; predictions for a
    sentence that is not evaluated are ignored; a wrong number of phrase lists, a phrase index outside the sentence, a missing prediction
    raise RuntimeError in `summarize()`.  An unknown image id or a sentence id outside the image's list raises RuntimeError in `update*`
    (the reference's two checks of that kind come after its `all_ids` filter and are never reached; here they are).  Within a phrase the
    order is score descending, ties in detection order (`torch.topk` leaves the order of ties open)."""

    def __init__(self, gt, boxes=None, topk=(1, 5, 10, -1), iou_thresh=0.5, merge_boxes=False, device="cuda"):
        if boxes is None:
            gt, boxes = gt
        self.device = torch.device(device)
        self.topk = tuple(int(k) for k in topk)
        if not self.topk or len(self.topk) > 30 or any(k == 0 or k < -1 for k in self.topk):
            raise ValueError("topk: 1 to 30 values, each > 0 or -1 (all)")
        self.iou_thresh = float(iou_thresh)
        self.acc = _ResultRows(self.device)
        self.results = None
        self.eval = {}
        self._ingest(gt, boxes, merge_boxes)

    @classmethod
    def from_entities_dir(cls, path, subset="test", merge_boxes=False, **kw):
        """The Flickr30k Entities layout: `<subset>.txt` (an image id per line), `Annotations/<id>.xml`, `Sentences/<id>.txt`."""
        with open(os.path.join(path, f"{subset}.txt")) as f:
            ids = [ln.strip() for ln in f]
        gt = OrderedDict((i, read_entities_sentences(os.path.join(path, "Sentences", f"{i}.txt"))) for i in ids)
        boxes = {i: read_entities_boxes(os.path.join(path, "Annotations", f"{i}.xml")) for i in ids}
        return cls(gt, boxes, merge_boxes=merge_boxes, **kw)

    # ------------------------------------------------------------------ ground truth, once
    def _ingest(self, gt, boxes, merge_boxes):
        dev = self.device
        self.sentences, self.gt_boxes = OrderedDict(), {}
        self.slot = {}                                           # (image id, sentence id) -> slot of an evaluated sentence
        self.slot_name = []
        ph_off, phrase_gt, gt_box, cat_off, cat_idx = [0], [], [], [0], []
        boxes = {str(k): v for k, v in boxes.items()}
        kept_types = set()
        for img, sents in gt.items():
            img = str(img)
            bx = {}
            for pid, bl in boxes.get(img, {}).items():
                b = np.asarray(bl, dtype=np.float64).reshape(-1, 4)
                if merge_boxes and len(b) > 1:
                    b = np.array([[b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()]])
                bx[str(pid)] = b
            self.gt_boxes[img] = {k: v.tolist() for k, v in bx.items()}
            out = []
            for s in sents:
                kept = [{"phrase_id": str(p["phrase_id"]), "phrase_type": list(p["phrase_type"])} for p in (s or []) if str(p["phrase_id"]) in bx]
                out.append(kept if kept else None)
                for p in kept:
                    kept_types.update(p["phrase_type"])
            self.sentences[img] = out
        self.categories = ["all"] + sorted(kept_types - {"all"})
        col = {c: n for n, c in enumerate(self.categories)}
        for img, sents in self.sentences.items():
            for sid, s in enumerate(sents):
                if s is None:
                    continue
                self.slot[(img, sid)] = len(self.slot_name)
                self.slot_name.append((img, sid))
                for p in s:
                    b = np.asarray(self.gt_boxes[img][p["phrase_id"]], dtype=np.float64).reshape(-1, 4)
                    phrase_gt.append((len(gt_box), len(b)))
                    gt_box.extend(b.tolist())
                    cat_idx.extend(col[t] for t in p["phrase_type"])
                    cat_off.append(len(cat_idx))
                ph_off.append(len(phrase_gt))
        if len(self.slot_name) >= _ID_LIMIT:
            raise ValueError("more than 2^24 evaluated sentences (the rows keep the sentence slot as fp32)")
        t = lambda a, dt, shape: torch.tensor(a, dtype=dt).reshape(shape).to(dev)          # noqa: E731
        self.S, self.P = len(self.slot_name), len(phrase_gt)
        self.ph_off = t(ph_off, torch.int64, (-1,))
        self.phrase_gt = t(phrase_gt, torch.int32, (-1, 2)).contiguous()
        self.gt_box = t(gt_box, torch.float64, (-1, 4)).contiguous()
        self.cat_off = t(cat_off, torch.int32, (-1,))
        self.cat_idx = t(cat_idx, torch.int32, (-1,))
        self.ks = t(list(self.topk), torch.int32, (-1,))
        self.iou_thr_t = t([self.iou_thresh], torch.float64, (-1,))

    # ------------------------------------------------------------------ the engine's calls
    def _slot_of(self, image_id, sentence_id):
        """-> slot, or None for a sentence that is not evaluated; RuntimeError for ids the ground truth does not hold"""
        img = str(int(image_id)) if torch.is_tensor(image_id) else str(image_id)
        if img not in self.sentences:
            raise RuntimeError(f"Unknown image id {img}")
        sid = int(sentence_id)
        if not 0 <= sid < len(self.sentences[img]):
            raise RuntimeError(f"Unknown sentence id {sid} in image {img}")
        return self.slot.get((img, sid))

    def _header(self, slot, n_lists, n_rows):
        r = torch.zeros(1 + n_rows, 8, dtype=torch.float32, device=self.device)
        r[:, 0] = float(slot)
        r[0, 1], r[0, 2], r[0, 7] = float(n_lists), -1.0, 1.0
        return r

    def update(self, predictions):
        """predictions: the reference's `mdetr_style_output`, [{"image_id", "sentence_id", "boxes": per phrase a list of [x1, y1, x2, y2] in
        the order to evaluate them (flickr_post_process: score descending, the dummy box last), "scores"}] -- `FlickrEvaluator.update`.  The
        lists' own order is kept (the rows' score is minus the position); the dummy box the kernel implies behind every list repeats the
        one the list ends with, which changes no prefix maximum."""
        for pred in predictions:
            slot = self._slot_of(pred["image_id"], pred["sentence_id"])
            if slot is None:
                if any(len(b) for b in pred["boxes"]):
                    warnings.warn(f"in image {pred['image_id']} no predictions were expected for sentence {pred['sentence_id']}: ignored")
                continue
            lists = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in pred["boxes"]]
            n = sum(len(b) for b in lists)
            if len(lists) >= _ID_LIMIT:
                raise ValueError("more than 2^24 phrase lists in one prediction")
            r = self._header(slot, len(lists), n)
            if n:
                body = np.zeros((n, 6), dtype=np.float32)
                body[:, 0] = np.concatenate([np.full(len(b), j) for j, b in enumerate(lists)])
                body[:, 1] = np.concatenate([-np.arange(len(b)) for b in lists])
                body[:, 2:] = np.concatenate(lists)
                r[1:, 1:7] = torch.from_numpy(body).to(self.device)
            self.acc.append(r)

    def update_boxlist(self, image_id, sentence_id, boxlist, n_phrases, plus=0, orig_size=None):
        """One raw output of the model -> rows, on the device and without a host sync: `resize_box` (to orig_size = (height, width), host
        numbers or a host tensor; None = keep the size) and `flickr_post_process` (phrase = label - plus; the per-phrase lists and their order
        are made in `summarize()`)."""
        slot = self._slot_of(image_id, sentence_id)
        if slot is None:
            return
        bl = boxlist.to(self.device)
        if orig_size is not None:
            h, w = (float(v) for v in orig_size)
            bl = bl.resize((w, h))
        n = len(bl)
        r = self._header(slot, int(n_phrases), n)
        if n:
            r[1:, 1] = (bl.get_field("labels").to(self.device) - int(plus)).float()
            r[1:, 2] = bl.get_field("scores").to(self.device).float()
            r[1:, 3:7] = bl.convert("xyxy").bbox.float()
        self.acc.append(r)

    def accumulate(self):
        pass

    def synchronize_between_processes(self, group=None, force=False):
        self.acc.synchronize_between_processes(group, force)

    # ------------------------------------------------------------------ evaluate
    def evaluate(self):
        """-> (positives [K, C] int64, totals [C] int64, flags [4] int64: predictions dropped as duplicates, evaluated sentences without a
        prediction, winners with a wrong number of phrase lists, detections with a phrase index outside their sentence) on the device;
        the per-phrase hit bits are kept in self.eval (test hook)."""
        from . import ops
        acc, dev, S = self.acc, self.device, self.S
        acc._fold()
        rows = acc.rows
        n = len(rows)
        i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)                   # noqa: E731
        head = rows[:, 7] > 0
        slot = rows[:, 0].long().clamp(0, max(S - 1, 0))
        pred_no = torch.cumsum(head.long(), 0)                   # arrival number of the prediction a row belongs to, from 1
        big = torch.full((), n + 1, dtype=torch.int64, device=dev)
        first = torch.full((max(S, 1),), n + 1, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, slot, torch.where(head, pred_no, big), "amin", include_self=True)
        win = pred_no == first[slot]
        dropped = (head & ~win).sum()
        missing = (first[:S] > n).sum()
        want = self.ph_off[1:] - self.ph_off[:-1]                # phrases per slot
        bad_len = (head & win & (rows[:, 1].long() != want[slot])).sum() if S else i64(0)[0]
        det = ~head & win
        ph = rows[:, 1].long()
        inside = (ph >= 0) & (ph < want[slot]) if S else det
        bad_phrase = (det & ~inside).sum()
        det &= inside
        d = rows[det]
        gp = (self.ph_off[:-1][slot[det]] + ph[det]) if S else ph[det]
        o = torch.sort(d[:, 2], descending=True, stable=True)[1]                          # ties: detection order
        o = o[torch.sort(gp[o], stable=True)[1]]
        d, gp = d[o], gp[o]
        pid = torch.arange(self.P, device=dev)
        ds = torch.searchsorted(gp, pid)
        de = torch.searchsorted(gp, pid, right=True)
        phrase_dt = torch.stack([ds, de - ds], 1).to(torch.int32).contiguous()
        dt_box = d[:, 3:7].contiguous()
        hits = ops.flickr_recall(phrase_dt, self.phrase_gt, dt_box, self.gt_box, self.ks, self.iou_thr_t)
        positives, totals = ops.flickr_tally(hits, self.cat_off, self.cat_idx, len(self.topk), len(self.categories))
        flags = torch.stack([dropped, missing, bad_len, bad_phrase])
        self.eval = {"hits": hits, "phrase_dt": phrase_dt, "dt_box": dt_box, "positives": positives, "totals": totals, "flags": flags,
                     "first": first}
        return positives, totals, flags

    def summarize(self):
        """FlickrEvaluator.summarize's `score`: {"Recall@1_all": .., .., "Upper_bound_<type>": ..}, k in topk order, categories sorted, values
        positives / total as Python floats -- on every rank (after the exchange every rank holds all rows)."""
        positives, totals, flags = self.evaluate()
        K, C = positives.shape
        vals = torch.cat([positives.reshape(-1), totals, flags]).cpu().tolist()           # the one host sync
        pos, tot, (dropped, missing, bad_len, bad_phrase) = vals[:K * C], vals[K * C:K * C + C], vals[K * C + C:]
        if dropped:
            warnings.warn(f"multiple predictions found for {dropped} sentence prediction(s): the first one of a sentence counts")
        if bad_len or bad_phrase:
            raise RuntimeError(f"Error, {bad_len} prediction(s) with a number of phrase lists other than the sentence's number of phrases, "
                               f"{bad_phrase} detection(s) with a phrase index outside their sentence")
        if missing:
            first = self.eval["first"][:self.S].cpu().tolist()
            lost = [self.slot_name[s] for s, f in enumerate(first) if f > len(self.acc.rows)]
            raise RuntimeError("Missing predictions: " + ", ".join(f"sentence {sid} in image {img}" for img, sid in lost[:20])
                               + (" ..." if len(lost) > 20 else ""))
        self.results = OrderedDict()
        score = {}
        order = [c for c in sorted(range(C), key=lambda c: self.categories[c]) if tot[c] > 0]     # "all" sorts among the types
        for j, k in enumerate(self.topk):
            header = "Upper_bound" if k == -1 else f"Recall@{k}"
            self.results[k] = {self.categories[c]: pos[j * C + c] / tot[c] for c in order}
            for c in order:
                score[f"{header}_{self.categories[c]}"] = pos[j * C + c] / tot[c]
        return score

    @staticmethod
    def write_results(score, path):
        """`write_flickr_results` (engine/inference.py:368-381): bbox.csv."""
        lines = ["metric, avg "] + [f"{name}, {value} " for name, value in score.items()]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
