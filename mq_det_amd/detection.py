"""Detection evaluation: the `TEST.EVAL_TASK = "detection"` branch of the reference's `inference()` (engine/inference.py:577-733: the loop over
the chunk captions, `resize_box`, the evaluator calls, bbox.csv) for the LVIS Fixed AP and the COCO / ODinW evaluators of this package.

Batches are `(images, targets, image_ids, ...)`.  For `LvisFixedAPEvaluator` a target is a dict with "image_id" and "orig_size" ((height,
width)) or a BoxList with such fields, and the original id is the target's "image_id"; for `CocoAPEvaluator` the original id is
`data_loader.dataset.id_to_img_map[image_id]` where the loader's dataset has that map, else `image_id`, and the boxes are resized to the
ground-truth file's image size.

Three paths lead from the model to the evaluator:
  * packed (`forward_chunks_packed` -> `update_packed`): the detections never leave the device and the host waits for nothing per image --
    csrc/eval_rows.hip turns a forward's packed detections into evaluator rows in one launch, the counts are read when the accumulator folds;
  * BoxLists (`forward_chunks`, or one `model(...)` per chunk for a model without it -> `update`): the path INTEGRATION.md spells out by hand;
  * TEST.USE_MULTISCALE: one `tta.im_detect_bbox_aug` per batch with the LAST chunk's caption and map, as the reference does (:588-600).
All three leave the same rows (tests/detection_eval_checks.py).

Difference by design: the reference's LVIS branch reads `output[0]` / `targets[0]` only and so needs TEST.IMS_PER_BATCH = 1; here a batch of
any size gives the rows of the batch-1 run over the same image order.  Not here: DATASETS.LVIS_USE_NORMAL_AP, MQ-GroundingDINO on the packed
path (it takes one `model(...)` per chunk), the visualizer, VISION_QUERY.RETURN_ATTN_GATE_VALUE."""
import warnings

import torch

from .evaluation import CocoAPEvaluator, LvisFixedAPEvaluator
from .structures import cat_boxlist, to_image_list

TIE_OVERFLOW_WARNING = ("image(s) had more detections tied with the DETECTIONS_PER_IMG-th score than MODEL.ATSS.TIE_SLOTS output slots: the "
                        "reference would return all of them (rpn/inference.py:757-766)")


def _field(target, name):
    return target[name] if isinstance(target, dict) else target.get_field(name)


def _has(target, name):
    return name in target if isinstance(target, dict) else target.has_field(name)


def _orig_ids(evaluator, data_loader, targets, image_ids):
    if isinstance(evaluator, LvisFixedAPEvaluator):
        return [int(_field(t, "image_id")) if _has(t, "image_id") else int(i) for t, i in zip(targets, image_ids)]
    id_map = getattr(getattr(data_loader, "dataset", None), "id_to_img_map", None)
    return [int(i) if id_map is None else int(id_map[int(i)]) for i in image_ids]


def _orig_sizes(targets):
    return [tuple(float(v) for v in _field(t, "orig_size")) for t in targets]            # (height, width)


def _update_boxlists(evaluator, ids, targets, per_image):
    """per_image[b] = the BoxLists of image b, one per chunk (one in all under TEST.USE_MULTISCALE) -> the evaluator's `update`."""
    if isinstance(evaluator, LvisFixedAPEvaluator):
        out = []
        for i, (h, w), bls in zip(ids, _orig_sizes(targets), per_image):
            for bl in bls:                                     # resize_box + the tuple of :643-648
                bl = bl.resize((w, h))
                out.append((i, {"scores": bl.get_field("scores"), "labels": bl.get_field("labels"), "boxes": bl.bbox}))
        evaluator.update(out)
    else:
        evaluator.update([(i, cat_boxlist(bls)) for i, bls in zip(ids, per_image)])


@torch.no_grad()
def evaluate_detection(model, data_loader, evaluator, queries_and_maps, device="cuda", output_file=None, max_items=32, packed="auto"):
    """-> what `evaluator.summarize()` returns (the main process: the summary lines; other ranks: None).  `queries_and_maps` =
    `(all_queries, all_positive_map_label_to_token)` of the caller's `create_queries_and_maps_from_dataset`.  packed: "auto" takes the
    packed path where the model offers it, True insists (ValueError otherwise), False takes the BoxList path.  The main process writes
    `output_file` (bbox.csv: `write_lvis_results` for the LVIS evaluator, the summary lines for the COCO one) when given, and
    TEST.LVIS_RESULTS_SAVE_PATH when set and the evaluator is the LVIS one."""
    if not isinstance(evaluator, (LvisFixedAPEvaluator, CocoAPEvaluator)):
        raise TypeError("evaluate_detection takes a LvisFixedAPEvaluator or a CocoAPEvaluator")
    if packed not in ("auto", True, False):
        raise ValueError(f"packed = {packed!r}: 'auto', True or False")
    cfg = model.cfg
    if cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE:
        raise NotImplementedError("evaluate_detection with VISION_QUERY.RETURN_ATTN_GATE_VALUE (a diagnostic of the reference's loop)")
    device = torch.device(device)
    all_queries, all_maps = queries_and_maps
    chunks = list(zip(all_queries, all_maps))
    multiscale = bool(cfg.TEST.get("USE_MULTISCALE", False))
    can_pack = hasattr(model, "forward_chunks_packed") and not multiscale
    if packed is True and not can_pack:
        raise ValueError("packed=True: " + ("TEST.USE_MULTISCALE takes the test-time-augmentation path" if multiscale else
                                            f"{type(model).__name__} has no forward_chunks_packed"))
    subset = cfg.TEST.get("SUBSET", -1)
    used_packed = False
    model.eval()
    for i, batch in enumerate(data_loader):
        if i == subset:
            break
        images, targets, image_ids, *_ = batch
        ids = _orig_ids(evaluator, data_loader, targets, image_ids)
        if multiscale:
            from . import tta
            caption, positive_map = chunks[-1]
            out = tta.im_detect_bbox_aug(model, images, device, [caption] * len(targets), positive_map)
            _update_boxlists(evaluator, ids, targets, [[o] for o in out])
            continue
        images = to_image_list(images).to(device)
        groups = model.forward_chunks_packed(images, chunks, max_items) if can_pack and packed is not False else None
        if groups is not None:
            used_packed = True
            sizes = _orig_sizes(targets) if isinstance(evaluator, LvisFixedAPEvaluator) else None
            if len(groups) == 1 or isinstance(evaluator, LvisFixedAPEvaluator) and len(ids) == 1:
                for pk, counts, g in groups:
                    evaluator.update_packed(pk, counts, ids, images.image_sizes, sizes, g)
            else:
                # the chunks of an image lie in several launch groups, and an image's rows are one run (LVIS: the batch-1 order; COCO: one
                # block per image): one table over all groups -- the packed tensors are concatenated on the device, nothing is read
                evaluator.update_packed(torch.cat([pk for pk, _, _ in groups]), torch.cat([c for _, c, _ in groups]), ids,
                                        images.image_sizes, sizes, sum(g for _, _, g in groups))
            continue
        if packed is True:
            raise ValueError("packed=True: the model's forward_chunks_packed declined (0 < VISION_QUERY.TEXT_DROPOUT < 1 draws a mask per item)")
        if hasattr(model, "forward_chunks"):
            per_chunk = model.forward_chunks(images, chunks, max_items)
        else:
            per_chunk = []
            for caption, positive_map in chunks:
                out = model(images, captions=[caption] * len(targets), positive_map=positive_map)
                per_chunk.append(out[0] if isinstance(out, tuple) else out)
        _update_boxlists(evaluator, ids, targets, [[chunk[b] for chunk in per_chunk] for b in range(len(ids))])
    evaluator.synchronize_between_processes()
    score = evaluator.summarize()
    if used_packed and evaluator.tie_overflow():               # the one read of the flag the row kernel ORs on the device
        warnings.warn(TIE_OVERFLOW_WARNING)
    main = not (torch.distributed.is_available() and torch.distributed.is_initialized()) or torch.distributed.get_rank() == 0
    if main and score is not None:
        lvis = isinstance(evaluator, LvisFixedAPEvaluator)
        if output_file is not None:
            if lvis:
                evaluator.write_results(score, output_file)
            else:
                with open(output_file, "w") as f:
                    f.write("\n".join(score) + "\n")
        if lvis and cfg.TEST.get("LVIS_RESULTS_SAVE_PATH", ""):
            evaluator.save_instances_results(cfg.TEST.LVIS_RESULTS_SAVE_PATH)
    return score
