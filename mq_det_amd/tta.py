"""Test-time augmentation: the TEST.USE_MULTISCALE evaluation path of the reference, on the device.

`im_detect_bbox_aug(model, images, device, captions, positive_map_label_to_token)` is the drop-in for
maskrcnn_benchmark/data/datasets/evaluation/box_aug.py:12-63 with SPECIAL_NMS = 'none':
  * the images are uploaded ONCE as uint8; every (scale, flip) canvas is made on the device by mq_tta_ingest_fwd (csrc/tta.hip), bit-exact
    to T.Resize (PIL BILINEAR) -> T.RandomHorizontalFlip(1.0) -> T.ToTensor -> T.Normalize -> to_image_list (box_aug.py:65-127);
  * one model(ImageList, captions, positive_map) per transform, 2 x len(TEST.SCALES) with TEST.FLIP;
  * the detections of all transforms are un-flipped, band-filtered, rescaled and merged (per-class NMS at TEST.TH, top TEST.PRE_NMS_TOP_N
    with ties) by mq_tta_merge_prep / mq_ml_nms / mq_tta_merge_finalize, straight from model.last_packed (box_aug.py:21-63, 150-238).
`merge` / `merge_result_from_multi_scales` also take TEST.SPECIAL_NMS = 'soft-nms', 'vote' and 'soft-vote' (mq_tta_merge_special; box_aug.py:209-349).

THE REFERENCE'S PROTOCOL is selected by model.cfg.TEST.USE_MULTISCALE = True, the switch its engine sets whenever it calls this function: the
ATSS post-processor is then built with bbox_aug_enabled and skips select_over_all_levels (rpn/inference.py:737-742, 846), so every transform
hands the merge ALL its candidates -- per level the top PRE_NMS_TOP_N scores above INFERENCE_TH, no per-class NMS, no DETECTIONS_PER_IMG cut --
and the merge is the only suppression step.  With the switch on the detector returns those candidates (pipeline.postprocess, candidate mode),
`im_detect_bbox_aug` merges up to transforms x 5 x PRE_NMS_TOP_N rows per image (mq_tta_merge_nms beyond the 16 384 rows of mq_ml_nms) and takes
all four TEST.SPECIAL_NMS modes.  With the switch off (the configuration default) every transform contributes its NMS'ed top
(DETECTIONS_PER_IMG + TIE_SLOTS) rows instead -- cheaper, and NOT the reference's result: NMS-then-merge-NMS drops candidates the merge alone
would have kept -- and `im_detect_bbox_aug` refuses the special modes (check_supported).
The forwards run eagerly: the default scales give 12 canvas shapes per batch, more than MODEL.HIP_GRAPH_CACHE keeps, so replaying graphs
would capture one per forward (USE_HIP_GRAPH below switches them back on; tools/tta_bench.py measures both).
"""
import functools
import math
import warnings

import numpy as np
import torch

from .structures import BoxList, ImageList

USE_HIP_GRAPH = False          # graphs for the TTA forwards (the model's MODEL.USE_HIP_GRAPH still has to allow them)
TIMING = None                  # a dict: filled with device-event milliseconds {"ingest", "forwards", "merge"} of the last call
_WARNED_CLASSES = False
CANDIDATE_LEVELS = 5           # FPN levels of the ATSS head: a transform returns at most CANDIDATE_LEVELS x PRE_NMS_TOP_N candidates per image


def get_size(image_size, size, max_size):
    """data/transforms/transforms.py:93-115 (Resize.get_size with one min_size): (w, h) -> (oh, ow)."""
    w, h = image_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


def input_format(cfg):
    """box_aug.py:69-72: INPUT.FORMAT when set, else 'bgr255' when INPUT.TO_BGR255 (lower-cased like T.Normalize)."""
    fmt = cfg.INPUT.get("FORMAT", "")
    if fmt != "":
        return fmt.lower()
    if cfg.INPUT.get("TO_BGR255", True):
        return "bgr255"
    raise ValueError("INPUT.FORMAT is empty and INPUT.TO_BGR255 is False: the reference's box_aug.py has no input format then")


@functools.lru_cache(maxsize=256)
def pil_coeffs(in_size, out_size):
    """PIL's uint8 BILINEAR coefficients of one axis (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc) in float64 ->
    (bounds [out, 2] int32: first input index, taps; coef [out, ksize] int32 with 22 fractional bits).  A dimension that does not change
    is a pass PIL skips: one tap of weight 1 << 22, the identity."""
    if in_size == out_size:
        return np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32), np.full((out_size, 1), 1 << 22, np.int32)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs * 1.0
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    k = np.zeros((out_size, ksize), np.float64)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                    # the C loop's order: sequential sums
        x = np.abs(((j + xmin).astype(np.float64) - center + 0.5) * ss)
        w = np.where(x < 1.0, 1.0 - x, 0.0)
        w = np.where(j < xmax, w, 0.0)
        k[:, j] = w
        ww = ww + w
    k = np.where(ww[:, None] != 0.0, k / np.where(ww == 0.0, 1.0, ww)[:, None], k)
    fixed = np.where(k < 0, np.trunc(-0.5 + k * (1 << 22)), np.trunc(0.5 + k * (1 << 22))).astype(np.int32)
    return np.stack([xmin, xmax], 1).astype(np.int32), fixed


def ingest_tables(in_hw, out_hw, TH=16, lds_bytes=64 << 10):
    """Per-image tables of mq_tta_ingest_fwd for in_hw / out_hw [(h, w)] -> (meta [B, 16], bounds, coef int32 numpy, TH, R)."""
    meta, bounds, coef, nb, nk = [], [], [], 0, 0
    ybs = []
    for (hi, wi), (ho, wo) in zip(in_hw, out_hw):
        xb, xk = pil_coeffs(wi, wo)
        yb, yk = pil_coeffs(hi, ho)
        meta.append([hi, wi, ho, wo, nb, nk, xk.shape[1], nb + wo, nk + xk.size, yk.shape[1]] + [0] * 6)
        bounds += [xb, yb]
        coef += [xk.reshape(-1), yk.reshape(-1)]
        nb, nk = nb + wo + ho, nk + xk.size + yk.size
        ybs.append(yb)

    def window(th):
        r = 1
        for yb in ybs:
            lo, hi = yb[:, 0].astype(np.int64), (yb[:, 0] + yb[:, 1]).astype(np.int64)
            n = len(lo)
            starts = np.arange(0, n, th)
            top = np.maximum.reduceat(hi, starts)
            r = max(r, int((top - lo[starts]).max()))
        return r
    R = window(TH)
    while R * 64 * 3 > lds_bytes and TH > 1:
        TH //= 2
        R = window(TH)
    return (np.asarray(meta, np.int32), np.concatenate(bounds).astype(np.int32), np.concatenate(coef).astype(np.int32), TH, R)


def _as_u8(img):
    """A PIL image (converted to RGB like the reference's loader), or an HWC uint8 tensor / array -> contiguous HWC uint8 numpy."""
    if isinstance(img, torch.Tensor):
        a = img.detach().cpu().numpy()
    elif isinstance(img, np.ndarray):
        a = img
    else:
        a = np.asarray(img.convert("RGB") if getattr(img, "mode", "RGB") != "RGB" else img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"TTA images are RGB PIL images or HWC uint8 arrays with 3 channels, got {a.dtype} {tuple(a.shape)}")
    return np.ascontiguousarray(a)


class Upload:
    """The batch's pixels on the device once: packed uint8 + per-image offsets and (h, w)."""

    def __init__(self, images, device):
        arrs = [_as_u8(im) for im in images]
        self.hw = [(a.shape[0], a.shape[1]) for a in arrs]
        offs = np.cumsum([0] + [a.size for a in arrs])
        self.src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(device)
        self.off = torch.tensor(offs[:-1], dtype=torch.int64, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)      # set by the kernel if a tile's row window exceeds the tables' R
        self.device = device


def ingest(up, scale, max_size, cfg, flip):
    """One scale of box_aug.py im_detect_bbox / im_detect_bbox_hflip -> (canvas, flipped canvas or None, image_sizes [(h, w)])."""
    from . import ops
    out_hw = [get_size((w, h), scale, max_size) for (h, w) in up.hw]
    meta, bounds, coef, TH, R = ingest_tables(up.hw, out_hw)
    d = cfg.DATALOADER.SIZE_DIVISIBILITY
    Hp, Wp = max(h for h, _ in out_hw), max(w for _, w in out_hw)
    if d > 0:
        Hp, Wp = int(math.ceil(Hp / d) * d), int(math.ceil(Wp / d) * d)
    fmt = input_format(cfg)
    dev = up.device
    t = torch.from_numpy(np.concatenate([meta.reshape(-1), bounds.reshape(-1), coef])).to(dev)
    nm, nb = meta.size, bounds.size
    plain, flipped = ops.tta_ingest(up.src, up.off, t[:nm], t[nm:nm + nb], t[nm + nb:], len(up.hw), Hp, Wp, TH, R,
                                    cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, "bgr" in fmt, "255" in fmt, flip, up.err)
    return plain, flipped, [tuple(s) for s in out_hw]


def class_list(cfg):
    """box_aug.py merge_result_from_multi_scales: SELECT_CLASSES in its given order, else range(1, NUM_CLASSES)."""
    sel = cfg.TEST.get("SELECT_CLASSES", ())
    return [int(c) for c in sel] if len(sel) else list(range(1, cfg.TEST.NUM_CLASSES))


def merge(dets, orig_wh, cfg, device, row_cap=None, stats=None, nms_path="auto"):
    """dets: per transform (packed [B, K, 6], counts [B], scaled (w, h) per image, flipped, range or None) in concatenation order ->
    list[BoxList] of box_aug.py's merge with TEST.SPECIAL_NMS 'none', 'soft-nms', 'vote' or 'soft-vote' (ops.tta_merge; the last three:
    mq_tta_merge_special, csrc/tta.hip).  row_cap / stats: ops.tta_merge (the LDS row cap of the special modes, and the count of classes
    that went through the global workspace, returned as an int in stats["workspace_classes"]).  nms_path ('none' only): "auto" = mq_ml_nms
    up to ops.TTA_MERGE_MAX_ROWS rows per image and mq_tta_merge_nms beyond, "segmented" = mq_tta_merge_nms at any size; the same rows."""
    global _WARNED_CLASSES
    from . import ops
    T, B = len(dets), len(orig_wh)
    K = max(d[0].shape[1] for d in dets)
    packed = torch.zeros(T, B, K, 6, dtype=torch.float32, device=device)
    for t, d in enumerate(dets):
        packed[t, :, :d[0].shape[1]] = d[0]
    counts = torch.tensor([d[1] for d in dets], dtype=torch.int32, device=device).reshape(T, B)
    tp = []
    for d in dets:
        for (w, h), (ws, hs) in zip(orig_wh, d[2]):
            tp.append([float(ws) if d[3] else -1.0, float(w) / float(ws), float(h) / float(hs), 0.0])   # BoxList.resize: ratios in double
    tparam = torch.tensor(tp, dtype=torch.float32, device=device).reshape(T, B, 4)
    band = None
    if all(d[4] is not None for d in dets):
        band = torch.tensor([[float(d[4][0] * d[4][0]), float(d[4][1] * d[4][1])] for d in dets], dtype=torch.float32, device=device)
    rank = np.full(max([1] + [c + 1 for c in class_list(cfg)]), -1, np.int32)     # the output follows the class list's order
    for i, c in enumerate(class_list(cfg)):
        if c >= 0:
            rank[c] = i
    mode = cfg.TEST.get("SPECIAL_NMS", "none")
    aux = float(cfg.MODEL.get("RETINANET", {}).get("INFERENCE_TH", 0.05)) if mode == "soft-vote" else 0.0
    if mode == "soft-vote" and cfg.TEST.TH > 0 and not aux > 0:
        raise ValueError(f"MODEL.RETINANET.INFERENCE_TH = {aux} must be > 0 for TEST.SPECIAL_NMS = 'soft-vote': at <= 0 the reference keeps "
                         "every member of a cluster beside the merged row, more rows than the merge has room for")
    st = {} if stats is not None else None
    boxes, scores, labels, n_out, ndrop = ops.tta_merge(packed, counts, tparam, band, torch.from_numpy(rank).to(device), float(cfg.TEST.TH),
                                                        int(cfg.TEST.PRE_NMS_TOP_N), mode=mode, aux=aux, row_cap=row_cap, stats=st,
                                                        nms_path=nms_path)
    ran = st is not None and "workspace_classes" in st          # (not with mq_ml_nms, nor at TEST.TH <= 0: no per-class step ran)
    nd = torch.cat([n_out, ndrop] + ([st["workspace_classes"]] if ran else [])).tolist()      # one read-back for all three
    if stats is not None:
        stats["workspace_classes"] = nd[2 * B] if ran else 0
    n_out, ndrop = nd[:B], nd[B:2 * B]
    if sum(ndrop) and not _WARNED_CLASSES:
        _WARNED_CLASSES = True
        warnings.warn(f"TTA merge dropped {sum(ndrop)} detection(s) whose labels are outside TEST.SELECT_CLASSES / range(1, TEST.NUM_CLASSES = "
                      f"{cfg.TEST.NUM_CLASSES}), as the reference's merge_result_from_multi_scales does")
    out = []
    for b, (w, h) in enumerate(orig_wh):
        bl = BoxList(boxes[b, :n_out[b]], (int(w), int(h)), mode="xyxy")
        bl.add_field("scores", scores[b, :n_out[b]])
        bl.add_field("labels", labels[b, :n_out[b]])
        out.append(bl)
    return out


def merge_result_from_multi_scales(boxlists, cfg, row_cap=None, stats=None, nms_path="auto"):
    """box_aug.py:166-206 under its own name: list[BoxList] (one per image: the detections of every transform, already concatenated in the
    image's original frame, fields "scores" and "labels") -> list[BoxList], merged per class by TEST.SPECIAL_NMS ('none', 'soft-nms', 'vote',
    'soft-vote') at TEST.TH and cut to TEST.PRE_NMS_TOP_N, on the device the boxes live on.  For a caller that keeps the reference's own
    im_detect_bbox_aug loop and swaps only the merge: it is `merge` with one identity transform."""
    if not len(boxlists):
        return []
    device = boxlists[0].bbox.device
    K = max(1, max(len(bl) for bl in boxlists))
    packed = torch.zeros(len(boxlists), K, 6, dtype=torch.float32, device=device)
    for b, bl in enumerate(boxlists):
        n = len(bl)
        if n:
            x = bl.convert("xyxy")
            packed[b, :n, :4] = x.bbox.to(device=device, dtype=torch.float32)
            packed[b, :n, 4] = bl.get_field("scores").to(device=device, dtype=torch.float32)
            packed[b, :n, 5] = bl.get_field("labels").to(device=device, dtype=torch.float32)
    wh = [tuple(bl.size) for bl in boxlists]
    return merge([(packed, [len(bl) for bl in boxlists], wh, False, None)], wh, cfg, device, row_cap=row_cap, stats=stats, nms_path=nms_path)


def check_supported(model):
    """Everything the call would refuse, checked before the first forward.  TEST.USE_MULTISCALE (the reference's protocol: every
    transform returns its un-suppressed candidates) lifts the refusal of the special merges and sizes the rows as transforms x levels x
    PRE_NMS_TOP_N against the 2^24 of the per-class merges."""
    from . import ops
    cfg = model.cfg
    candidates = bool(cfg.TEST.get("USE_MULTISCALE", False))
    nms = cfg.TEST.get("SPECIAL_NMS", "none")
    if nms not in ops.TTA_SPECIAL_MODES:
        raise ValueError(f"TEST.SPECIAL_NMS = {nms!r}: one of {sorted(ops.TTA_SPECIAL_MODES)}")
    if nms != "none" and not candidates:
        raise NotImplementedError(f"TEST.SPECIAL_NMS = {nms!r} is not implemented by the device TTA merge (only 'none') unless "
                                  "TEST.USE_MULTISCALE is set: the reference runs the special merges on un-suppressed candidates only")
    if cfg.get("GROUNDINGDINO", {}).get("enabled", False):
        raise NotImplementedError("test-time augmentation (TEST.USE_MULTISCALE) is implemented for MQ-GLIP only, not MQ-GroundingDINO")
    cl = class_list(cfg)
    if len(set(cl)) != len(cl):
        # the reference would return such a class's detections once per repetition; the device merge ranks rows by class-list position
        raise NotImplementedError(f"TEST.SELECT_CLASSES repeats a class ({cl}): not supported by the device TTA merge")
    from .modeling.pipeline import TIE_SLOTS
    transforms = len(cfg.TEST.SCALES) * (2 if cfg.TEST.FLIP else 1)
    if candidates:
        rows = transforms * CANDIDATE_LEVELS * int(cfg.MODEL.ATSS.PRE_NMS_TOP_N)
        if rows > ops.TTA_MERGE_MAX_ROWS_ANY:
            raise ValueError(f"TTA merge: {rows} candidate rows per image (transforms x {CANDIDATE_LEVELS} levels x MODEL.ATSS.PRE_NMS_TOP_N) "
                             f"exceed the {ops.TTA_MERGE_MAX_ROWS_ANY} the merge takes: lower MODEL.ATSS.PRE_NMS_TOP_N or the number of TEST.SCALES")
        return
    kd = int(cfg.MODEL.ATSS.DETECTIONS_PER_IMG)
    rows = transforms * (kd + int(cfg.MODEL.ATSS.get("TIE_SLOTS", TIE_SLOTS)))
    if cfg.TEST.TH > 0 and kd > 0 and rows > ops.TTA_MERGE_MAX_ROWS:
        raise ValueError(f"TTA merge: {rows} detection rows per image (transforms x (DETECTIONS_PER_IMG + TIE_SLOTS)) exceed the "
                         f"{ops.TTA_MERGE_MAX_ROWS} the merge's NMS takes: lower MODEL.ATSS.DETECTIONS_PER_IMG or the number of TEST.SCALES")


@torch.no_grad()
def im_detect_bbox_aug(model, images, device, captions=None, positive_map_label_to_token=None):
    """box_aug.py:12-63, reading model.cfg (TEST.USE_MULTISCALE True: the reference's protocol, un-suppressed candidates from every
    transform and any TEST.SPECIAL_NMS; False: post-NMS rows and 'none' only -- see the module docstring).  images: RGB PIL images (BBoxAugCollator) or HWC uint8 tensors / arrays.
    Every transform goes through `model(...)`, so vision-only evaluation (VISION_QUERY.MASK_DURING_INFERENCE, detector._masked_ids) applies
    to each of them with no code here."""
    check_supported(model)
    cfg = model.cfg
    device = torch.device(device)
    scales = list(cfg.TEST.SCALES)
    ranges = list(cfg.TEST.RANGES) if len(cfg.TEST.RANGES) == len(scales) else [None] * len(scales)
    timing = TIMING
    ev = (lambda: torch.cuda.Event(enable_timing=True)) if timing is not None else None
    spans = {"ingest": [], "forwards": [], "merge": []}

    def mark(kind, fn):
        if ev is None:
            return fn()
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        spans[kind].append((a, b))
        return r

    up = mark("ingest", lambda: Upload(images, device))
    orig_wh = [(w, h) for (h, w) in up.hw]
    saved = getattr(model, "use_hip_graph", None)
    if saved is not None:
        model.use_hip_graph = saved and USE_HIP_GRAPH
    dets = []
    try:
        for scale, rng in zip(scales, ranges):
            plain, flipped, sizes = mark("ingest", lambda: ingest(up, scale, cfg.TEST.MAX_SIZE, cfg, bool(cfg.TEST.FLIP)))
            wh = [(w, h) for (h, w) in sizes]
            for canvas, fl in ((plain, False), (flipped, True)):
                if canvas is None:
                    continue
                il = ImageList(canvas, sizes)
                res = mark("forwards", lambda: model(il) if captions is None else
                           model(il, captions=captions, positive_map=positive_map_label_to_token))
                dets.append((model.last_packed, [len(r) for r in res], wh, fl, rng))
    finally:
        if saved is not None:
            model.use_hip_graph = saved
    out = mark("merge", lambda: merge(dets, orig_wh, cfg, device))
    if int(up.err.item()):
        raise RuntimeError("mq_tta_ingest_fwd: a tile needed more input rows than its LDS window (coefficient tables and R disagree)")
    if timing is not None:
        torch.cuda.synchronize()
        timing.clear()
        for k, v in spans.items():
            timing[k] = sum(a.elapsed_time(b) for a, b in v)
    return out
