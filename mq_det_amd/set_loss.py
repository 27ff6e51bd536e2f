"""The set criterion of MQ-GroundingDINO, evaluated forward-only on the device (csrc/set_loss.hip).

Reference: groundingdino_new/models/GroundingDINO/matcher.py HungarianMatcher (:49-86) and loss.py SetCriterion (:42-178).  The reference copies
a dense cost matrix to the host and runs scipy's linear_sum_assignment per image, once per decoder layer; here the cost, the assignment of
every (layer, image) problem and the loss sums are three launches and no device->host transfer.  This is NOT a training mode: there is no
autograd and `model.train()` keeps raising.  What it serves: choosing between checkpoints by held-out loss (`evaluate_loss`), and handing the
reference's own trainer its matching (`hungarian_match` in place of `self.matcher(...)`).

  validate_set_loss_config(cfg)                                  NotImplementedError, naming the key, for what this path does not restate
  hungarian_match(outputs, targets, positive_map, cfg)           -> per layer the reference's [(index_i, index_j)] per image
  SetCriterionLoss(cfg)(outputs, targets, text_mask, positive_map) -> the reference's weighted loss dict + the raw sums and the matching

Layers: `outputs["aux_outputs"]` are decoder layers 0 .. L - 2 and `outputs` itself is the last one; tensors stacked [L, ...] are in that order.
"""
import torch

from . import ops
from .losses import _upload, _world

SUM_NAMES = ("sum_token", "sum_l1", "sum_giou")


def validate_set_loss_config(cfg):
    """Raise NotImplementedError, naming the key, for every setting of the reference's criterion this path does not evaluate."""
    gd = cfg.GROUNDINGDINO
    m = gd.get("matcher", {})
    mt = m.get("matcher_type", gd.get("matcher_type", "HungarianMatcher"))
    if mt != "HungarianMatcher":
        raise NotImplementedError(f"GROUNDINGDINO.matcher.matcher_type = {mt!r}: the device criterion restates HungarianMatcher only")
    vq = cfg.VISION_QUERY
    if vq.get("ENABLED", False) and not vq.get("CONDITION_GATE", False):
        raise NotImplementedError("VISION_QUERY.CONDITION_GATE = False with VISION_QUERY.ENABLED: the reference's gate term indexes a module "
                                  "there; loss_gate is restated for the conditional gates only")
    if vq.get("ENABLED", False) and vq.get("CONDITION_GATE", False) and not vq.get("NONLINEAR_GATE", True):
        raise NotImplementedError("VISION_QUERY.NONLINEAR_GATE = False: loss_gate is restated for the ff_gate parameters only")
    if vq.get("ENABLED", False) and float(vq.get("FIX_ATTN_GATE", -1.0)) != -1.0:
        raise NotImplementedError(f"VISION_QUERY.FIX_ATTN_GATE = {vq.FIX_ATTN_GATE}: the blocks have no ff_gate then and the reference's gate term "
                                  "(bertwarper.py get_gate_value) raises; loss_gate is restated for learned gates only")
    fc = cfg.MODEL.DYHEAD.FUSE_CONFIG
    if float(fc.get("TOKEN_GAMMA", 2.0)) <= 0:
        raise NotImplementedError(f"MODEL.DYHEAD.FUSE_CONFIG.TOKEN_GAMMA = {fc.TOKEN_GAMMA}: a positive exponent")
    if all(float(m.get(k, 1.0)) == 0 for k in ("set_cost_class", "set_cost_bbox", "set_cost_giou")):
        raise NotImplementedError("GROUNDINGDINO.matcher.set_cost_*: all three are 0 (the reference asserts)")


def _coefficients(cfg):
    gd = cfg.GROUNDINGDINO
    m = gd.get("matcher", {})
    return {"cost_class": float(m.get("set_cost_class", 1.0)), "cost_bbox": float(m.get("set_cost_bbox", 5.0)),
            "cost_giou": float(m.get("set_cost_giou", 2.0)), "focal_alpha": float(m.get("focal_alpha", gd.get("focal_alpha", 0.25)))}


def _normed_cxcywh(t):
    """The target's 'normed_cxcy_boxes' field, or what the reference's dataset derives (modulated_coco_new.py:269-275): xyxy / (w, h, w, h)
    of the BoxList's size, as centre and extent."""
    if not (hasattr(t, "bbox") and hasattr(t, "fields") and hasattr(t, "size")):
        raise ValueError(f"targets: BoxLists expected, got {type(t).__name__}")
    if "normed_cxcy_boxes" in t.fields():
        return t.get_field("normed_cxcy_boxes").reshape(-1, 4).float()
    if t.mode != "xyxy":
        raise ValueError(f"targets: BoxLists in 'xyxy' mode (or with a 'normed_cxcy_boxes' field) expected, got '{t.mode}'")
    w, h = t.size
    b = t.bbox.reshape(-1, 4).float() / torch.tensor([[w, h, w, h]], dtype=torch.float32, device=t.bbox.device)
    return torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], -1)


def _pack(targets, positive_map, device):
    """-> (gt [G, 4] fp32, posmap [G, Tpm] fp32, gt_off [B + 1] int32 on the device, host counts).  No device->host transfer."""
    if not isinstance(targets, (list, tuple)) or len(targets) == 0:
        raise ValueError("targets: a non-empty list of BoxLists, one per image")
    boxes = [_normed_cxcywh(t) for t in targets]
    counts = [int(b.shape[0]) for b in boxes]
    total = sum(counts)
    if not torch.is_tensor(positive_map) or positive_map.dim() != 2 or positive_map.shape[0] != total:
        raise ValueError(f"positive_map: a [{total}, T] tensor expected (one row per gt box of the batch, image after image)")
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    gt = _upload(torch.cat(boxes).contiguous(), device)
    pm = _upload(positive_map.float().contiguous(), device)
    return gt, pm, _upload(torch.tensor(offs, dtype=torch.int32), device), counts


def _stack_outputs(outputs):
    """the reference's dict -> logits [L, B, nq, T] and boxes [L, B, nq, 4] fp32: aux layers first, the main output last"""
    layers = list(outputs.get("aux_outputs", ())) + [outputs]
    logits = torch.stack([o["pred_logits"].float() for o in layers]).contiguous()
    boxes = torch.stack([o["pred_boxes"].float() for o in layers]).contiguous()
    if logits.dim() != 4 or boxes.shape != (*logits.shape[:3], 4):
        raise ValueError(f"outputs: pred_logits {tuple(logits.shape[1:])} / pred_boxes {tuple(boxes.shape[1:])} per layer")
    return logits, boxes


def _check_counts(counts, nq):
    if nq > ops.HUNGARIAN_MAX_QUERIES:
        raise NotImplementedError(f"set criterion: {nq} queries, the assignment kernel takes {ops.HUNGARIAN_MAX_QUERIES}")
    if max(counts) > nq:
        raise ValueError(f"set criterion: an image with {max(counts)} gt boxes for {nq} queries (every gt needs a query of its own)")


def match(logits, boxes, gt, pm, gt_off, counts, coef):
    """cost + assignment of every (layer, image): -> (match_q [L, G], q2g [L, B, nq]) int32 on the device"""
    _check_counts(counts, logits.shape[2])                        # by count, before any launch
    cost = ops.set_cost(logits, boxes, gt, pm, gt_off, **coef)
    return ops.hungarian(cost, gt_off, counts)


@torch.no_grad()
def hungarian_match(outputs, targets, positive_map, cfg, host=False):
    """HungarianMatcher.forward for the main output and every aux output: -> a list of L entries (aux layers 0 .. L - 2, then the main output),
    each the reference's list per image of (index_i, index_j) int64 tensors sorted by query index -- what a reference trainer splices in place
    of `self.matcher(...)`.  On the device, no device->host transfer, unless `host` asks for host tensors."""
    validate_set_loss_config(cfg)
    logits, boxes = _stack_outputs(outputs)
    gt, pm, gt_off, counts = _pack(targets, positive_map, logits.device)
    match_q, _ = match(logits, boxes, gt, pm, gt_off, counts, _coefficients(cfg))
    if host:
        match_q = match_q.cpu()
    out = []
    for l in range(logits.shape[0]):
        per_image, off = [], 0
        for c in counts:
            qi, order = torch.sort(match_q[l, off:off + c].long())
            per_image.append((qi, order))
            off += c
        out.append(per_image)
    return out


def matching_from_indices(indices, counts, nq, device):
    """The inverse of `hungarian_match`'s return format: -> (match_q [L, G], q2g [L, B, nq]) int32"""
    L, B, G = len(indices), len(counts), sum(counts)
    match_q = torch.full((L, max(G, 0)), -1, dtype=torch.int32)
    q2g = torch.full((L, B, nq), -1, dtype=torch.int32)
    for l in range(L):
        off = 0
        for b, c in enumerate(counts):
            qi, gj = (torch.as_tensor(x).long().cpu() for x in indices[l][b])
            match_q[l, off + gj] = qi.int()
            q2g[l, b, qi] = gj.int()
            off += c
    return _upload(match_q, device), _upload(q2g, device)


class SetCriterionLoss:
    """SetCriterion.forward (loss.py:114-178) with `losses = ['labels', 'boxes']`: -> the reference's dict (`loss_ce`, `loss_bbox`, `loss_giou`
    and `loss_*_{i}` of the aux layers, weighted by loss_ce_coef / loss_bbox_coef / loss_giou_coef), plus `sums` [L, 3] (SUM_NAMES, raw),
    `num_boxes` (the batch's gt count, a host int), `match_q` [L, G] and `q2g` [L, B, nq].  Everything but `num_boxes` stays on the device."""

    def __init__(self, cfg):
        validate_set_loss_config(cfg)
        self.cfg = cfg
        gd, fc = cfg.GROUNDINGDINO, cfg.MODEL.DYHEAD.FUSE_CONFIG
        self.coef = (float(gd.get("loss_ce_coef", 2.0)), float(gd.get("loss_bbox_coef", 5.0)), float(gd.get("loss_giou_coef", 2.0)))
        self.alpha, self.gamma = float(fc.get("TOKEN_ALPHA", 0.25)), float(fc.get("TOKEN_GAMMA", 2.0))

    @torch.no_grad()
    def __call__(self, outputs, targets, text_mask, positive_map, indices=None):
        """`indices`: a matching in `hungarian_match`'s format to evaluate instead of the device's own."""
        validate_set_loss_config(self.cfg)                        # before the first launch, and again if the cfg was edited since
        logits, boxes = _stack_outputs(outputs)
        dev = logits.device
        L, B, nq, T = logits.shape
        gt, pm, gt_off, counts = _pack(targets, positive_map, dev)
        if len(counts) != B or text_mask.dim() != 2 or text_mask.shape[0] != B or text_mask.shape[1] < T:
            raise ValueError(f"set criterion: {B} images of {T} text positions, {len(counts)} targets, text_mask {tuple(text_mask.shape)}")
        mask = _upload(text_mask[:, :T].to(torch.int32).contiguous(), dev)
        if indices is None:
            match_q, q2g = match(logits, boxes, gt, pm, gt_off, counts, _coefficients(self.cfg))
        else:
            _check_counts(counts, nq)
            match_q, q2g = matching_from_indices(indices, counts, nq, dev)
        sums = ops.set_loss(logits, boxes, gt, pm, gt_off, mask, q2g, match_q, self.alpha, self.gamma)
        out = self.losses_from_sums(sums, sum(counts))
        out.update(sums=sums, num_boxes=sum(counts), match_q=match_q, q2g=q2g)
        return out

    def losses_from_sums(self, sums, total_gt):
        """The reference's normalisation and weighting loop: num_boxes = max(all-reduced gt count / world, 1); `name in k` (loss.py:166-171)."""
        world = _world()
        n = torch.tensor([float(total_gt)], dtype=torch.float32, device=sums.device)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(n)
        n = (n / world).clamp(min=1.0)[0]
        L = sums.shape[0]
        out = {}
        for l in range(L):
            sfx = "" if l == L - 1 else f"_{l}"
            for j, name in enumerate(("loss_ce", "loss_bbox", "loss_giou")):
                out[name + sfx] = sums[l, j] / n * self.coef[j]
        return out


@torch.no_grad()
def evaluate_set_loss(model, data_loader, device="cuda"):
    """Dataset means of the set criterion from the raw sums (`mq_det_amd.evaluate_loss` dispatches here for MQ-GroundingDINO): the sums of
    all batches are added on the device and normalised once by max(all gts / world, 1), then weighted as the reference's loop does.  A batch
    is (images, targets, ...); captions and positive maps come from the targets' 'caption' / 'positive_map' fields.  ONE device->host
    transfer, at the end.  -> dict of floats with the reference's keys (+ 'loss_gate' with vision queries, 'num_boxes', 'batches')."""
    model.eval()
    crit = SetCriterionLoss(model.cfg)
    total, boxes, n, gate = None, 0, 0, None
    for batch in data_loader:
        images, targets = batch[0], batch[1]
        out = model.forward_losses(images.to(device) if hasattr(images, "to") else images, targets)
        total = out["sums"].double() if total is None else total + out["sums"].double()
        boxes += int(out["num_boxes"])                            # a host count: the targets' lengths
        gate = out.get("loss_gate", gate)
        n += 1
    if total is None:
        raise ValueError("evaluate_loss: the data loader yielded no batch")
    world = _world()
    cnt = torch.tensor([float(boxes)], dtype=torch.float64, device=total.device)
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(total)
        dist.all_reduce(cnt)
    flat = torch.cat([total.reshape(-1), cnt] + ([gate.double().reshape(1)] if gate is not None else [])).tolist()   # the one transfer
    L = total.shape[0]
    num = max(flat[3 * L] / world, 1.0)
    res = {}
    for l in range(L):
        sfx = "" if l == L - 1 else f"_{l}"
        for j, name in enumerate(("loss_ce", "loss_bbox", "loss_giou")):
            res[name + sfx] = flat[3 * l + j] / world / num * crit.coef[j]
    if gate is not None:
        res["loss_gate"] = flat[-1]
    res.update(num_boxes=boxes, batches=n)
    return res
